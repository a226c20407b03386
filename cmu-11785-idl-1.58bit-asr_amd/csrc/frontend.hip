// frontend.hip — Kaldi fbank + CMVN + SpecAugment + zero-padded collate of a padded batch of
// 16 kHz waveforms, one launch (the definition: include/onebit_hip.h, ob_frontend_fwd).
//
// Reference: src/data/dataset.py:117-135 computes torchaudio.compliance.kaldi.fbank per
// utterance on the host, normalises, masks (:150-209) and the collate pads (:245-273).
//
// Layout. A block of 4 waves owns kFPB = 16 consecutive frames of one utterance and stages
// their contiguous sample span (400 + 160 * 15 = 2800 floats: neighbouring frames share 240
// samples, so a sample is read from HBM once per block, 1.17x overall) and the sparse mel
// weights (512 floats) in LDS. Each wave then takes 4 frames, one after the other:
//   - DC mean: 7 strided reads per lane, xor-butterfly reduction (fixed order);
//   - pre-emphasis + window into z[n] = y[2n] + i y[2n+1], n = lane + 64 r, as one 8-byte LDS
//     read per point: exactly the operands of lane's first radix-4 butterfly;
//   - 256-point complex FFT, radix-4 Stockham, one butterfly per lane and stage; stages 1-3
//     exchange through the wave's own LDS buffer (in-wave: no block barrier), the first reads
//     and the last writes registers;
//   - split step to the 512-point real spectrum (one more exchange for Z[256 - k]), power into
//     LDS;
//   - one lane per mel filter walks its contiguous bins (ascending, fp32), log, CMVN, masks,
//     and the row goes out as one coalesced store. Bin 256 has no weight and is not computed.
// Window, twiddles and filter descriptors sit in registers for the wave's four frames (read
// once from the table); no sincosf/powf here. Frames >= m, pad rows and time-masked frames
// are stored as zeros without computing. No atomics: run-to-run bitwise reproducible.
#include <cmath>

#include "ob_launch.h"

namespace ob {

namespace {

constexpr int kFrameLen = 400, kFrameShift = 160, kFft = 512, kHalf = 256;
constexpr int kWaves = 4, kFramesPerWave = 4, kFPB = kWaves * kFramesPerWave;
constexpr int kSpan = kFrameLen + kFrameShift * (kFPB - 1);
constexpr int kMaxWeights = 512;  // a bin has at most two filters: <= 510 in use
constexpr int kTabWindow = 0, kTabTwiddle = kFrameLen, kTabFilters = kTabTwiddle + 2 * kFft;
constexpr float kLogFloor = 1.1920929e-07f;

__device__ __forceinline__ void wave_sync() {
  // orders this wave's LDS writes before its later LDS reads (other lanes' data)
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
  __builtin_amdgcn_wave_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
}

struct Cx {
  float r, i;
};
__device__ __forceinline__ Cx cmul(Cx a, Cx w) { return {a.r * w.r - a.i * w.i, a.r * w.i + a.i * w.r}; }

// forward radix-4 DFT of v[0..3] in place
__device__ __forceinline__ void dft4(Cx v[4]) {
  const Cx a0 = {v[0].r + v[2].r, v[0].i + v[2].i}, a1 = {v[0].r - v[2].r, v[0].i - v[2].i};
  const Cx a2 = {v[1].r + v[3].r, v[1].i + v[3].i};
  const Cx a3 = {v[1].i - v[3].i, v[3].r - v[1].r};  // -i (v1 - v3)
  v[0] = {a0.r + a2.r, a0.i + a2.i};
  v[1] = {a1.r + a3.r, a1.i + a3.i};
  v[2] = {a0.r - a2.r, a0.i - a2.i};
  v[3] = {a1.r - a3.r, a1.i - a3.i};
}

__global__ __launch_bounds__(64 * kWaves) void fbank_kernel(
    const float* __restrict__ wave, int64_t wave_stride, const int64_t* __restrict__ wave_lens,
    int64_t n_max, const float* __restrict__ table, int n_mels, const float* __restrict__ cmvn_mean,
    const float* __restrict__ cmvn_std, const int* __restrict__ mask_starts, int n_fmask,
    int fmask_w, int n_tmask, int tmask_w, float* __restrict__ feats, int64_t T, int chunks,
    int64_t* __restrict__ feat_lens) {
  __shared__ __attribute__((aligned(16))) float s_x[kSpan];
  __shared__ float s_w[kMaxWeights];
  __shared__ float s_re[kWaves][kHalf], s_im[kWaves][kHalf], s_p[kWaves][kHalf];

  const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
  const int64_t b = blockIdx.x / chunks;
  const int64_t f0 = (int64_t)(blockIdx.x % chunks) * kFPB;
  int64_t n = wave_lens[b];
  n = n < 0 ? 0 : (n > n_max ? n_max : n);
  const int64_t m = n < kFrameLen ? 0 : 1 + (n - kFrameLen) / kFrameShift;
  if (f0 == 0 && tid == 0) feat_lens[b] = m;
  const int rows = (int)(T - f0 < kFPB ? T - f0 : kFPB);  // rows of feats this block owns
  float* out = feats + (b * T + f0) * n_mels;
  if (f0 >= m) {  // pad rows only
    for (int i = tid; i < rows * n_mels; i += 64 * kWaves) out[i] = 0.0f;
    return;
  }
  const int live = (int)(m - f0 < kFPB ? m - f0 : kFPB);  // frames to compute, >= 1
  {
    // frame f0 + live - 1 ends at 160 (f0 + live - 1) + 400 <= 160 (m - 1) + 400 <= n
    const int need = kFrameLen + kFrameShift * (live - 1);
    const float* src = wave + b * wave_stride + f0 * kFrameShift;
    for (int i = tid; i < need; i += 64 * kWaves) s_x[i] = src[i];
    const float* wts = table + kTabFilters + 3 * n_mels;
    for (int i = tid; i < kMaxWeights; i += 64 * kWaves) s_w[i] = wts[i];
  }

  // per-lane constants, kept for the wave's frames
  float win[8];  // window[2n], window[2n+1] for n = lane + 64 r
  Cx tw[3][3];   // stage s+1, operand r+1: W256^((r+1) * (lane % 4^(s+1)) * 64 / 4^(s+1))
  Cx ts[4];      // split step: W512^(lane + 64 r)
  const float2* twid = reinterpret_cast<const float2*>(table + kTabTwiddle);
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int j = 2 * (lane + 64 * r);
    win[2 * r] = j < kFrameLen ? table[kTabWindow + j] : 0.0f;
    win[2 * r + 1] = j < kFrameLen ? table[kTabWindow + j + 1] : 0.0f;
    const float2 t = twid[lane + 64 * r];
    ts[r] = {t.x, t.y};
  }
#pragma unroll
  for (int s = 0; s < 3; ++s) {
    const int ns = 4 << (2 * s);  // 4, 16, 64
    const int k = lane & (ns - 1);
#pragma unroll
    for (int r = 0; r < 3; ++r) {
      const float2 t = twid[2 * ((r + 1) * k * (64 / ns))];  // W256^e = W512^(2e), 2e <= 378
      tw[s][r] = {t.x, t.y};
    }
  }
  int f_first[2], f_count[2], f_off[2];
  float c_mean[2], c_std[2];
  bool f_masked[2];
  const int wf = fmask_w < n_mels ? fmask_w : n_mels;
  const int* starts = mask_starts ? mask_starts + b * (n_fmask + n_tmask) : nullptr;
#pragma unroll
  for (int h = 0; h < 2; ++h) {
    const int f = lane + 64 * h;
    f_first[h] = f_count[h] = f_off[h] = 0;
    c_mean[h] = 0.0f;
    c_std[h] = 1.0f;
    f_masked[h] = false;
    if (f < n_mels) {
      const float* d = table + kTabFilters + 3 * f;
      f_first[h] = (int)d[0];
      f_count[h] = (int)d[1];
      f_off[h] = (int)d[2];
      if (cmvn_mean) {
        c_mean[h] = cmvn_mean[f];
        c_std[h] = cmvn_std[f];
      }
      if (starts)
        for (int q = 0; q < n_fmask; ++q) f_masked[h] |= f >= starts[q] && f - starts[q] < wf;
    }
  }
  const int64_t wt = tmask_w < m ? tmask_w : m;
  __syncthreads();

  float* re = s_re[wv];
  float* im = s_im[wv];
  float* pw = s_p[wv];
  for (int q = 0; q < kFramesPerWave; ++q) {
    const int fl = wv * kFramesPerWave + q;  // frame within the block (wave-uniform)
    if (fl >= rows) break;
    float* row = out + fl * n_mels;
    bool zero = fl >= live;
    if (!zero && starts) {
      const int64_t f = f0 + fl;
      for (int t = 0; t < n_tmask; ++t) {
        const int64_t st = starts[n_fmask + t];
        zero |= f >= st && f - st < wt;
      }
    }
    if (zero) {
      for (int f = lane; f < n_mels; f += 64) row[f] = 0.0f;
      continue;
    }
    const float* x = s_x + fl * kFrameShift;
    float sum = 0.0f;
#pragma unroll
    for (int r = 0; r < 7; ++r) {
      const int j = lane + 64 * r;
      if (j < kFrameLen) sum += x[j];
    }
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);
    const float mean = sum / (float)kFrameLen;

    Cx v[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int j = 2 * (lane + 64 * r);
      v[r] = {0.0f, 0.0f};
      if (j < kFrameLen) {
        const float2 p = *reinterpret_cast<const float2*>(x + j);  // x is 8-byte aligned at even j
        const float x0 = p.x - mean, x1 = p.y - mean;
        const float xm = j > 0 ? x[j - 1] - mean : x0;
        v[r] = {(x0 - 0.97f * xm) * win[2 * r], (x1 - 0.97f * x0) * win[2 * r + 1]};
      }
    }
    // radix-4 Stockham: stage s reads in[lane + 64 r], writes out[(lane / ns) * 4 ns + lane % ns
    // + r ns]; stage 0 (ns = 1) has unit twiddles and its inputs are already in v
    dft4(v);
    wave_sync();  // the previous frame's reads of re/im/pw are done
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      re[4 * lane + r] = v[r].r;
      im[4 * lane + r] = v[r].i;
    }
#pragma unroll
    for (int s = 0; s < 3; ++s) {
      const int ns = 4 << (2 * s);
      wave_sync();
#pragma unroll
      for (int r = 0; r < 4; ++r) v[r] = {re[lane + 64 * r], im[lane + 64 * r]};
#pragma unroll
      for (int r = 1; r < 4; ++r) v[r] = cmul(v[r], tw[s][r - 1]);
      dft4(v);
      wave_sync();
      if (s < 2) {
        const int j0 = (lane / ns) * (4 * ns) + (lane & (ns - 1));
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          re[j0 + r * ns] = v[r].r;
          im[j0 + r * ns] = v[r].i;
        }
      } else {  // ns = 64: Z[lane + 64 r] = v[r], also kept in registers
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          re[lane + 64 * r] = v[r].r;
          im[lane + 64 * r] = v[r].i;
        }
      }
    }
    wave_sync();
    // X[k] = E[k] + W512^k O[k], E = (Z[k] + conj Z[256-k]) / 2, O = (Z[k] - conj Z[256-k]) / 2i
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int k = lane + 64 * r;
      const int kc = (kHalf - k) & (kHalf - 1);
      const float cr = re[kc], ci = im[kc];
      const float er = 0.5f * (v[r].r + cr), ei = 0.5f * (v[r].i - ci);
      const float orr = 0.5f * (v[r].i + ci), oi = -0.5f * (v[r].r - cr);
      const float xr = er + ts[r].r * orr - ts[r].i * oi;
      const float xi = ei + ts[r].r * oi + ts[r].i * orr;
      pw[k] = xr * xr + xi * xi;
    }
    wave_sync();
#pragma unroll
    for (int h = 0; h < 2; ++h) {
      const int f = lane + 64 * h;
      if (f < n_mels) {
        float e = 0.0f;
        for (int i = 0; i < f_count[h]; ++i) e += s_w[f_off[h] + i] * pw[f_first[h] + i];
        float val = logf(e > kLogFloor ? e : kLogFloor);
        if (cmvn_mean) val = (val - c_mean[h]) / c_std[h];
        row[f] = f_masked[h] ? 0.0f : val;
      }
    }
  }
}

double mel_of(double hz) { return 1127.0 * std::log(1.0 + hz / 700.0); }

}  // namespace

int64_t fbank_num_frames(int64_t n) {
  return n < kFrameLen ? 0 : 1 + (n - kFrameLen) / kFrameShift;
}

int64_t frontend_table_floats(int n_mels) {
  return kTabFilters + 3 * (int64_t)n_mels + kMaxWeights;
}

void frontend_table_fill(float* t, int n_mels) {
  const double pi = 3.14159265358979323846;
  for (int j = 0; j < kFrameLen; ++j)
    t[kTabWindow + j] =
        (float)std::pow(0.5 - 0.5 * std::cos(2.0 * pi * j / (kFrameLen - 1)), 0.85);
  for (int k = 0; k < kFft; ++k) {
    t[kTabTwiddle + 2 * k] = (float)std::cos(2.0 * pi * k / kFft);
    t[kTabTwiddle + 2 * k + 1] = (float)-std::sin(2.0 * pi * k / kFft);
  }
  float* desc = t + kTabFilters;
  float* wts = desc + 3 * n_mels;
  for (int i = 0; i < kMaxWeights; ++i) wts[i] = 0.0f;
  const double lo = mel_of(20.0), hi = mel_of(8000.0), d = (hi - lo) / (n_mels + 1);
  int off = 0;
  for (int f = 0; f < n_mels; ++f) {
    const double left = lo + f * d, centre = lo + (f + 1) * d, right = lo + (f + 2) * d;
    int first = 0, count = 0;
    for (int k = 0; k < kHalf; ++k) {
      const double mk = mel_of(k * (16000.0 / kFft));
      const double up = (mk - left) / (centre - left), down = (right - mk) / (right - centre);
      const double w = std::fmax(0.0, std::fmin(up, down));
      if (w > 0.0 && off + count < kMaxWeights) {  // a bin has at most two filters: <= 510
        if (count == 0) first = k;
        wts[off + count++] = (float)w;
      }
    }
    desc[3 * f] = (float)first;
    desc[3 * f + 1] = (float)count;
    desc[3 * f + 2] = (float)off;
    off += count;
  }
}

int64_t frontend_blocks(int64_t B, int64_t T) {
  const int64_t chunks = T > 0 ? ceil_div(T, kFPB) : 1;
  return B * chunks;
}

void launch_frontend(const float* wave, int64_t wave_stride, const int64_t* wave_lens, int64_t B,
                     int64_t n_max, const float* table, int n_mels, const float* cmvn_mean,
                     const float* cmvn_std, const int* mask_starts, int n_fmask, int fmask_w,
                     int n_tmask, int tmask_w, float* feats, int64_t T, int64_t* feat_lens,
                     hipStream_t s) {
  if (B == 0) return;
  const int chunks = (int)(T > 0 ? ceil_div(T, kFPB) : 1);
  hipLaunchKernelGGL(fbank_kernel, dim3((unsigned)(B * chunks)), dim3(64 * kWaves), 0, s, wave,
                     wave_stride, wave_lens, n_max, table, n_mels, cmvn_mean, cmvn_std,
                     mask_starts, n_fmask, fmask_w, n_tmask, tmask_w, feats, T, chunks, feat_lens);
}

}  // namespace ob
