// rescore.hip — the second pass of two-pass decoding: score the CTC n-best (beam.hip) with the
// attention decoder under teacher forcing and pick the best combined hypothesis.
//
//   prepare   hyp / hyp_len / n_hyp -> the decoder's inputs at a static length Lc:
//             tgt_inp [B*N][Lc+1] = bos, y_1..y_n, pad...; target = y_1..y_n, eos, -1...;
//             tgt_pad; ok[b] = 0 when a live hypothesis of utterance b is longer than Lc
//   scorer    lp[r] = (h_r . W[tgt_r] + b[tgt_r]) - logsumexp_v(h_r . W[v] + b[v]) for the
//             decoder's hidden rows h [R][d] and its output layer W [V][d], without the [R][V]
//             logits: only a (max, sum of exp) pair per (row, 64-column tile) leaves the GEMM
//   select    att[b][k] = sum of lp over hypothesis k's len+1 rows (fp64, ascending position),
//             total = att + ctc_weight * ctc_score, winner = largest total (ties: smaller k)
//
// Scorer arithmetic: the products are exact fp32 on the bf16 matrix cores (ob_mma.h): both
// operands split into three bf16 planes (x = hi + mid + lo), six v_mfma_f32_16x16x32_bf16 per
// k-step (mm, lh, hl, mh, hm, hh; the dropped terms are below 2^-25 |x||w|).
// Block = 4 waves and one 64-column tile of W, whose three-plane image ([64][3][dpad+8] bf16,
// the pad keeps the B-fragment ds_read_b128 conflict-free) is built once in LDS; the block
// then walks its share of the 16-row subtiles of h, one subtile per wave at a time. A subtile
// whose 16 targets are all -1 is skipped before its rows are loaded, and a block whose whole
// row share is skipped returns before it reads W. Per row and tile: m = max of the tile's
// valid logits, s = sum exp(x - m) (fp32, fixed order: the 4 column fragments of a lane, then
// an xor butterfly over the 16 lanes of a row), and the target's logit from the one lane that
// holds it. The merge kernel (one wave per row) takes the tiles in index order: M = max m,
// S = sum s * exp(m - M) in fp64, lp = x_tgt - (M + log S). No atomics: every word has one
// writer and every sum a fixed order, so results are bitwise reproducible.
//
// Fragment map of v_mfma_f32_16x16x32_bf16 (lane l, r = l&15, g = l>>4):
//   A[i=r][kk=8g+j] (j<8), B[kk=8g+j][col=r], D[row=4g+reg][col=r].
#include <math.h>

#include <algorithm>

#include "ob_launch.h"
#include "ob_scorer.h"

namespace ob {

namespace {

using namespace scorer;  // the shared exact-fp32 tile (ob_scorer.h)

__global__ __launch_bounds__(64 * kScWaves) void seq_logprob_tile_kernel(
    const float* __restrict__ Hd, int64_t R, int K, const float* __restrict__ W, int V,
    const float* __restrict__ bias, const int* __restrict__ tgt, int n_ct, int n16, int rgroups,
    float2* __restrict__ part, float* __restrict__ tl) {
  constexpr int kThr = 64 * kScWaves;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* bimg = reinterpret_cast<__bf16*>(smem);
  const int kpad = sc_kpad(K);
  const int stride = kpad + 8;    // bf16 per plane row
  const int cpitch = 3 * stride;  // bf16 per image column (three planes)
  const int ct = blockIdx.x % n_ct;
  const int rg = blockIdx.x / n_ct;
  const int n0 = ct * kScBN;
  // this block's 16-row subtiles [s0, s1), dealt round-robin to its waves
  const int s0 = (int)((int64_t)rg * n16 / rgroups), s1 = (int)((int64_t)(rg + 1) * n16 / rgroups);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int kg = 8 * g;

  // nothing to score in this block's rows: leave before W is read
  {
    const int64_t lo = (int64_t)16 * s0, hi = (int64_t)16 * s1 < R ? (int64_t)16 * s1 : R;
    int any = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThr) any |= tgt[i] >= 0;
    if (!__syncthreads_or(any)) return;
  }

  sc_build_image(bimg, W, K, V, n0);
  __syncthreads();

  const __bf16* brow = bimg + r * cpitch + kg;
  float bcol[kScNT];
  bool cvalid[kScNT];
#pragma unroll
  for (int t = 0; t < kScNT; ++t) {
    const int col = n0 + 16 * t + r;
    cvalid[t] = col < V;
    bcol[t] = (bias && cvalid[t]) ? bias[col] : 0.0f;
  }

  for (int j = s0 + wave; j < s1; j += kScWaves) {
    const int64_t m0 = (int64_t)16 * j;
    // the subtile's targets: lane (r, g) holds row m0 + r's; all -1 -> no load, no work
    const int t_r = m0 + r < R ? tgt[m0 + r] : -1;
    if (__ballot(t_r >= 0) == 0ull) continue;
    const int64_t arow_i = m0 + r < R ? m0 + r : R - 1;
    const float* arow = Hd + arow_i * (int64_t)K;

    f32x4 acc[kScNT];
    sc_subtile_mma(arow, brow, K, kg, acc);

    // D[row = 4g + reg][col = r]: per row the tile's max, sum of exp and the target's logit
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = m0 + 4 * g + reg;
      const int tg = __shfl(t_r, 4 * g + reg);  // lane (r' = 4g + reg, g' = 0) holds it
      float x[kScNT];
      float m = -INFINITY;
#pragma unroll
      for (int t = 0; t < kScNT; ++t) {
        x[t] = acc[t][reg] + bcol[t];
        if (cvalid[t]) m = fmaxf(m, x[t]);
      }
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < kScNT; ++t) s += cvalid[t] ? expf(x[t] - m) : 0.0f;
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o);  // the same bits in all 16 lanes
      if (row < R && tg >= 0) {
#pragma unroll
        for (int t = 0; t < kScNT; ++t)
          if (n0 + 16 * t + r == tg) tl[row] = x[t];
        if (r == 0) part[row * n_ct + ct] = make_float2(m, s);
      }
    }
  }
}

// one wave per row: the tiles' (m, s) pairs in index order
__global__ __launch_bounds__(256) void seq_logprob_merge_kernel(
    const float2* __restrict__ part, const float* __restrict__ tl, const int* __restrict__ tgt,
    int64_t R, int V, int n_ct, float* __restrict__ lp) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  const int tg = tgt[row];
  if (tg < 0 || tg >= V) {  // skipped row: 0; a target outside the vocabulary: NaN
    if (lane == 0) lp[row] = tg < 0 ? 0.0f : __int_as_float(0x7fc00000);
    return;
  }
  const float2* p = part + row * n_ct;
  float M = -INFINITY;
  for (int c = lane; c < n_ct; c += 64) M = fmaxf(M, p[c].x);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
  double S = 0.0;
  for (int c = lane; c < n_ct; c += 64) {
    const float2 v = p[c];
    S += (double)v.y * exp((double)v.x - (double)M);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) S += __shfl_xor(S, o);  // the same bits in every lane
  if (lane == 0) lp[row] = (float)((double)tl[row] - ((double)M + log(S)));
}

// block = utterance; threads over its N * (Lc + 1) positions
__global__ __launch_bounds__(256) void rescore_prepare_kernel(
    const int* __restrict__ hyp, const int* __restrict__ hyp_len, const int* __restrict__ n_hyp,
    int N, int T, int Lc, int bos, int eos, int pad, int64_t* __restrict__ tgt_inp,
    int* __restrict__ target, uint8_t* __restrict__ tgt_pad, uint8_t* __restrict__ ok) {
  const int b = blockIdx.x;
  int nh = n_hyp[b];
  nh = nh < 0 ? 0 : (nh > N ? N : nh);
  bool fits = true;
  for (int k = 0; k < nh; ++k) fits = fits && hyp_len[(int64_t)b * N + k] <= Lc;
  if (threadIdx.x == 0) ok[b] = fits ? 1 : 0;
  const int L1 = Lc + 1;
  for (int e = threadIdx.x; e < N * L1; e += blockDim.x) {
    const int k = e / L1, j = e - k * L1;
    const int64_t hk = (int64_t)b * N + k;
    const bool live = fits && k < nh;  // (an utterance that does not fit is not rescored)
    int len = live ? hyp_len[hk] : 0;
    len = len < 0 ? 0 : (len > T ? T : len);
    const int* y = hyp + hk * T;
    const int64_t o = hk * L1 + j;
    tgt_inp[o] = j == 0 ? bos : (j <= len ? y[j - 1] : pad);
    target[o] = !live ? -1 : (j < len ? y[j] : (j == len ? eos : -1));
    tgt_pad[o] = j > len ? 1 : 0;
  }
}

// total = (a + w * c) + lw * l, the LM product and the last sum rounded on their own
__device__ __forceinline__ double lm_total(double base, double lw, double l) {
#pragma clang fp contract(off)
  const double pl = lw * l;
  return base + pl;
}

// w * c rounded, then the sum: the LM pick's (att + ctc_weight * ctc)
__device__ __forceinline__ double att_ctc_total(double a, double w, double c) {
#pragma clang fp contract(off)
  const double pc = w * c;
  return a + pc;
}

// block = utterance (one wave): lane k sums hypothesis k, lane 0 picks, all lanes copy.
// LM: the pick with an LM term; lp null = no attention pass (ok / att may be null too)
template <bool LM>
__global__ __launch_bounds__(64) void rescore_select_kernel(
    const float* __restrict__ lp, const int* __restrict__ hyp, const int* __restrict__ hyp_len,
    const int* __restrict__ n_hyp, const double* __restrict__ ctc, const uint8_t* __restrict__ ok,
    int N, int T, int Lc, double w, int* __restrict__ out, int* __restrict__ out_len,
    int* __restrict__ best_k, double* __restrict__ att, double* __restrict__ total,
    uint8_t* __restrict__ rescored, const double* __restrict__ lm, double lw) {
  __shared__ double s_tot[64];
  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  int nh = n_hyp[b];
  nh = nh < 0 ? 0 : (nh > N ? N : nh);
  const bool fits = (LM && !ok) ? true : ok[b] != 0;
  const double kNegInf = -(double)INFINITY;
  double tot = kNegInf;
  if (lane < N) {
    const int64_t hk = (int64_t)b * N + lane;
    double a = 0.0;
    if (fits && lane < nh) {
      int len = hyp_len[hk];
      len = len < 0 ? 0 : (len > Lc ? Lc : len);
      const float* row = lp + hk * (Lc + 1);
      if constexpr (LM) {
        if (lp) {
          for (int j = 0; j <= len; ++j) a += (double)row[j];
          tot = lm_total(att_ctc_total(a, w, ctc[hk]), lw, lm[hk]);
        } else {
          tot = lm_total(ctc[hk], lw, lm[hk]);
        }
      } else {
        for (int j = 0; j <= len; ++j) a += (double)row[j];
        tot = a + w * ctc[hk];
      }
    }
    if (!LM || att) att[hk] = a;
    total[hk] = tot;
  }
  s_tot[lane] = tot;
  __syncthreads();
  int k = 0;
  if (fits) {
    double bv = s_tot[0];
    for (int q = 1; q < nh; ++q)
      if (s_tot[q] > bv) {  // strict: ties stay with the smaller k
        bv = s_tot[q];
        k = q;
      }
  }
  int len = nh > 0 ? hyp_len[(int64_t)b * N + k] : 0;
  len = len < 0 ? 0 : (len > T ? T : len);
  const int* src = hyp + ((int64_t)b * N + k) * T;
  int* dst = out + (int64_t)b * T;
  for (int t = lane; t < T; t += 64) dst[t] = t < len ? src[t] : -1;
  if (lane == 0) {
    out_len[b] = len;
    best_k[b] = k;
    rescored[b] = fits ? 1 : 0;
  }
}

}  // namespace

bool seq_logprob_supported(int64_t d, int64_t V) {
  return d >= 16 && d <= 256 && d % 16 == 0 && V >= 1 && V <= INT32_MAX;
}

size_t seq_logprob_workspace(int64_t R, int64_t d, int64_t V) {
  (void)d;
  const unsigned __int128 n_ct = (unsigned __int128)ceil_div(V, kScBN);
  const unsigned __int128 bytes = (unsigned __int128)R * n_ct * 8 + (unsigned __int128)R * 4;
  return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : (size_t)((bytes + 7) / 8 * 8);
}

void launch_seq_logprob(const float* hidden, int64_t R, int64_t d, const float* weight,
                        const float* bias, int64_t V, const int* target, void* ws, float* lp,
                        hipStream_t s) {
  if (R == 0) return;
  const int n_ct = (int)ceil_div(V, kScBN);
  const int n16 = (int)ceil_div(R, 16);
  const size_t lds = sc_lds_bytes((int)d);
  const int per_cu = (int)std::min<size_t>(kScLdsCU / lds, 2);
  // row groups: fill every CU, at least one subtile per wave and block
  int64_t rgroups = std::max<int64_t>(1, (int64_t)256 * per_cu / n_ct);
  rgroups = std::min<int64_t>(rgroups, ceil_div(n16, kScWaves));
  float2* part = static_cast<float2*>(ws);
  float* tl = reinterpret_cast<float*>(part + R * n_ct);
  hipLaunchKernelGGL(seq_logprob_tile_kernel, dim3((unsigned)(rgroups * n_ct)),
                     dim3(64 * kScWaves), lds, s, hidden, R, (int)d, weight, (int)V, bias, target,
                     n_ct, n16, (int)rgroups, part, tl);
  hipLaunchKernelGGL(seq_logprob_merge_kernel, dim3((unsigned)ceil_div(R, 4)), dim3(256), 0, s,
                     (const float2*)part, (const float*)tl, target, R, (int)V, n_ct, lp);
}

void launch_rescore_prepare(const int* hyp, const int* hyp_len, const int* n_hyp, int64_t B,
                            int64_t N, int64_t T, int64_t Lc, int bos, int eos, int pad,
                            int64_t* tgt_inp, int* target, uint8_t* tgt_pad, uint8_t* ok,
                            hipStream_t s) {
  if (B == 0) return;
  hipLaunchKernelGGL(rescore_prepare_kernel, dim3((unsigned)B), dim3(256), 0, s, hyp, hyp_len,
                     n_hyp, (int)N, (int)T, (int)Lc, bos, eos, pad, tgt_inp, target, tgt_pad, ok);
}

void launch_rescore_select(const float* lp, const int* hyp, const int* hyp_len, const int* n_hyp,
                           const double* ctc, const double* lm, const uint8_t* ok, int64_t B,
                           int64_t N, int64_t T, int64_t Lc, double ctc_weight, double lm_weight,
                           int* out, int* out_len, int* best_k, double* att, double* total,
                           uint8_t* rescored, hipStream_t s) {
  if (B == 0) return;
  // two instantiations: they round att + w * ctc differently (see the kernel)
  const auto kernel = !lm ? rescore_select_kernel<false> : rescore_select_kernel<true>;
  hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, s, lp, hyp, hyp_len, n_hyp, ctc, ok,
                     (int)N, (int)T, (int)Lc, ctc_weight, out, out_len, best_k, att, total,
                     rescored, lm, lm_weight);
}

}  // namespace ob
