// relattn_long.hip — the relative-position attention core of MHSA for long utterances:
// a forward-only inference kernel with no T x T state and no T-sized LDS image, 1 <= T <= 4096.
//
// The same computation as relattn.hip's forward (its header comment has the reference ops, the
// layouts and rel_shift as a flat re-reading) with no dropout and nothing saved: it writes ctx
// only. Instead of a query tile's whole score row it walks the keys in chunks of kLongKC with
// an online softmax (running row max and sum in fp32, the ctx accumulators rescaled when the
// max moves), so registers and LDS do not grow with T.
//
// rel_shift per element (X = (q + vb) p^T, T the padded length of the tensor):
//   j <= i   : bd[i][j] = X[i][T-1-i+j]
//   j == i+1 : 0
//   j >= i+2 : bd[i][j] = X[i+1][j-i-2]
// The upper part of row i reads the NEXT query's product. A lane keeps q[i+1] + vb beside
// q[i] + vb, so both parts of row i are products of the lane's own column of an MFMA and the
// tile below a block needs no special row.
//
// Block = (64 queries, head, batch row), 16 queries per wave. Per chunk of kLongKC keys from j0,
// wave rows i = iw0 .. iw0+15:
//   lower band: positions T-1-(iw0+15)+j0 + (0 .. kLongKC+14), product with q[i] + vb; the
//               element of (query i, position m) is bd[i][j] at j = m - (T-1-i);
//   upper band: positions j0-(iw0+15)-2 + (0 .. kLongKC+14), product with q[i+1] + vb; the
//               element of (query i, position m) is bd[i][j] at j = m + i + 2.
// In both bands lane (r, g), tile s, element e lands at chunk column 16s + 4g + e + r - 15, so
// the skew is undone by the store into a [64][kLongKC] LDS image that the scores phase reads back
// as one dwordx4 per key tile. kLongKC/16 + 1 position tiles per band: the redundant work is
// (kLongKC + 16) / kLongKC. A wave whose chunk lies wholly below its diagonal skips the upper
// band, wholly above it the lower band (wave-uniform; no barrier inside).
// ctx: the lane's probabilities P[query r][key 16t + 4g + e] are the B operand of the 16x16x4
// MFMA as they stand (k index g = key 16t + 4g + e, for each e), the A operand v[key][col] comes
// from the chunk's v rows in LDS.
// All products on v_mfma_f32_16x16x4_f32 (exact fp32 fma chains). No atomics; every sum has a
// fixed order, so two runs give the same bits.
#include <math.h>

#include "ob_launch.h"
#include "ob_mma.h"

namespace ob {

namespace {

constexpr int kThreads = 256;
constexpr int kTile = 64;               // query rows per block (16 per wave)
constexpr int kLongKC = 128;            // keys per chunk
constexpr int kLongMaxT = 4096;
constexpr int kNT = kLongKC / 16;       // key tiles per chunk
constexpr int kZP = kLongKC + 4;        // bd image pitch (floats; rows stay 16-B aligned)
static_assert(kLongKC % 16 == 0 && kZP % 4 == 0, "chunk of whole key tiles, aligned image rows");

// v image pitch: D + 4 rounded so that 4 * pitch = 16 (mod 32): the four key rows a wave's
// ds_read_b32 touches fall on disjoint banks
constexpr int v_pitch(int D) { return D % 16 == 4 ? D : D + 4; }

size_t long_lds_bytes(int D) {
  return sizeof(float) * ((size_t)kTile * kZP + (size_t)kLongKC * v_pitch(D) + 16);
}

typedef f32x4 f32x4u __attribute__((aligned(4)));

template <int N>
__device__ __forceinline__ void load_run(const float* __restrict__ p, float (&out)[N]) {
#pragma unroll
  for (int i = 0; i + 4 <= N; i += 4) {
    const f32x4 v = *(const f32x4u*)(p + i);
    out[i] = v[0];
    out[i + 1] = v[1];
    out[i + 2] = v[2];
    out[i + 3] = v[3];
  }
#pragma unroll
  for (int i = N & ~3; i < N; ++i) out[i] = p[i];
}

// x op x[lane ^ 16], then ^ 32: over the four lanes that hold one query's values
__device__ __forceinline__ float xmax_g(float v) {
  v = fmaxf(v, __shfl_xor(v, 16));
  return fmaxf(v, __shfl_xor(v, 32));
}
__device__ __forceinline__ float xsum_g(float v) {
  v += __shfl_xor(v, 16);
  return v + __shfl_xor(v, 32);
}

// One band of the chunk: X of (the lane's query operand qx, positions p0 + 0 .. kLongKC+14)
// into the wave's rows of the bd image. Lane (r, g), tile s, element e is chunk column
// 16s + 4g + e + r - 15, key j = j0 + that. LOWER keeps j <= i + 1 (0 at j == i + 1), the upper
// band j >= i + 2: together they write every element of the row once.
template <int DQ, bool LOWER>
__device__ __forceinline__ void band(const float* __restrict__ pb, int C, int T, int p0, int j0,
                                     int qi, int r, int g, const float (&qx)[DQ],
                                     float* __restrict__ zrow) {
  constexpr int NG = 3;  // position tiles per group
  static_assert((kNT + 1) % NG == 0, "whole groups");
#pragma unroll
  for (int s0 = 0; s0 < kNT + 1; s0 += NG) {
    float pa[NG][DQ];
#pragma unroll
    for (int uu = 0; uu < NG; ++uu) {
      const int row = min(max(p0 + 16 * (s0 + uu) + r, 0), T - 1);  // (clamped: never kept)
      load_run<DQ>(pb + row * C + g * DQ, pa[uu]);
    }
    f32x4 acc[NG];
#pragma unroll
    for (int uu = 0; uu < NG; ++uu) acc[uu] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
    for (int s = 0; s < DQ; ++s)
#pragma unroll
      for (int uu = 0; uu < NG; ++uu) acc[uu] = mfma4(pa[uu][s], qx[s], acc[uu]);
#pragma unroll
    for (int uu = 0; uu < NG; ++uu)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const int jc = 16 * (s0 + uu) + 4 * g + e + r - 15;
        const int j = j0 + jc;
        if (jc < 0 || jc >= kLongKC) continue;
        if (LOWER) {
          if (j <= qi + 1) zrow[jc] = j <= qi ? acc[uu][e] : 0.0f;
        } else {
          if (j >= qi + 2) zrow[jc] = acc[uu][e];
        }
      }
  }
}

template <int DQ>
__global__ __launch_bounds__(kThreads) void relattn_long_kernel(
    const float* __restrict__ q, const float* __restrict__ k, const float* __restrict__ v,
    const float* __restrict__ pos, const float* __restrict__ u, const float* __restrict__ vbias,
    const int* __restrict__ lens, int Bp, int T, int H, float inv_sqrt_d,
    float* __restrict__ ctx) {
  constexpr int D = 4 * DQ;
  constexpr int CT = (D + 15) / 16;
  constexpr int DP = v_pitch(D);
  extern __shared__ __attribute__((aligned(16))) float smem[];
  float* zimg = smem;                 // [kTile][kZP]: bd of (tile query, chunk key)
  float* vimg = smem + kTile * kZP;   // [kLongKC][DP]: the chunk's v rows (+ 16 floats of slack)
  const int i0 = (int)blockIdx.x * kTile, h = (int)blockIdx.y, b = (int)blockIdx.z;
  const int C = H * D;
  const int L = min(max(lens[b], 0), T);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, r = lane & 15, g = lane >> 4;
  const size_t bo = (size_t)b * T * C + h * D;
  float* cb = ctx + bo;

  // a query tile wholly past the valid frames: zeros, and out before any barrier
  if (i0 >= L) {
    for (int e = threadIdx.x; e < kTile * DQ; e += kThreads) {
      const int row = e / DQ, cq = e - row * DQ;
      if (i0 + row < T) *(f32x4u*)(cb + (i0 + row) * C + 4 * cq) = f32x4{0.f, 0.f, 0.f, 0.f};
    }
    return;
  }

  const float* qb = q + bo;
  const float* kb = k + bo;
  const float* vbp = v + bo;
  const float* pb = pos + (size_t)(b / Bp) * T * C + h * D;
  const float* ub = u + h * D;
  const float* vbb = vbias + h * D;

  const int iw0 = i0 + 16 * __builtin_amdgcn_readfirstlane(w);  // the wave's first query
  const int qi = iw0 + r;                                       // this lane's query
  float qu[DQ], qv[DQ], qw[DQ];  // q[i] + u, q[i] + vb, q[i+1] + vb: B operands, columns g*DQ ..
  {
    float x[DQ], xn[DQ];
    load_run<DQ>(qb + min(qi, T - 1) * C + g * DQ, x);
    load_run<DQ>(qb + min(qi + 1, T - 1) * C + g * DQ, xn);  // (i = T-1 has no upper part)
#pragma unroll
    for (int s = 0; s < DQ; ++s) {
      const int c = g * DQ + s;
      qu[s] = x[s] + ub[c];
      qv[s] = x[s] + vbb[c];
      qw[s] = xn[s] + vbb[c];
    }
  }
  const int Lq = qi < L ? L : 0;  // valid keys of this row
  float* zrow = zimg + (16 * w + r) * kZP;

  float mrun = -INFINITY, srun = 0.0f;
  f32x4 o[CT];
#pragma unroll
  for (int ct = 0; ct < CT; ++ct) o[ct] = f32x4{0.f, 0.f, 0.f, 0.f};

  const int nch = (L + kLongKC - 1) / kLongKC;  // chunks wholly past L are skipped (block-uniform)
  for (int ch = 0; ch < nch; ++ch) {
    const int j0 = ch * kLongKC;
    __syncthreads();  // the previous chunk's images are read
    // v rows of the chunk (rows >= L: zeros, their probabilities are 0)
    for (int e = threadIdx.x; e < kLongKC * DQ; e += kThreads) {
      const int row = e / DQ, cq = e - row * DQ;
      const int key = j0 + row;
      f32x4 x = f32x4{0.f, 0.f, 0.f, 0.f};
      if (key < L) x = *(const f32x4u*)(vbp + key * C + 4 * cq);
      *reinterpret_cast<f32x4*>(vimg + row * DP + 4 * cq) = x;
    }
    // bd of the wave's rows (wave-uniform tests)
    if (j0 <= iw0 + 16)  // some j <= i + 1
      band<DQ, true>(pb, C, T, T - 1 - (iw0 + 15) + j0, j0, qi, r, g, qv, zrow);
    if (j0 + kLongKC - 1 >= iw0 + 2)  // some j >= i + 2
      band<DQ, false>(pb, C, T, j0 - (iw0 + 15) - 2, j0, qi, r, g, qw, zrow);
    __syncthreads();

    // scores of (query qi, keys j0 + 16t + 4g + e): ac by MFMA (A = k rows, B = q + u)
    f32x4 sc[kNT];
    float cmax = -INFINITY;
#pragma unroll
    for (int t0 = 0; t0 < kNT; t0 += 4) {
      float ka[4][DQ];
#pragma unroll
      for (int uu = 0; uu < 4; ++uu)
        load_run<DQ>(kb + min(j0 + 16 * (t0 + uu) + r, T - 1) * C + g * DQ, ka[uu]);
#pragma unroll
      for (int uu = 0; uu < 4; ++uu) sc[t0 + uu] = f32x4{0.f, 0.f, 0.f, 0.f};
#pragma unroll
      for (int s = 0; s < DQ; ++s)
#pragma unroll
        for (int uu = 0; uu < 4; ++uu) sc[t0 + uu] = mfma4(ka[uu][s], qu[s], sc[t0 + uu]);
#pragma unroll
      for (int uu = 0; uu < 4; ++uu) {
        const int t = t0 + uu;
        const f32x4 z = *reinterpret_cast<const f32x4*>(zrow + 16 * t + 4 * g);
#pragma unroll
        for (int e = 0; e < 4; ++e) {
          const float s = (sc[t][e] + z[e]) * inv_sqrt_d;
          sc[t][e] = j0 + 16 * t + 4 * g + e < Lq ? s : -INFINITY;
          cmax = fmaxf(cmax, sc[t][e]);
        }
      }
    }
    // online softmax. A row with no valid key so far keeps its max at -inf: the exponentials
    // are taken against 0 there (exp(-inf - 0) = 0), never against -inf.
    cmax = xmax_g(cmax);
    const float mnew = fmaxf(mrun, cmax);
    const float msafe = mnew == -INFINITY ? 0.0f : mnew;
    const float alpha = __expf(mrun - msafe);
    float psum = 0.0f;
#pragma unroll
    for (int t = 0; t < kNT; ++t)
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float p = __expf(sc[t][e] - msafe);
        sc[t][e] = p;
        psum += p;
      }
    psum = xsum_g(psum);
    srun = srun * alpha + psum;
    mrun = mnew;
#pragma unroll
    for (int ct = 0; ct < CT; ++ct)
#pragma unroll
      for (int e = 0; e < 4; ++e) o[ct][e] *= alpha;

    // ctx^T += v^T P^T: D[col 16ct + 4g + e'][query r], k index g = key 16t + 4g + e.
    // (columns >= D of the last column tile read the next image row: their results are dropped)
#pragma unroll
    for (int t = 0; t < kNT; ++t) {
      if (j0 + 16 * t >= L) continue;  // block-uniform: the tile's probabilities are all 0
#pragma unroll
      for (int e = 0; e < 4; ++e) {
        const float* vr = vimg + (16 * t + 4 * g + e) * DP + r;
#pragma unroll
        for (int ct = 0; ct < CT; ++ct) o[ct] = mfma4(vr[16 * ct], sc[t][e], o[ct]);
      }
    }
  }

  const float rs = srun > 0.0f ? 1.0f / srun : 0.0f;
  if (qi < T) {
#pragma unroll
    for (int ct = 0; ct < CT; ++ct) {
      const int col = 16 * ct + 4 * g;
      if (col >= D) continue;
      f32x4 out = f32x4{0.f, 0.f, 0.f, 0.f};  // rows >= lens[b]: exactly 0
      if (qi < L) out = o[ct] * rs;
      *(f32x4u*)(cb + qi * C + col) = out;
    }
  }
}

}  // namespace

int64_t relattn_long_key_chunk() { return kLongKC; }
int64_t relattn_long_max_t() { return kLongMaxT; }

// every in-slice offset of the kernel is a 32-bit int: the [T][H*d] slice must fit
bool relattn_long_supported(int64_t T, int64_t H, int64_t d) {
  if (T < 1 || T > kLongMaxT || H < 1 || !(d == 16 || d == 32 || d == 36 || d == 64)) return false;
  return T * H * d <= ((int64_t)1 << 29);
}

void launch_relattn_long(const float* q, const float* k, const float* v, const float* pos,
                         const float* u, const float* vb, const int* lens, int64_t Bt, int64_t P,
                         int64_t T, int64_t H, int64_t d, float* ctx, hipStream_t s) {
  const dim3 grid((unsigned)((T + kTile - 1) / kTile), (unsigned)H, (unsigned)Bt);
  const float inv_sqrt_d = 1.0f / (float)sqrt((double)d);  // torch: tensor / scalar = * (1/scalar)
  const size_t lds = long_lds_bytes((int)d);
#define OB_RAL(DQ)                                                                              \
  hipLaunchKernelGGL((relattn_long_kernel<DQ>), grid, dim3(kThreads), lds, s, q, k, v, pos, u, vb, \
                     lens, (int)(Bt / P), (int)T, (int)H, inv_sqrt_d, ctx)
  if (d == 16) OB_RAL(4);
  else if (d == 32) OB_RAL(8);
  else if (d == 36) OB_RAL(9);
  else OB_RAL(16);
#undef OB_RAL
}

}  // namespace ob
