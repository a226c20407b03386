// ob_scorer.h — the exact-fp32 output-layer GEMM tile shared by the sequence scorer
// (rescore.hip, ob_seq_logprob) and the top-k output layer (attdec.hip, ob_seq_topk).
//
// Both operands are split into three bf16 planes (x = hi + mid + lo), six
// v_mfma_f32_16x16x32_bf16 per k-step (mm, lh, hl, mh, hm, hh; the dropped terms are below
// 2^-25 |x||w|): the split and the product order of ob_mma.h. A block holds the three-plane
// image of one 64-column tile of W in LDS ([64][3][kpad+8] bf16, the pad keeps the B-fragment
// ds_read_b128 conflict-free) and walks 16-row subtiles of the hidden rows, one subtile per
// wave at a time.
//
// Fragment map of v_mfma_f32_16x16x32_bf16 (lane l, r = l&15, g = l>>4):
//   A[i=r][kk=8g+j] (j<8), B[kk=8g+j][col=r], D[row=4g+reg][col=r].
#pragma once
#include "ob_mma.h"

namespace ob {
namespace scorer {

constexpr int kScWaves = 4;
constexpr int kScNT = 4;             // 16-column fragments per tile
constexpr int kScBN = 16 * kScNT;    // columns per tile
constexpr size_t kScLdsCU = 160 * 1024;

__host__ __device__ inline int sc_kpad(int K) { return (K + 31) & ~31; }
__host__ __device__ inline size_t sc_lds_bytes(int K) {
  return (size_t)kScBN * 3 * (sc_kpad(K) + 8) * sizeof(uint16_t);
}

// B image of the tile starting at vocabulary row n0: column c (row n0 + c of W) along k in 3
// planes; loader unit = one dwordx4 of a W row (clamped address; zeros selected for k >= K and
// for columns >= V). The caller synchronises the block afterwards.
__device__ __forceinline__ void sc_build_image(__bf16* __restrict__ bimg,
                                               const float* __restrict__ W, int K, int V, int n0) {
  constexpr int kThr = 64 * kScWaves;
  const int kpad = sc_kpad(K);
  const int stride = kpad + 8;    // bf16 per plane row
  const int cpitch = 3 * stride;  // bf16 per image column (three planes)
  const int kq = kpad >> 2;
  const int units = kScBN * kq;
  for (int u = threadIdx.x; u < units; u += kThr) {
    const int c = u / kq, k4 = u - c * kq;
    const int n = n0 + c < V ? n0 + c : V - 1;
    const int kk = 4 * k4 < K - 4 ? 4 * k4 : K - 4;
    const f32x4 v = *reinterpret_cast<const f32x4*>(W + (int64_t)n * K + kk);
    const bool ok = 4 * k4 < K && n0 + c < V;
    const f32x4 x = ok ? v : f32x4{0.f, 0.f, 0.f, 0.f};
    bf16x4 h, m, l;
    split3x4(x, h, m, l);
    __bf16* col = bimg + c * cpitch + 4 * k4;
    *reinterpret_cast<bf16x4*>(col) = h;
    *reinterpret_cast<bf16x4*>(col + stride) = m;
    *reinterpret_cast<bf16x4*>(col + 2 * stride) = l;
  }
}

// acc[t] = the 16 x 16 fragment t of (16 hidden rows) x (the tile's 64 columns): arow = this
// lane's hidden row (lane r), brow = bimg + r * cpitch + 8 g.
__device__ __forceinline__ void sc_subtile_mma(const float* __restrict__ arow,
                                               const __bf16* __restrict__ brow, int K, int kg,
                                               f32x4 (&acc)[kScNT]) {
  const int kpad = sc_kpad(K);
  const int stride = kpad + 8;
  const int cpitch = 3 * stride;
#pragma unroll
  for (int t = 0; t < kScNT; ++t) acc[t] = f32x4{0.f, 0.f, 0.f, 0.f};
  f32x4 c0, c1, p0, p1;
  load8(arow, kg, K, c0, c1);
  for (int kc = 0; kc < kpad; kc += 32) {
    load8(arow, kc + 32 + kg, K, p0, p1);  // the next chunk (clamped past the end)
    bf16x8 a[3];
    split3x8(c0, c1, a[0], a[1], a[2]);
#pragma unroll
    for (int t0 = 0; t0 < kScNT; t0 += 2) {
      bf16x8 b[2][3];
#pragma unroll
      for (int t = 0; t < 2; ++t)
#pragma unroll
        for (int q = 0; q < 3; ++q)
          b[t][q] = *reinterpret_cast<const bf16x8*>(brow + (t0 + t) * 16 * cpitch +
                                                      q * stride + kc);
#pragma unroll
      for (int p = 0; p < 6; ++p)
#pragma unroll
        for (int t = 0; t < 2; ++t)
          acc[t0 + t] = mfma_bf16(a[kProdA[p]], b[t][kProdB[p]], acc[t0 + t]);
    }
    c0 = p0;
    c1 = p1;
  }
}

}  // namespace scorer
}  // namespace ob
