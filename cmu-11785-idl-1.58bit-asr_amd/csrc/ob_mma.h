// ob_mma.h — the exact-fp32 bf16 MFMA device primitives every GEMM-class kernel shares: the
// vector types, the MFMA wrappers, the three-plane split, the product order, and the block /
// buffer helpers that go with them. This is the single definition of the convention; a
// kernel that writes pre-split planes for another to read agrees with it by construction.
//
// Exact fp32 on the bf16 matrix cores: x = hi + mid + lo, each plane the bf16 (RNE) rounding
// of what the planes before it left, the residuals exact in fp32 (8 + 8 + 8 significand
// bits). Of the nine plane products of x.w the six with plane index sum <= 2 are kept; the
// dropped ones (ml, lm, ll) are below 2^-25 |x||w|. The kept products are accumulated
// smallest first -- mm lh hl mh hm hh -- so the small terms are not absorbed by a large
// partial sum. Ternary codes are exact in bf16: those GEMMs need the three products of the
// activation planes only.
//
// The split has two source forms that compute the same values but may compile differently:
// the scalar cast (split3 and its x4 / x8 shapes: `(__bf16)x` per element) and the packed
// pair (cvt2 / split2: v_cvt_pk_bf16_f32 on two values). A kernel keeps the form it uses.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ob {

typedef float f32x2 __attribute__((ext_vector_type(2)));
typedef float f32x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x2 __attribute__((ext_vector_type(2)));
typedef __bf16 bf16x4 __attribute__((ext_vector_type(4)));
typedef __bf16 bf16x8 __attribute__((ext_vector_type(8)));
typedef uint32_t u32x4 __attribute__((ext_vector_type(4)));

// v_mfma_f32_16x16x32_bf16, fragment map (lane l, r = l&15, g = l>>4):
//   A[i=r][kk=8g+j] (j<8), B[kk=8g+j][col=r], D[row=4g+reg][col=r].
__device__ __forceinline__ f32x4 mfma_bf16(const bf16x8& a, const bf16x8& b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x32_bf16(a, b, c, 0, 0, 0);
}

// v_mfma_f32_16x16x4_f32 (an exact fp32 fma chain): A[i=r][kk=g], B[kk=g][j=r].
__device__ __forceinline__ f32x4 mfma4(float a, float b, f32x4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// ---- scalar-cast split: x = h + m + l exactly
__device__ __forceinline__ void split3(float x, __bf16& h, __bf16& m, __bf16& l) {
  h = (__bf16)x;
  const float r1 = x - (float)h;
  m = (__bf16)r1;
  l = (__bf16)(r1 - (float)m);
}

// 4 floats into one bf16x4 per plane. split3's steps written out: through the call the
// B-image builders (dgemm.hip, ob_scorer.h) compile to different code.
__device__ __forceinline__ void split3x4(const f32x4& a, bf16x4& hi, bf16x4& mid, bf16x4& lo) {
#pragma unroll
  for (int j = 0; j < 4; ++j) {
    const __bf16 h = (__bf16)a[j];
    const float r1 = a[j] - (float)h;
    const __bf16 m = (__bf16)r1;
    hi[j] = h;
    mid[j] = m;
    lo[j] = (__bf16)(r1 - (float)m);
  }
}

// 8 floats (a then b) into one bf16x8 fragment per plane
__device__ __forceinline__ void split3x8(const f32x4& a, const f32x4& b, bf16x8& hi, bf16x8& mid,
                                         bf16x8& lo) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 h, m, l;
    split3(j < 4 ? a[j] : b[j - 4], h, m, l);
    hi[j] = h;
    mid[j] = m;
    lo[j] = l;
  }
}

// the same from 8 floats in an array, the planes as p[0 .. 2] (mfma_x6's operand)
__device__ __forceinline__ void split3x8(const float (&x)[8], bf16x8 (&p)[3]) {
#pragma unroll
  for (int j = 0; j < 8; ++j) {
    __bf16 h, m, l;
    split3(x[j], h, m, l);
    p[0][j] = h;
    p[1][j] = m;
    p[2][j] = l;
  }
}

// ---- packed split
// Round two fp32 to bf16 (v_cvt_pk_bf16_f32), packed (a low, b high); also returns the two
// rounded values as fp32.
__device__ __forceinline__ uint32_t cvt2(float a, float b, float& ra, float& rb) {
  const bf16x2 v = __builtin_convertvector(f32x2{a, b}, bf16x2);
  const uint32_t u = __builtin_bit_cast(uint32_t, v);
  ra = __uint_as_float(u << 16);
  rb = __uint_as_float(u & 0xFFFF0000u);
  return u;
}

// hi / mid / lo of two values as three packed dwords (x0 in the low half)
__device__ __forceinline__ void split2(float x0, float x1, uint32_t& ph, uint32_t& pm,
                                       uint32_t& pl) {
  float h0, h1, m0, m1, l0, l1;
  ph = cvt2(x0, x1, h0, h1);
  const float r0 = x0 - h0, r1 = x1 - h1;
  pm = cvt2(r0, r1, m0, m1);
  pl = cvt2(r0 - m0, r1 - m1, l0, l1);
}

// ---- product order: plane of A and of B (0 = hi, 1 = mid, 2 = lo) per product, in the order
// the products are accumulated: mm lh hl mh hm hh
constexpr int kProdA[6] = {1, 2, 0, 1, 0, 0};
constexpr int kProdB[6] = {1, 0, 2, 0, 1, 0};

constexpr bool prod_order_ok() {
  for (int p = 0; p < 6; ++p) {
    if (kProdA[p] + kProdB[p] > 2) return false;  // one of the dropped terms
    if (p > 0 && kProdA[p] + kProdB[p] > kProdA[p - 1] + kProdB[p - 1]) return false;
  }
  return true;
}
static_assert(prod_order_ok(), "bf16x6 products: plane index sum <= 2, summed smallest first");

__device__ __forceinline__ f32x4 mfma_x6(const bf16x8 (&a)[3], const bf16x8 (&b)[3], f32x4 c) {
#pragma unroll
  for (int p = 0; p < 6; ++p) c = mfma_bf16(a[kProdA[p]], b[kProdB[p]], c);
  return c;
}

// ---- block and buffer helpers
// Bijective XCD-aware remap (hardware block b runs on XCD b % 8): consecutive logical ids
// land on one XCD under round-robin dispatch, so blocks that share operands share one L2.
__device__ __forceinline__ int xcd_logical(int b, int nb) {
  const int q = nb / 8, r = nb % 8, x = b % 8;
  return (x < r ? x * (q + 1) : r * (q + 1) + (x - r) * q) + b / 8;
}

// Buffer descriptor over [base, base + bytes): loads past the end return 0 (hardware range
// check) and every offset is a 32-bit sum, so rows past the end need no per-lane test.
__device__ __forceinline__ __amdgpu_buffer_rsrc_t make_rsrc(const float* base, int64_t bytes) {
  const uint32_t nrec = bytes > 0xFFFFFFF0ll ? 0xFFFFFFF0u : (uint32_t)bytes;
  return __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(base), (short)0, (int)nrec,
                                           0x00020000);
}

// Two dwordx4 of one row at k and k+4. The address is clamped into the row instead of
// guarding the load (a guarded `cond ? *p : 0` makes hipcc branch around the load and wait
// vmcnt(0) at it, and an unguarded load keeps a prefetch window in flight). Clamped
// positions k >= K read the row's own last floats and must meet zero rows of the B image.
__device__ __forceinline__ void load8(const float* __restrict__ arow, int k, int K, f32x4& a,
                                      f32x4& b) {
  const int ka = k < K - 4 ? k : K - 4;
  const int kb = k + 4 < K - 4 ? k + 4 : K - 4;
  a = *reinterpret_cast<const f32x4*>(arow + ka);
  b = *reinterpret_cast<const f32x4*>(arow + kb);
}

}  // namespace ob
