// ob_ctc.h — device primitives shared by the CTC kernels (ctc.hip, ctcnbest.hip, ctcprefix.hip,
// align.hip).
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

namespace ob {

// A barrier that orders LDS only: __syncthreads()'s workgroup release also covers global
// memory, which on gfx950 waits for every outstanding vector-memory operation -- a recursion's
// prefetched loads and its stores for later launches included -- at each step.
__device__ __forceinline__ void lds_barrier() {
  __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup", "local");
  __builtin_amdgcn_s_barrier();
  __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup", "local");
}

// log(exp(a) + exp(b)) in fp32, -inf for two -inf: the training CTC's (ctc.hip, ctcnbest.hip).
__device__ __forceinline__ float ctc_lse2(float a, float b) {
  const float m = fmaxf(a, b);
  if (m == -INFINITY) return -INFINITY;
  return m + logf(expf(a - m) + expf(b - m));
}

// The max or the sum of v over a block of kThreads (waves of 64): butterfly within the wave, the
// waves' values through red[kThreads / 64] in wave order. The same bits in every thread; red may
// be reused by the next call.
template <int kThreads>
__device__ __forceinline__ float ctc_block_reduce(float v, bool is_max, float* red) {
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float w = __shfl_xor(v, o);
    v = is_max ? fmaxf(v, w) : v + w;
  }
  __syncthreads();  // red reused across calls
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  float r = red[0];
#pragma unroll
  for (int w = 1; w < kThreads / 64; ++w) r = is_max ? fmaxf(r, red[w]) : r + red[w];
  return r;
}

// The float64 log-sum-exp of one frame's fp32 logits x[0..V) by one whole wave (row max, fp64
// sum of exp(z - max) in lane order, butterfly): the same bits in every lane. Every fp64 CTC
// score of the project uses x[v] - this value.
__device__ __forceinline__ double ctc_frame_lse_wave(const float* __restrict__ x, int V, int lane) {
  float mx = -INFINITY;
  for (int v = lane; v < V; v += 64) {
    const float e = x[v];
    if (e > mx) mx = e;
  }
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) {
    const float om = __shfl_xor(mx, o);
    if (om > mx) mx = om;
  }
  double sum = 0.0;
  for (int v = lane; v < V; v += 64) sum += exp((double)x[v] - (double)mx);
#pragma unroll
  for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o);  // same bits in every lane
  return (double)mx + log(sum);
}

}  // namespace ob
