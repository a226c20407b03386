// ob_ctc.h — device primitives shared by the CTC kernels (ctc.hip, ctcprefix.hip, align.hip).
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
