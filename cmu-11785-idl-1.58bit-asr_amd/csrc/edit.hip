// edit.hip — batched Levenshtein distance over padded int32 sequences, and what the eval path
// builds on it: error counts (substitutions / insertions / deletions), the distances of an n-best
// to its reference and among its entries, and the minimum-Bayes-risk pick.
//
//   pairs kernel    one wave64 per (reference, hypothesis) pair, the DP of ob_edit.h; a fixed
//                   pool of wave slots walks the pairs, each slot with one row of the workspace
//                   for the band boundary of references longer than 64.
//   n-best kernel   the same pool over the jobs of every utterance, in one launch: entry k against
//                   the reference (with counts), and entry j against entry k for j <= k (distance
//                   only; the wave writes [j][k] and [k][j], a diagonal job writes its 0).
//   mbr kernel      one wave per utterance: posterior from the totals, expected distance of every
//                   entry, the smallest wins; fp64, ascending index order, nothing contracted.
//
// No atomics, every word one writer, integer results: the outputs are a function of the inputs
// alone. No kernel synchronises with the host.
#include <math.h>

#include <algorithm>

#include "ob_edit.h"
#include "ob_launch.h"

namespace ob {

namespace {

using namespace edit;

constexpr int kEdWaves = 4;         // pairs in flight per block
constexpr int kEdMaxBlocks = 1024;  // 4 blocks per CU: the slot pool, and the workspace, stay bounded
constexpr int kMbrMaxN = 32;

__device__ __forceinline__ int clamp_to(int n, int hi) { return n < 0 ? 0 : (n > hi ? hi : n); }

// one pair on the calling wave, its distance returned to every lane; a negative length marks an
// absent pair (-1 everywhere)
template <bool OPS>
__device__ __forceinline__ int edit_pair(const int* a, int la, int La, const int* b, int lb,
                                         int Lb, int lane, uint64_t* row, int* dist, int* ops) {
  using C = Cell<OPS>;
  int d = -1, su = -1, in = -1, de = -1;
  if (la >= 0 && lb >= 0) {
    la = la > La ? La : la;
    lb = lb > Lb ? Lb : lb;
    const typename C::type c =
        edit_wave<OPS>(a, la, b, lb, lane, reinterpret_cast<typename C::type*>(row));
    d = (int)C::dist(c);
    if constexpr (OPS) {
      su = (int)(c >> C::kSubShift) & 0x1fff;
      in = (int)(c >> C::kInsShift) & 0x1fff;
      de = (int)c & 0x1fff;
    }
  }
  if (lane == 0) {
    if (dist) *dist = d;
    if constexpr (OPS) {
      if (ops) {
        ops[0] = su;
        ops[1] = in;
        ops[2] = de;
      }
    }
  }
  return d;
}

template <bool OPS>
__global__ __launch_bounds__(64 * kEdWaves) void edit_pairs_kernel(
    const int* __restrict__ a, const int* __restrict__ a_len, const int* __restrict__ b,
    const int* __restrict__ b_len, int64_t P, int La, int Lb, uint64_t* __restrict__ ws,
    int* __restrict__ dist, int* __restrict__ ops) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t slot = (int64_t)blockIdx.x * kEdWaves + wave;
  const int64_t nslots = (int64_t)gridDim.x * kEdWaves;
  uint64_t* row = ws + slot * Lb;
  for (int64_t p = slot; p < P; p += nslots) {
    const int la = __builtin_amdgcn_readfirstlane(a_len[p]);
    const int lb = __builtin_amdgcn_readfirstlane(b_len[p]);
    edit_pair<OPS>(a + p * La, la, La, b + p * Lb, lb, Lb, lane, row, dist + p,
                   OPS ? ops + p * 3 : nullptr);
  }
}

// jobs per utterance: [0, nref) entry k against the reference; then the pairs j <= k, row-major
__global__ __launch_bounds__(64 * kEdWaves) void nbest_edit_kernel(
    const int* __restrict__ hyp, const int* __restrict__ hyp_len, const int* __restrict__ n_hyp,
    const int* __restrict__ ref, const int* __restrict__ ref_len, int64_t B, int N, int T, int S,
    int nref, int jobs, uint64_t* __restrict__ ws, int* __restrict__ dref,
    int* __restrict__ ops_ref, int* __restrict__ dpair) {
  const int lane = threadIdx.x & 63;
  const int wave = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int64_t slot = (int64_t)blockIdx.x * kEdWaves + wave;
  const int64_t nslots = (int64_t)gridDim.x * kEdWaves;
  uint64_t* row = ws + slot * T;
  const int64_t total = B * jobs;
  for (int64_t q = slot; q < total; q += nslots) {
    const int64_t u = q / jobs;
    int r = (int)(q - u * jobs);
    const int n = clamp_to(__builtin_amdgcn_readfirstlane(n_hyp[u]), N);
    const int* hu = hyp + u * (int64_t)N * T;
    const int* lu = hyp_len + u * (int64_t)N;
    if (r < nref) {
      const bool live = r < n;
      const int la = live ? __builtin_amdgcn_readfirstlane(ref_len[u]) : -1;
      const int lb = live ? clamp_to(__builtin_amdgcn_readfirstlane(lu[r]), T) : -1;
      edit_pair<true>(ref + u * (int64_t)S, la, S, hu + (int64_t)r * T, lb, T, lane, row,
                      dref ? dref + u * N + r : nullptr,
                      ops_ref ? ops_ref + (u * N + r) * 3 : nullptr);
      continue;
    }
    r -= nref;
    int j = 0;
    while (r >= N - j) {
      r -= N - j;
      ++j;
    }
    const int k = j + r;
    int* dp = dpair + u * (int64_t)N * N;
    if (k >= n) {  // an absent entry's row and column
      if (lane == 0) dp[j * N + k] = dp[k * N + j] = -1;
    } else if (j == k) {
      if (lane == 0) dp[j * N + j] = 0;
    } else {
      const int la = clamp_to(__builtin_amdgcn_readfirstlane(lu[j]), T);
      const int lb = clamp_to(__builtin_amdgcn_readfirstlane(lu[k]), T);
      const int d = edit_pair<false>(hu + (int64_t)j * T, la, T, hu + (int64_t)k * T, lb, T, lane,
                                     row, dp + j * N + k, nullptr);
      if (lane == 0) dp[k * N + j] = d;
    }
  }
}

// block = utterance (one wave): lane k holds entry k
__global__ __launch_bounds__(64) void mbr_select_kernel(
    const int* __restrict__ dpair, const int* __restrict__ hyp, const int* __restrict__ hyp_len,
    const int* __restrict__ n_hyp, const double* __restrict__ score, double scale, int N, int T,
    int* __restrict__ out, int* __restrict__ out_len, int* __restrict__ best_k,
    double* __restrict__ risk, double* __restrict__ post) {
#pragma clang fp contract(off)
  __shared__ double s_v[64];
  const int64_t b = blockIdx.x;
  const int lane = threadIdx.x;
  const int n = clamp_to(n_hyp[b], N);
  const double kInf = (double)INFINITY;
  const double* sc = score + b * N;
  double m = -kInf;
  for (int q = 0; q < n; ++q)
    if (sc[q] > m) m = sc[q];
  const bool any = m > -kInf;  // false: no live entry, or none with a finite total (or a NaN one)
  const bool mine = any && lane < n;
  // an entry at -inf has weight 0 at every scale (0 * -inf is not formed)
  const double w = mine && sc[lane] > -kInf ? exp(scale * (sc[lane] - m)) : 0.0;
  s_v[lane] = w;
  __syncthreads();
  double z = 0.0;
  for (int q = 0; q < n; ++q) z += s_v[q];
  const double p = mine ? w / z : 0.0;
  __syncthreads();
  s_v[lane] = p;
  __syncthreads();
  double r = kInf;
  if (mine) {
    const int* dk = dpair + (b * N + lane) * (int64_t)N;
    r = 0.0;
    for (int q = 0; q < n; ++q) {
      const double t = s_v[q] * (double)dk[q];
      r += t;
    }
  }
  if (lane < N) {
    risk[b * N + lane] = r;
    post[b * N + lane] = p;
  }
  __syncthreads();
  s_v[lane] = r;
  __syncthreads();
  int k = 0;
  double bv = s_v[0];
  for (int q = 1; q < n; ++q)
    if (s_v[q] < bv) {  // strict: ties stay with the smaller k
      bv = s_v[q];
      k = q;
    }
  const int len = n > 0 ? clamp_to(hyp_len[b * N + k], T) : 0;
  const int* src = hyp + (b * N + k) * (int64_t)T;
  int* dst = out + b * (int64_t)T;
  for (int t = lane; t < T; t += 64) dst[t] = t < len ? src[t] : -1;
  if (lane == 0) {
    out_len[b] = len;
    best_k[b] = k;
  }
}

// wave slots for `jobs` waves of work, and the blocks that hold them
int64_t edit_blocks(int64_t jobs) {
  return std::max<int64_t>(1, std::min<int64_t>(ceil_div(jobs, kEdWaves), kEdMaxBlocks));
}

int64_t nbest_jobs(int64_t N, bool with_ref, bool with_pair) {
  return (with_ref ? N : 0) + (with_pair ? N * (N + 1) / 2 : 0);
}

}  // namespace

bool edit_supported(int64_t La, int64_t Lb) {
  return La >= 0 && La <= kMaxLen && Lb >= 0 && Lb <= kMaxLen;
}

bool nbest_edit_supported(int64_t B, int64_t N, int64_t T, int64_t S) {
  return B >= 0 && N >= 1 && N <= kMbrMaxN && edit_supported(S, T) &&
         B <= INT32_MAX / (N * (N + 3) / 2);
}

// one row of Lb (at least one) 8-byte cells per wave slot
size_t edit_distance_workspace(int64_t P, int64_t La, int64_t Lb) {
  if (!edit_supported(La, Lb) || P < 0 || P > INT32_MAX) return 0;
  return (size_t)(edit_blocks(P) * kEdWaves) * (size_t)std::max<int64_t>(Lb, 1) * 8;
}

// sized for the call with both outputs, whichever are asked for
size_t nbest_edit_distance_workspace(int64_t B, int64_t N, int64_t T, int64_t S) {
  if (!nbest_edit_supported(B, N, T, S)) return 0;
  return edit_distance_workspace(B * nbest_jobs(N, true, true), S, T);
}

void launch_edit_distance(const int* a, const int* a_len, const int* b, const int* b_len,
                          int64_t P, int64_t La, int64_t Lb, void* ws, int* dist, int* ops,
                          hipStream_t s) {
  if (P == 0) return;
  const dim3 grid((unsigned)edit_blocks(P)), block(64 * kEdWaves);
  uint64_t* w = static_cast<uint64_t*>(ws);
  if (ops)
    hipLaunchKernelGGL(edit_pairs_kernel<true>, grid, block, 0, s, a, a_len, b, b_len, P, (int)La,
                       (int)Lb, w, dist, ops);
  else
    hipLaunchKernelGGL(edit_pairs_kernel<false>, grid, block, 0, s, a, a_len, b, b_len, P,
                       (int)La, (int)Lb, w, dist, ops);
}

void launch_nbest_edit_distance(const int* hyp, const int* hyp_len, const int* n_hyp,
                                const int* ref, const int* ref_len, int64_t B, int64_t N,
                                int64_t T, int64_t S, void* ws, int* dref, int* ops_ref,
                                int* dpair, hipStream_t s) {
  if (B == 0) return;
  const bool with_ref = dref || ops_ref;
  const int64_t jobs = nbest_jobs(N, with_ref, dpair != nullptr);
  hipLaunchKernelGGL(nbest_edit_kernel, dim3((unsigned)edit_blocks(B * jobs)),
                     dim3(64 * kEdWaves), 0, s, hyp, hyp_len, n_hyp, ref, ref_len, B, (int)N,
                     (int)T, (int)S, with_ref ? (int)N : 0, (int)jobs, static_cast<uint64_t*>(ws),
                     dref, ops_ref, dpair);
}

void launch_mbr_select(const int* dpair, const int* hyp, const int* hyp_len, const int* n_hyp,
                       const double* score, double scale, int64_t B, int64_t N, int64_t T,
                       int* out, int* out_len, int* best_k, double* risk, double* post,
                       hipStream_t s) {
  if (B == 0) return;
  hipLaunchKernelGGL(mbr_select_kernel, dim3((unsigned)B), dim3(64), 0, s, dpair, hyp, hyp_len,
                     n_hyp, score, scale, (int)N, (int)T, out, out_len, best_k, risk, post);
}

}  // namespace ob
