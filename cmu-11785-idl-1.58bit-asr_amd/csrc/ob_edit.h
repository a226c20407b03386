// ob_edit.h — the Levenshtein DP of one (reference, hypothesis) pair on one wave64 (edit.hip).
//
// Definition (include/onebit_hip.h, tests/edit_ref.py): a cell is (d, sub, ins, del);
// D[0][j] = (j, 0, j, 0), D[i][0] = (i, 0, 0, i); a[i-1] == b[j-1] copies D[i-1][j-1]; otherwise the
// smallest d among diagonal (substitution), up (deletion), left (insertion) wins, ties in that
// order, and d and the winner's count grow by 1. The counts travel with the cell: no backtrace.
//
// Work mapping: lane l owns reference row i = 64 * band + l + 1; at step s it forms column
// j = s - l + 1, so a step is one anti-diagonal. The hypothesis token and the cell of the row below
// move up one lane per step (a wave-wide DPP shift, no LDS); the diagonal neighbour is the value
// the lane received a step earlier; the left neighbour is the lane's own previous cell. Lane 0
// takes its tokens and, from the second band on, the cells of the previous band's last row from
// 64-element chunks held in registers (loaded coalesced one chunk ahead, read with v_readlane at
// the wave-uniform step index), so no load sits on the dependent chain. Lane 63's cell of step k
// of a chunk is parked in lane k and the chunk is stored at once, coalesced, into `row` for the
// next band. The store of a chunk covers columns that were loaded two chunks earlier, so one row
// serves in place.
//
// OPS = true: the four fields in one uint64, 13 bits each (lengths <= 4096 < 2^13), d on top so
// that the d comparison is a shift. OPS = false: the cell is d alone in a uint32.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

namespace ob {
namespace edit {

constexpr int kMaxLen = 4096;  // 13-bit fields

// lane l takes v of lane l - 1, lane 0 takes `first` (v_mov_b32_dpp wave_shr:1; a lane without a
// source keeps the old value, which is `first`)
__device__ __forceinline__ int shift_up(int first, int v) {
  return __builtin_amdgcn_update_dpp(first, v, 0x138, 0xf, 0xf, false);
}

template <bool OPS>
struct Cell;

template <>
struct Cell<true> {
  using type = uint64_t;
  static constexpr int kD = 39, kSubShift = 26, kInsShift = 13;
  static constexpr type kSub = (type(1) << kD) | (type(1) << kSubShift);
  static constexpr type kIns = (type(1) << kD) | (type(1) << kInsShift);
  static constexpr type kDel = (type(1) << kD) | type(1);
  __device__ static type col0(int j) { return type(j) * kIns; }  // D[0][j]
  __device__ static type row0(int i) { return type(i) * kDel; }  // D[i][0]
  __device__ static uint32_t dist(type c) { return (uint32_t)(c >> kD); }
  __device__ static type readlane(type v, int l) {
    const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
    const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
    return ((type)hi << 32) | lo;
  }
  __device__ static type shift_up(type first, type v) {
    const uint32_t lo = edit::shift_up((int)(uint32_t)first, (int)(uint32_t)v);
    const uint32_t hi = edit::shift_up((int)(uint32_t)(first >> 32), (int)(uint32_t)(v >> 32));
    return ((type)hi << 32) | lo;
  }
};

template <>
struct Cell<false> {
  using type = uint32_t;
  static constexpr type kSub = 1, kIns = 1, kDel = 1;
  __device__ static type col0(int j) { return (type)j; }
  __device__ static type row0(int i) { return (type)i; }
  __device__ static uint32_t dist(type c) { return c; }
  __device__ static type readlane(type v, int l) {
    return (type)__builtin_amdgcn_readlane((int)v, l);
  }
  __device__ static type shift_up(type first, type v) {
    return (type)edit::shift_up((int)first, (int)v);
  }
};

// D[la][lb] of a[0..la) against b[0..lb), the same value in every lane. 0 <= la, lb <= kMaxLen,
// both wave-uniform; the whole wave calls. row: lb cells of this wave's own global memory, used
// when la > 64 only.
template <bool OPS>
__device__ __forceinline__ typename Cell<OPS>::type edit_wave(const int* __restrict__ a, int la,
                                                              const int* __restrict__ b, int lb,
                                                              int lane,
                                                              typename Cell<OPS>::type* row) {
  using C = Cell<OPS>;
  using T = typename C::type;
  if (la == 0) return C::col0(lb);
  if (lb == 0) return C::row0(la);
  const int nb = (la + 63) >> 6;
  T cur = 0;
  int an = lane < la ? a[lane] : 0;  // the reference tokens too are loaded a band ahead
  for (int band = 0; band < nb; ++band) {
    const bool last = band + 1 == nb;
    const int i = band * 64 + lane + 1;
    const int ai = an;
    an = i + 64 <= la ? a[i + 63] : 0;
    // the last band stops once the lane of row la has its column lb
    const int nsteps = lb + (last ? ((la - 1) & 63) : 63);
    cur = C::row0(i);       // D[i][0]: the left neighbour of column 1
    T up = C::row0(i - 1);  // D[i-1][0]: becomes the diagonal neighbour of column 1
    int tok = 0;
    // chunks: tokens b[s0 + lane] and the previous band's cells of columns s0 + lane + 1. The
    // pass at s0 = -64 only loads the first chunk, so that every load is issued at one place, a
    // chunk ahead of its use.
    int bn = 0;
    T rn = 0;
    for (int s0 = -64; s0 < nsteps; s0 += 64) {
      const int bc = bn;
      const T rc = rn;
      const int nx = s0 + 64 + lane;
      bn = nx < lb ? b[nx] : 0;
      rn = (band > 0 && nx < lb) ? row[nx] : 0;
      const int send = s0 < 0 ? 0 : (nsteps - s0 < 64 ? nsteps - s0 : 64);
      T park = 0;  // lane 63's cell of step s0 + lane: column s0 + lane - 62
      for (int k = 0; k < send; ++k) {
        const int s = s0 + k;
        const int j = s - lane + 1;
        const T in0 = band == 0 ? C::col0(s + 1) : C::readlane(rc, k);
        const T diag = up;
        up = C::shift_up(in0, cur);
        tok = shift_up(__builtin_amdgcn_readlane(bc, k), tok);
        T best = diag + C::kSub;
        const T cu = up + C::kDel, cl = cur + C::kIns;
        if (C::dist(cu) < C::dist(best)) best = cu;
        if (C::dist(cl) < C::dist(best)) best = cl;
        if (tok == ai) best = diag;
        if (j >= 1 && j <= lb) cur = best;
        if (!last) {
          const T c63 = C::readlane(cur, 63);
          if (lane == k) park = c63;
        }
      }
      if (!last) {
        const int c = s0 + lane - 63;  // column index - 1
        if (lane < send && c >= 0 && c < lb) row[c] = park;
      }
    }
    // this band's stores before the next band's loads (one wave, one CU)
    if (!last) __threadfence_block();
  }
  return C::readlane(cur, (la - 1) & 63);
}

}  // namespace edit
}  // namespace ob
