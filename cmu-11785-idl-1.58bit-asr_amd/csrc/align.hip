// align.hip — CTC forced alignment: the Viterbi path of a given token sequence through the CTC
// trellis of the encoder's logits, in float64, with the frame span and the score of every token.
//
//   emission kernel   one wave per (utterance, frame) with t < lens[b]: the frame's float64
//                     log-sum-exp (ctc_frame_lse_wave, the prefix scorer's), then the emission row
//                     E[b][t][0..tlen] = x[t][blank], x[t][target_0], ... in fp64, x[t][v] =
//                     (double)z[t][v] - flse[t]. The logits are read once; the recursion never
//                     gathers at stride V. A target token outside [0, V) or equal to blank is never
//                     used as an index: its emission is -inf, which makes the utterance infeasible.
//   trellis kernel    one block per utterance. v_t(s) = max(v_{t-1}(s), v_{t-1}(s-1), v_{t-1}(s-2)
//                     where the skip is allowed) + E[t][label(s)] over the extended labels of
//                     ctc.hip; stay wins a tie over s-1, which wins over s-2 (strict > in that
//                     order). States are spread over the threads, 1 or 4 per thread; the previous
//                     row lives in LDS, the steps are separated by the LDS-only barrier, a state's
//                     next kAlRing emissions travel in registers ahead of the dependent chain, and
//                     one back-pointer byte per (t, s) goes to the workspace. At the last frame the
//                     final token state wins a tie against the trailing blank. One thread walks the
//                     back-pointers into LDS; the block then writes path, span and tok_score in
//                     parallel: token u's span is the run of frames on state 2u + 1, tok_score the
//                     sum of its emissions over the span in frame order.
//
// No atomics, every word one writer, every sum in frame order: an utterance gets the same bits in
// every batch slot and for every padded T' and S.
#include <math.h>

#include "ob_ctc.h"
#include "ob_launch.h"

namespace ob {

namespace {

constexpr int kAlFrameWaves = 4;
constexpr int kAlThreads = 256;
constexpr int kAlMaxS = 511;                    // the CTC loss's limit
constexpr int kAlMaxStates = 2 * kAlMaxS + 1;
constexpr int kAlMaxT = 4096;
constexpr int kAlRing = 8;                      // emissions in flight ahead of the recursion

__device__ __forceinline__ int clamp_len(int64_t n, int hi) {
  return (int)(n < 0 ? 0 : (n > hi ? hi : n));
}

__global__ __launch_bounds__(64 * kAlFrameWaves) void align_emission_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ lens,
    const int* __restrict__ targets, const int* __restrict__ tlen, int64_t rows, int T, int V,
    int S, int blank, double* __restrict__ E) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kAlFrameWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t b = row / T;
  const int t = (int)(row - b * T);
  if (t >= clamp_len(lens[b], T)) return;
  const float* x = logits + row * (int64_t)V;
  const double fl = ctc_frame_lse_wave(x, V, lane);
  const int L = clamp_len(tlen[b], S);
  double* e = E + row * (int64_t)(S + 1);
  for (int c = lane; c <= L; c += 64) {
    const int tok = c == 0 ? blank : targets[b * (int64_t)S + c - 1];
    const bool ok = c == 0 || (tok >= 0 && tok < V && tok != blank);
    e[c] = ok ? (double)x[tok] - fl : -(double)INFINITY;
  }
}

// The recursion over the frames, NSLOT states per thread (s = threadIdx.x + k * kAlThreads).
// Leaves the last row in buf[(T - 1) & 1]; T >= 1.
template <int NSLOT>
__device__ __forceinline__ void align_trellis(const double* __restrict__ Eb,
                                              const int* __restrict__ tg, int T, int NS, int SE,
                                              int SS, double (*buf)[kAlMaxStates + 1],
                                              uint8_t* __restrict__ bpb) {
  const double kNegInf = -(double)INFINITY;
  const int tl = T - 1;
  bool act[NSLOT], skip[NSLOT];
  const double* col[NSLOT];
  double ring[NSLOT][kAlRing];
#pragma unroll
  for (int k = 0; k < NSLOT; ++k) {
    const int s = threadIdx.x + k * kAlThreads;
    act[k] = s < NS;
    // the skip rule of ctc.hip: a token state whose token differs from the previous token's
    skip[k] = act[k] && (s & 1) && s >= 3 && tg[s >> 1] != tg[(s >> 1) - 1];
    col[k] = Eb + (act[k] && (s & 1) ? (s >> 1) + 1 : 0);
#pragma unroll
    for (int i = 0; i < kAlRing; ++i) ring[k][i] = col[k][(int64_t)(i < tl ? i : tl) * SE];
  }
  for (int t0 = 0; t0 < T; t0 += kAlRing) {
#pragma unroll
    for (int i = 0; i < kAlRing; ++i) {
      const int t = t0 + i;
      if (t >= T) break;  // block-uniform
      double* cur = buf[t & 1];
      const double* prev = buf[(t & 1) ^ 1];
#pragma unroll
      for (int k = 0; k < NSLOT; ++k) {
        const int s = threadIdx.x + k * kAlThreads;
        if (act[k]) {
          const double l = ring[k][i];
          double best;
          int d = 0;
          if (t == 0) {
            best = s <= 1 ? 0.0 : kNegInf;
          } else {
            best = prev[s];
            const double x1 = s >= 1 ? prev[s - 1] : kNegInf;
            const double x2 = skip[k] ? prev[s - 2] : kNegInf;
            if (x1 > best) { best = x1; d = 1; }
            if (x2 > best) { best = x2; d = 2; }
          }
          cur[s] = best + l;
          bpb[(int64_t)t * SS + s] = (uint8_t)d;
        }
        // the slot's next value (frame t + kAlRing), issued after l's last use
        ring[k][i] = col[k][(int64_t)(t + kAlRing < tl ? t + kAlRing : tl) * SE];
      }
      lds_barrier();
    }
  }
}

__global__ __launch_bounds__(kAlThreads) void align_trellis_kernel(
    const double* __restrict__ E, const int64_t* __restrict__ lens,
    const int* __restrict__ targets, const int* __restrict__ tlen, int Tp, int S, int blank,
    int walk, uint8_t* __restrict__ bp, int* __restrict__ path, int* __restrict__ span,
    double* __restrict__ tok_score, double* __restrict__ score) {
  __shared__ double buf[2][kAlMaxStates + 1];
  __shared__ uint16_t st[kAlMaxT];      // the path's state per frame
  __shared__ int sp[2][kAlMaxS + 1];    // (first frame, last frame + 1) per token
  __shared__ double sc_s;
  const double kNegInf = -(double)INFINITY;
  const int64_t b = blockIdx.x;
  const int T = clamp_len(lens[b], Tp);
  const int L = clamp_len(tlen[b], S);
  const int NS = 2 * L + 1;
  const int SE = S + 1, SS = 2 * S + 1;
  const int* tg = targets + b * (int64_t)S;
  const double* Eb = E + b * (int64_t)Tp * SE;
  uint8_t* bpb = bp + b * (int64_t)Tp * SS;

  if (T > 0) {
    if (NS <= kAlThreads)
      align_trellis<1>(Eb, tg, T, NS, SE, SS, buf, bpb);
    else
      align_trellis<(kAlMaxStates + kAlThreads - 1) / kAlThreads>(Eb, tg, T, NS, SE, SS, buf, bpb);
  }
  __syncthreads();  // the back-pointers in global memory, for the walk below
  if (threadIdx.x == 0) {
    double sc;
    int s = 0;
    if (T == 0) {
      sc = L == 0 ? 0.0 : kNegInf;
    } else {
      const double* last = buf[(T - 1) & 1];
      s = NS - 1;
      sc = last[s];
      if (NS >= 2 && last[NS - 2] >= sc) {  // the final token wins a tie against the blank
        s = NS - 2;
        sc = last[s];
      }
    }
    if (!(sc > kNegInf)) sc = kNegInf;  // no alignment (a NaN logit counts as none)
    sc_s = sc;
    score[b] = sc;
    if (walk && sc > kNegInf)
      for (int t = T - 1; t >= 0; --t) {
        st[t] = (uint16_t)s;
        if (t > 0) s -= bpb[(int64_t)t * SS + s];
      }
  }
  if (!walk) return;  // the recursion alone (timing): score only
  __syncthreads();
  const bool ok = sc_s > kNegInf;
  for (int t = threadIdx.x; t < Tp; t += kAlThreads) {
    int p = -1;
    if (ok && t < T) {
      const int s = st[t];
      p = (s & 1) ? tg[s >> 1] : blank;
      if (s & 1) {  // a token state is one contiguous run of frames: one writer per end
        if (t == 0 || st[t - 1] != s) sp[0][s >> 1] = t;
        if (t == T - 1 || st[t + 1] != s) sp[1][s >> 1] = t + 1;
      }
    }
    path[b * (int64_t)Tp + t] = p;
  }
  __syncthreads();
  for (int u = threadIdx.x; u < S; u += kAlThreads) {
    int f = -1, e = -1;
    double acc = 0.0;
    if (ok && u < L) {
      f = sp[0][u];
      e = sp[1][u];
      for (int t = f; t < e; ++t) acc += Eb[(int64_t)t * SE + u + 1];
    }
    span[(b * (int64_t)S + u) * 2] = f;
    span[(b * (int64_t)S + u) * 2 + 1] = e;
    tok_score[b * (int64_t)S + u] = acc;
  }
}

size_t round8(size_t n) { return (n + 7) & ~size_t(7); }

}  // namespace

bool ctc_align_supported(int64_t Tp, int64_t S) {
  return Tp >= 1 && Tp <= kAlMaxT && S >= 0 && S <= kAlMaxS;
}

// E fp64 [B][T'][S + 1], then the back-pointers uint8 [B][T'][2S + 1]
size_t ctc_align_workspace(int64_t B, int64_t Tp, int64_t S) {
  if (!ctc_align_supported(Tp, S) || B < 0) return 0;
  const unsigned __int128 rows = (unsigned __int128)B * Tp;
  const unsigned __int128 bytes = rows * (S + 1) * sizeof(double) + rows * (2 * S + 1) + 8;
  return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : round8((size_t)bytes);
}

void launch_ctc_align(const float* logits, const int64_t* lens, const int* targets,
                      const int* tlen, int64_t B, int64_t Tp, int64_t V, int64_t S, int blank,
                      int stages, void* ws, int* path, int* span, double* tok_score,
                      double* score, hipStream_t s) {
  const int64_t rows = B * Tp;
  if (rows == 0) return;
  double* E = static_cast<double*>(ws);
  uint8_t* bp = static_cast<uint8_t*>(ws) + sizeof(double) * (size_t)(rows * (S + 1));
  if (stages & 1)
    hipLaunchKernelGGL(align_emission_kernel, dim3((unsigned)ceil_div(rows, kAlFrameWaves)),
                       dim3(64 * kAlFrameWaves), 0, s, logits, lens, targets, tlen, rows, (int)Tp,
                       (int)V, (int)S, blank, E);
  if (stages & 2)
    hipLaunchKernelGGL(align_trellis_kernel, dim3((unsigned)B), dim3(kAlThreads), 0, s,
                       (const double*)E, lens, targets, tlen, (int)Tp, (int)S, blank,
                       (stages & 4) ? 1 : 0, bp, path, span, tok_score, score);
}

}  // namespace ob
