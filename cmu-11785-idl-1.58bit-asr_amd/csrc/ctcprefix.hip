// ctcprefix.hip — the CTC prefix scorer of the joint CTC/attention beam search: for every beam
// row and each of its K attention candidates the log-probability that the transcript starts
// with (the row's prefix + the candidate), in float64, once per search step.
//
//   frame kernel    one wave per (utterance, frame) with t < lens[b]: the float64 log-sum-exp of
//                   the frame's fp32 CTC logits (row max, fp64 sum of exp(z - max), butterfly).
//                   x[t][v] = (double)z[t][v] - flse[t] is formed where it is used.
//   scorer step     one wave per row, or two rows per wave (one per half) when K <= 31. A row's
//                   prefix g has ONE stored state, [T'][2] fp64 = (gb[t], tot[t] = lse(gn[t],
//                   gb[t])): an extension needs nothing else of its parent (phi is gb or tot, the
//                   eos score is tot[T-1]). Two tables [R][T'][2] are used alternately: at a
//                   step the row first derives its own state from its parent's row of the input
//                   table (the parent row and the parent's last token as the joint beam step
//                   recorded them, the row's last token from tok, root iff len == 0) and stores
//                   it in the output table; its K candidates are scored from that state.
//                   Lane roles: lanes 0..K-1 of the half carry one candidate each (hn, psi), the
//                   "own" lane carries the row's state (gn, gb, tot). Both recursions have the
//                   form  u' = lse(u, P) + X ; v' = lse(Q, R) + Y  and run as the same
//                   instructions; a candidate's frame t needs the row's state at t - 1 only, so
//                   one loop serves both, the candidates one frame behind through a broadcast of
//                   (gb, tot). The chain is T long. The logit columns (a stride-V gather per
//                   lane), flse and the parent's state travel in registers one chunk of frames
//                   ahead of the recursion, so no load sits inside the dependent chain.
//
// No atomics, every word one writer, every loop bounded by lens[b] or K, every sum in a fixed
// order that depends on the prefix alone: bitwise reproducible, whichever slot holds a prefix.
#include <math.h>

#include "ob_ctc.h"
#include "ob_launch.h"

namespace ob {

namespace {

constexpr int kCpFrameWaves = 4;
constexpr int kCpChunk = 4;  // frames in flight ahead of the recursion

__global__ __launch_bounds__(64 * kCpFrameWaves) void ctc_frame_lse_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ lens, int64_t rows, int T, int V,
    double* __restrict__ flse) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kCpFrameWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t b = row / T;
  const int t = (int)(row - b * T);
  int64_t L = lens[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  if (t >= L) return;
  const double fl = ctc_frame_lse_wave(logits + row * (int64_t)V, V, lane);
  if (lane == 0) flse[row] = fl;
}

// log(exp(a) + exp(b)); -inf when both are
__device__ __forceinline__ double lse2(double a, double b) {
  const double m = fmax(a, b);
  if (m == -(double)INFINITY) return m;
  return m + log1p(exp(fmin(a, b) - m));
}

struct CpFrame {  // what one frame of the recursion reads
  float zc, zb;   // the lane's logit column, the blank column
  double fl;      // the frame's log-sum-exp
  double pb, pt;  // the parent's (gb, tot) one frame earlier
};

// RPW rows per wave: a row owns 64 / RPW lanes, candidates on its lanes 0..K-1, the row's own
// state on lane kOwn of them.
template <int RPW>
__global__ __launch_bounds__(64) void ctc_prefix_step_kernel(
    const float* __restrict__ logits, const double* __restrict__ flse,
    const int64_t* __restrict__ lens, const int* __restrict__ topi, const int64_t* __restrict__ tok,
    const int* __restrict__ len, const int* __restrict__ link, const uint8_t* __restrict__ skip,
    int64_t R, int N, int K, int Tp, int V, int blank, int eos,
    const double* __restrict__ st_in, double* __restrict__ st_out, double* __restrict__ cpsi) {
  constexpr int kLanes = 64 / RPW;
  constexpr int kOwn = RPW == 2 ? 31 : 32;
  const double kNegInf = -(double)INFINITY;
  const int lane = threadIdx.x;
  const int sub = lane % kLanes;
  const int64_t row_raw = (int64_t)blockIdx.x * RPW + lane / kLanes;
  const int64_t row = row_raw < R ? row_raw : R - 1;
  const bool live = row_raw < R && skip[row] == 0;
  if (__ballot(live) == 0ull) return;
  const int own_lane = lane - sub + kOwn;
  const bool own = sub == kOwn;
  const bool cand = sub < K;

  const int64_t b = row / N;
  int64_t T64 = lens[b];
  const int T = live ? (int)(T64 < 0 ? 0 : (T64 > Tp ? Tp : T64)) : 0;
  const int n = len[row];
  const bool root = n <= 0;        // the row's prefix is empty
  const bool par_root = n == 1;    // its parent's prefix is
  int64_t last64 = tok[row];
  const int last = root ? -1 : (int)(last64 < 0 ? 0 : (last64 >= V ? V - 1 : last64));
  int par = link[2 * row];
  par = par < 0 ? 0 : (par >= R ? (int)(R - 1) : par);
  const int par_last = link[2 * row + 1];
  const bool own_rep = !root && !par_root && par_last == last;  // last(parent) == the row's token

  int h = cand ? topi[row * K + sub] : -1;
  const bool is_pad = h < 0;
  const bool is_eos = h == eos;
  h = h < 0 ? 0 : (h >= V ? V - 1 : h);
  const bool rep = !root && h == last;  // the candidate repeats the prefix's last token
  const int col = own ? (root ? blank : last) : h;

  const float* zrow = logits + b * (int64_t)Tp * V;
  const double* frow = flse + b * (int64_t)Tp;
  const double* prow = st_in + (int64_t)par * Tp * 2;
  double* orow = st_out + row * (int64_t)Tp * 2;

  // frame t of this lane's row, clamped into the row's valid frames (a lane past its T keeps
  // loading its last frame and ignores it)
  auto fetch = [&](int t) {
    const int tc = t < T ? t : (T > 0 ? T - 1 : 0);
    const int tp = tc > 0 ? tc - 1 : 0;
    CpFrame f;
    f.zc = zrow[(int64_t)tc * V + col];
    f.zb = zrow[(int64_t)tc * V + blank];
    f.fl = frow[tc];
    f.pb = prow[2 * tp];
    f.pt = prow[2 * tp + 1];
    return f;
  };

  int Tmax = T;
#pragma unroll
  for (int o = 32; o >= kLanes; o >>= 1) {
    const int ot = __shfl_xor(Tmax, o);
    Tmax = ot > Tmax ? ot : Tmax;
  }

  // s1 = gn (own) / hn (candidate); s2 = gb / psi; s3 = tot (own); G_b, G_t: the row's (gb, tot)
  // of the previous frame, in every lane of the row
  double s1 = kNegInf, s2 = kNegInf, s3 = kNegInf, G_b = kNegInf, G_t = kNegInf;
  if (T > 0) {
    const CpFrame f = fetch(0);
    const double xc = (double)f.zc - f.fl, xb = (double)f.zb - f.fl;
    if (own) {
      s1 = par_root ? xc : kNegInf;   // gn[0]
      s2 = root ? xb : kNegInf;       // gb[0]
      s3 = root ? xb : s1;            // tot[0]
      orow[0] = s2;
      orow[1] = s3;
    } else {
      s1 = root ? xc : kNegInf;       // hn[0]
      s2 = s1;                        // psi
    }
  }
  G_b = __shfl(s2, own_lane);
  G_t = __shfl(s3, own_lane);

  CpFrame cur[kCpChunk], nxt[kCpChunk];
#pragma unroll
  for (int u = 0; u < kCpChunk; ++u) nxt[u] = fetch(1 + u);
  for (int t0 = 1; t0 < Tmax; t0 += kCpChunk) {
#pragma unroll
    for (int u = 0; u < kCpChunk; ++u) cur[u] = nxt[u];
    if (t0 + kCpChunk < Tmax) {
#pragma unroll
      for (int u = 0; u < kCpChunk; ++u) nxt[u] = fetch(t0 + kCpChunk + u);
    }
#pragma unroll
    for (int u = 0; u < kCpChunk; ++u) {
      const int t = t0 + u;
      if (t >= Tmax) break;
      const CpFrame& f = cur[u];
      const double xc = (double)f.zc - f.fl, xb = (double)f.zb - f.fl;
      double P, Q, Rr, X, Y;
      if (own) {
        P = root ? kNegInf : (own_rep ? f.pb : f.pt);  // phi of the row's own extension
        X = xc;
        Q = s1;
        Rr = s2;
        Y = xb;
      } else {
        P = rep ? G_b : G_t;                           // phi of the candidate
        X = xc;
        Q = s2;
        Rr = P + xc;
        Y = 0.0;
      }
      const double r1 = lse2(s1, P) + X;
      const double r2 = lse2(Q, Rr) + Y;
      const bool act = t < T;
      double r3 = s3;
      if (own) r3 = lse2(r1, r2);
      if (act) {
        s1 = r1;
        s2 = r2;
        s3 = r3;
        if (own) {
          orow[2 * t] = r2;
          orow[2 * t + 1] = r3;
        }
      }
      G_b = __shfl(s2, own_lane);
      G_t = __shfl(s3, own_lane);
    }
  }
  // G_t is now tot[T-1] of the row: log P_ctc(prefix | audio), the eos candidate's score
  if (live && cand) cpsi[row * K + sub] = (is_pad || T == 0) ? kNegInf : (is_eos ? G_t : s2);
}

}  // namespace

bool ctc_prefix_supported(int64_t N, int64_t K, int64_t Tp) {
  return N >= 1 && N <= K && K <= 32 && Tp >= 1 && Tp <= 256;
}

size_t ctc_prefix_workspace(int64_t B, int64_t N, int64_t K, int64_t Tp) {
  if (!ctc_prefix_supported(N, K, Tp) || B < 0) return 0;
  const unsigned __int128 bytes = (unsigned __int128)B * N * Tp * 2 * 2 * sizeof(double);
  return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : (size_t)bytes;
}

void launch_ctc_frame_lse(const float* logits, const int64_t* lens, int64_t B, int64_t Tp,
                          int64_t V, double* flse, hipStream_t s) {
  const int64_t rows = B * Tp;
  if (rows == 0) return;
  hipLaunchKernelGGL(ctc_frame_lse_kernel, dim3((unsigned)ceil_div(rows, kCpFrameWaves)),
                     dim3(64 * kCpFrameWaves), 0, s, logits, lens, rows, (int)Tp, (int)V, flse);
}

void launch_ctc_prefix_step(const float* logits, const double* flse, const int64_t* lens,
                            const int* topi, const int64_t* tok, const int* len, const int* link,
                            const uint8_t* skip, int64_t B, int64_t N, int64_t K, int64_t Tp,
                            int64_t V, int blank, int eos, const double* st_in, double* st_out,
                            double* cpsi, hipStream_t s) {
  const int64_t R = B * N;
  if (R == 0) return;
  if (K <= 31)
    hipLaunchKernelGGL(ctc_prefix_step_kernel<2>, dim3((unsigned)ceil_div(R, 2)), dim3(64), 0, s,
                       logits, flse, lens, topi, tok, len, link, skip, R, (int)N, (int)K, (int)Tp,
                       (int)V, blank, eos, st_in, st_out, cpsi);
  else
    hipLaunchKernelGGL(ctc_prefix_step_kernel<1>, dim3((unsigned)R), dim3(64), 0, s, logits, flse,
                       lens, topi, tok, len, link, skip, R, (int)N, (int)K, (int)Tp, (int)V, blank,
                       eos, st_in, st_out, cpsi);
}

}  // namespace ob
