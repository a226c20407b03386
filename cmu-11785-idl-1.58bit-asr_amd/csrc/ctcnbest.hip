// ctcnbest.hip — minimum-WER training over the CTC n-best: the CTC log-likelihood of every
// entry of an n-best straight from the CTC head's logits, the expected-error loss over the
// entries' posterior and the gradient w.r.t. the logits (the ABI text is in
// include/onebit_hip.h).
//
// The N entries of an utterance share its frames, so the row pass (max, log-sum-exp) runs once
// per frame and only gathers N compact rows: lpc[(b N + k) T + t][0 .. Th], index 0 blank and
// 1 + u token u of entry k. The B N compact problems then go through the training CTC's own
// alpha / beta launch (ctc.hip: launch_ctc_alpha_beta), blank' = 0, V' = Th + 1.
//
// Gradient: with c_k = dL/dll_k, dll_k/dx[t][v] = occ_k[t][v] - softmax[t][v], so
//   dL/dx[t][v] = sum_k c_k occ_k[t][v] - (sum_k c_k) softmax[t][v].
// The minimum-WER coefficients sum to zero over an utterance's entries, the softmax term
// vanishes, and what is left is non-zero only at blank and at the n-best's tokens: the kernel
// zero-fills the row and adds the entries' label columns, entry after entry (dense == 0). A
// general upstream gradient of ll (dense != 0) writes the softmax term first. Entries share
// columns, so their adds are separated by a block barrier: a fixed order, no atomics.
#include <math.h>

#include "ob_ctc.h"
#include "ob_launch.h"
#include "ob_mma.h"

namespace ob {

namespace {

constexpr int kThreads = 256;
constexpr int kMaxTh = 511;                // as the training CTC's target length
constexpr int kMaxStates = 2 * kMaxTh + 1;
constexpr int kMaxNbest = 32;              // as edit.hip's MAX_NBEST

__device__ __forceinline__ int clampi(int64_t v, int64_t lo, int64_t hi) {
  return (int)(v < lo ? lo : (v > hi ? hi : v));
}

// One block per frame (b, t). The t == 0 block also writes, per entry of utterance b, what does
// not depend on the frame: the expanded lengths of the B N compact problems (an absent entry
// k >= n_hyp[b] gets 0 frames: its recursions do nothing and its nll is +inf), the compact
// labels tgc[u] = 1 + (first u' with the same token) (0 for a token equal to blank) and, per
// extended-label state s, occ[s] = the next state with the same compact label (-1: none) and
// occ[SS + s] = 1 when s is the first state of its label (the chains the gradient walks).
__global__ __launch_bounds__(kThreads) void nbest_gather_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ lens, const int* __restrict__ hyp,
    const int* __restrict__ hyp_len, const int* __restrict__ n_hyp, int N, int T, int V, int Th,
    int blank, float* __restrict__ mls, float* __restrict__ lpc, int64_t* __restrict__ tgc,
    int* __restrict__ occ, int64_t* __restrict__ in_len, int64_t* __restrict__ tg_len) {
  __shared__ float red[kThreads / 64];
  __shared__ int lab_s[kMaxStates];
  const int64_t rowid = blockIdx.x;  // b * T + t
  const int b = (int)(rowid / T), t = (int)(rowid % T);
  const int nh = clampi(n_hyp[b], 0, N);
  const int Tb = clampi(lens[b], 0, T);
  const int SS = 2 * Th + 1;
  if (t == 0) {
    for (int k = 0; k < N; ++k) {
      const int64_t p = (int64_t)b * N + k;
      const bool present = k < nh;
      const int L = present ? clampi(hyp_len[p], 0, Th) : 0;
      if (threadIdx.x == 0) {
        in_len[p] = present ? Tb : 0;
        tg_len[p] = L;
      }
      if (!present) continue;  // block-uniform
      const int* hk = hyp + p * Th;
      const int NS = 2 * L + 1;
      for (int u = threadIdx.x; u < Th; u += kThreads) {
        int c = 0;
        if (u < L && hk[u] != blank) {
          int f = u;
          for (int q = 0; q < u; ++q)
            if (hk[q] == hk[u]) { f = q; break; }
          c = 1 + f;
        }
        tgc[p * Th + u] = c;
        if (u < L) lab_s[2 * u + 1] = c;
      }
      for (int st = 2 * threadIdx.x; st < NS; st += 2 * kThreads) lab_s[st] = 0;
      __syncthreads();
      int* ob = occ + p * 2 * SS;
      for (int st = threadIdx.x; st < NS; st += kThreads) {
        const int lab = lab_s[st];
        bool first = true;
        for (int q = 0; q < st; ++q)
          if (lab_s[q] == lab) { first = false; break; }
        int nx = -1;
        for (int q = st + 1; q < NS; ++q)
          if (lab_s[q] == lab) { nx = q; break; }
        ob[st] = nx;
        ob[SS + st] = first ? 1 : 0;
      }
      __syncthreads();  // lab_s is rewritten for the next entry
    }
  }
  if (t >= Tb) return;
  // the row's max and log-sum-exp: ctc_lse_gather_kernel's operations in its order
  const float* row = x + rowid * V;
  const bool vec = (V & 3) == 0;
  constexpr int kMaxQ = 8;
  const int nq = vec ? V / 4 : 0;
  f32x4 vals[kMaxQ];
  float m = -INFINITY;
  const bool regs = vec && nq <= kMaxQ * kThreads;
  if (regs) {
#pragma unroll
    for (int i = 0; i < kMaxQ; ++i) {
      const int q = threadIdx.x + i * kThreads;
      vals[i] = q < nq ? reinterpret_cast<const f32x4*>(row)[q]
                       : f32x4{-INFINITY, -INFINITY, -INFINITY, -INFINITY};
      m = fmaxf(m, fmaxf(fmaxf(vals[i][0], vals[i][1]), fmaxf(vals[i][2], vals[i][3])));
    }
  } else {
    for (int v = threadIdx.x; v < V; v += kThreads) m = fmaxf(m, row[v]);
  }
  m = ctc_block_reduce<kThreads>(m, true, red);
  float sum = 0.0f;
  if (regs) {
#pragma unroll
    for (int i = 0; i < kMaxQ; ++i) {
      const int q = threadIdx.x + i * kThreads;
      if (q < nq)
        sum += ((expf(vals[i][0] - m) + expf(vals[i][1] - m)) + expf(vals[i][2] - m)) +
               expf(vals[i][3] - m);
    }
  } else {
    for (int v = threadIdx.x; v < V; v += kThreads) sum += expf(row[v] - m);
  }
  sum = ctc_block_reduce<kThreads>(sum, false, red);
  const float logs = logf(sum);
  if (threadIdx.x == 0) {
    mls[2 * rowid] = m;
    mls[2 * rowid + 1] = logs;
  }
  // the compact rows of the utterance's present entries, from the one row
  const int W = Th + 1;
  for (int i = threadIdx.x; i < nh * W; i += kThreads) {
    const int k = i / W, c = i - k * W;
    const int64_t p = (int64_t)b * N + k;
    const int lab = c == 0 ? blank : clampi(hyp[p * Th + (c - 1)], 0, V - 1);  // padding: any column
    lpc[(p * T + t) * W + c] = (row[lab] - m) - logs;
  }
}

__global__ void nbest_ll_kernel(const float* __restrict__ nll, int64_t P, double* __restrict__ ll) {
  const int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (p < P) ll[p] = -(double)nll[p];
}

// One block, thread b takes utterance b (b strided); thread 0 then sums the utterances' losses
// in b order. fp64, every sum in ascending k.
__global__ __launch_bounds__(kThreads) void mwer_combine_kernel(
    const double* __restrict__ ll, const double* __restrict__ err, const int* __restrict__ n_hyp,
    double scale, int B, int N, double* __restrict__ loss, double* __restrict__ post,
    double* __restrict__ risk, double* __restrict__ coef) {
  for (int b = threadIdx.x; b < B; b += kThreads) {
    const int nh = clampi(n_hyp[b], 0, N);
    const double* l = ll + (int64_t)b * N;
    const double* e = err + (int64_t)b * N;
    double* po = post + (int64_t)b * N;
    double* co = coef + (int64_t)b * N;
    int live = 0;
    double m = -INFINITY;
    for (int k = 0; k < nh; ++k)
      if (isfinite(l[k])) {
        ++live;
        m = fmax(m, l[k]);
      }
    double z = 0.0;
    for (int k = 0; k < nh; ++k)
      if (isfinite(l[k])) z += exp(scale * (l[k] - m));
    double r = 0.0;
    for (int k = 0; k < N; ++k) {
      const bool lv = k < nh && isfinite(l[k]);
      const double pk = lv ? exp(scale * (l[k] - m)) / z : 0.0;
      po[k] = pk;
      if (lv) r += pk * e[k];
    }
    risk[b] = r;
    for (int k = 0; k < N; ++k) {
      const bool lv = live >= 2 && k < nh && isfinite(l[k]);
      co[k] = lv ? scale * po[k] * (e[k] - r) / (double)B : 0.0;
    }
  }
  __syncthreads();
  if (threadIdx.x != 0) return;
  double total = 0.0;
  for (int b = 0; b < B; ++b) {
    const int nh = clampi(n_hyp[b], 0, N);
    int live = 0;
    double es = 0.0;
    for (int k = 0; k < nh; ++k)
      if (isfinite(ll[(int64_t)b * N + k])) {
        ++live;
        es += err[(int64_t)b * N + k];
      }
    if (live >= 2) total += risk[b] - es / (double)live;
  }
  loss[0] = total / (double)B;
}

// One block per frame: the whole row of grad is written here (never read before).
__global__ __launch_bounds__(kThreads) void nbest_grad_kernel(
    const float* __restrict__ x, const int64_t* __restrict__ lens, const int* __restrict__ hyp,
    int N, int T, int V, int Th, int blank, const double* __restrict__ coef,
    const float* __restrict__ grad_out, int dense, const float* __restrict__ mls,
    const float* __restrict__ lpc, const int64_t* __restrict__ tgc,
    const int64_t* __restrict__ tg_len, const float* __restrict__ alpha,
    const float* __restrict__ beta, const float* __restrict__ nll, const int* __restrict__ occ,
    float* __restrict__ grad) {
  const int64_t rowid = blockIdx.x;
  const int b = (int)(rowid / T), t = (int)(rowid % T);
  const bool live = t < clampi(lens[b], 0, T);
  const float go = grad_out ? grad_out[0] : 1.0f;
  // the entries that contribute (block-uniform), and the sum of their coefficients in k order
  double csum = 0.0;
  bool any = false;
  if (live)
    for (int k = 0; k < N; ++k) {
      const double c = coef[(int64_t)b * N + k];
      if (c != 0.0 && !isinf(nll[(int64_t)b * N + k])) {
        csum += c;
        any = true;
      }
    }
  const float* row = x + rowid * V;
  float* g = grad + rowid * V;
  const bool soft = dense != 0 && any;
  const float sc = soft ? -(go * (float)csum) : 0.0f;
  const float m = soft ? mls[2 * rowid] : 0.0f, logs = soft ? mls[2 * rowid + 1] : 0.0f;
  if ((V & 3) == 0) {
    for (int q = threadIdx.x; q < V / 4; q += kThreads) {
      f32x4 o = {0.f, 0.f, 0.f, 0.f};
      if (soft) {
        const f32x4 v = reinterpret_cast<const f32x4*>(row)[q];
#pragma unroll
        for (int e = 0; e < 4; ++e) o[e] = expf((v[e] - m) - logs) * sc;
      }
      reinterpret_cast<f32x4*>(g)[q] = o;
    }
  } else {
    for (int v = threadIdx.x; v < V; v += kThreads)
      g[v] = soft ? expf((row[v] - m) - logs) * sc : 0.0f;
  }
  if (!any) return;
  __shared__ float xs[kMaxStates];
  __shared__ int nx[kMaxStates];
  __shared__ int own[kMaxStates];
  const int SS = 2 * Th + 1;
  const int W = Th + 1;
  for (int k = 0; k < N; ++k) {
    const int64_t p = (int64_t)b * N + k;
    const double c = coef[p];
    const float n = nll[p];
    if (c == 0.0 || isinf(n)) continue;  // block-uniform
    const float w = go * (float)c;
    const int NS = 2 * (int)tg_len[p] + 1;
    const int* ob = occ + p * 2 * SS;
    const float* a = alpha + (p * T + t) * SS;
    const float* be = beta + (p * T + t) * SS;
    // the row fill, and the previous entry's adds and LDS reads, are complete
    __syncthreads();
    for (int s = threadIdx.x; s < NS; s += kThreads) {
      xs[s] = a[s] + be[s];
      nx[s] = ob[s];
      own[s] = ob[SS + s];
    }
    __syncthreads();
    for (int s = threadIdx.x; s < NS; s += kThreads) {
      if (!own[s]) continue;  // not the first state of its label
      const int lab = (s & 1) ? (int)tgc[p * Th + (s >> 1)] : 0;  // compact label
      // occurrences of the label in state order, as ctc_logits_grad_kernel walks them
      float acc = xs[s];
      for (int q = nx[s]; q >= 0; q = nx[q]) acc = ctc_lse2(acc, xs[q]);
      const float l = lpc[(p * T + t) * W + lab];
      const int v = (s & 1) ? clampi(hyp[p * Th + (s >> 1)], 0, V - 1) : blank;  // vocabulary id
      g[v] += w * expf(acc + n - l);  // one owner per column within an entry
    }
  }
}

struct NbestWs {
  float *alpha, *beta, *nll, *lpc, *mls;
  int64_t *tgc, *in_len, *tg_len;
  int* occ;
  size_t total;
};

inline size_t up256(size_t v) { return (v + 255) & ~size_t(255); }

NbestWs split_nbest_ws(void* ws, int64_t B, int64_t N, int64_t T, int64_t Th) {
  const size_t P = (size_t)(B * N), SS = (size_t)(2 * Th + 1);
  NbestWs w;
  char* p = static_cast<char*>(ws);
  char* const p0 = p;
  w.alpha = reinterpret_cast<float*>(p);
  p += up256(sizeof(float) * P * (size_t)T * SS);
  w.beta = reinterpret_cast<float*>(p);
  p += up256(sizeof(float) * P * (size_t)T * SS);
  w.nll = reinterpret_cast<float*>(p);
  p += up256(sizeof(float) * P);
  w.lpc = reinterpret_cast<float*>(p);
  p += up256(sizeof(float) * P * (size_t)T * (size_t)(Th + 1));
  w.mls = reinterpret_cast<float*>(p);
  p += up256(sizeof(float) * 2 * (size_t)(B * T));
  w.tgc = reinterpret_cast<int64_t*>(p);
  p += up256(sizeof(int64_t) * (P * (size_t)Th + 8));
  w.in_len = reinterpret_cast<int64_t*>(p);
  p += up256(sizeof(int64_t) * P);
  w.tg_len = reinterpret_cast<int64_t*>(p);
  p += up256(sizeof(int64_t) * P);
  w.occ = reinterpret_cast<int*>(p);
  p += up256(sizeof(int) * 2 * P * SS);
  w.total = (size_t)(p - p0);
  return w;
}

}  // namespace

bool ctc_nbest_supported(int64_t N, int64_t Th) {
  return N >= 1 && N <= kMaxNbest && Th >= 0 && Th <= kMaxTh;
}

size_t ctc_nbest_workspace(int64_t B, int64_t N, int64_t T, int64_t Th) {
  return split_nbest_ws(nullptr, B, N, T, Th).total;
}

void launch_ctc_nbest_logprob(const float* x, const int64_t* lens, const int* hyp,
                              const int* hyp_len, const int* n_hyp, int64_t B, int64_t N,
                              int64_t T, int64_t V, int64_t Th, int blank, void* ws, double* ll,
                              hipStream_t s) {
  const NbestWs w = split_nbest_ws(ws, B, N, T, Th);
  const int64_t P = B * N;
  hipLaunchKernelGGL(nbest_gather_kernel, dim3((unsigned)(B * T)), dim3(kThreads), 0, s, x, lens,
                     hyp, hyp_len, n_hyp, (int)N, (int)T, (int)V, (int)Th, blank, w.mls, w.lpc,
                     w.tgc, w.occ, w.in_len, w.tg_len);
  launch_ctc_alpha_beta(w.lpc, w.tgc, w.in_len, w.tg_len, P, T, Th + 1, Th, 0, w.alpha, w.nll,
                        w.beta, s);
  hipLaunchKernelGGL(nbest_ll_kernel, dim3((unsigned)((P + kThreads - 1) / kThreads)),
                     dim3(kThreads), 0, s, (const float*)w.nll, P, ll);
}

void launch_mwer_combine(const double* ll, const double* err, const int* n_hyp, double scale,
                         int64_t B, int64_t N, double* loss, double* post, double* risk,
                         double* coef, hipStream_t s) {
  hipLaunchKernelGGL(mwer_combine_kernel, dim3(1), dim3(kThreads), 0, s, ll, err, n_hyp, scale,
                     (int)B, (int)N, loss, post, risk, coef);
}

void launch_ctc_nbest_grad(const float* x, const int64_t* lens, const int* hyp, int64_t B,
                           int64_t N, int64_t T, int64_t V, int64_t Th, int blank,
                           const double* coef, const float* grad_out, int dense, void* ws,
                           float* grad, hipStream_t s) {
  const NbestWs w = split_nbest_ws(ws, B, N, T, Th);
  hipLaunchKernelGGL(nbest_grad_kernel, dim3((unsigned)(B * T)), dim3(kThreads), 0, s, x, lens,
                     hyp, (int)N, (int)T, (int)V, (int)Th, blank, coef, grad_out, dense,
                     (const float*)w.mls, (const float*)w.lpc, (const int64_t*)w.tgc,
                     (const int64_t*)w.tg_len, (const float*)w.alpha, (const float*)w.beta,
                     (const float*)w.nll, (const int*)w.occ, grad);
}

}  // namespace ob
