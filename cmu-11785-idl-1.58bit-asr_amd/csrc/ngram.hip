// ngram.hip — back-off n-gram LM shallow fusion (layout, probe routine and scoring rule:
// ob_ngram.h): the host table builder and host scorer, and the two device scorers.
//
//   builder       host C. Entries are sorted by key and inserted in that order into a zeroed
//                 table, so the same entries in any order give the same bytes. The table starts at
//                 the smallest power of two >= 2 x the entry count and doubles until every entry
//                 sits within 64 slots of its home (max_probe, the lookup's bound).
//   step          per search step, one launch: two rows per wave, a row on 32 lanes. The row
//                 derives its context from its parent's stored context (one uint64) and its own
//                 last token and stores it; lanes 0..2 of the row each look up one context
//                 h[-m:] (the back-off chain, once per row, broadcast by three shuffles); lanes
//                 0..K-1 score one candidate each: the home-slot gathers of all len(h) + 1
//                 candidate keys and of the lane's context key are issued before any is examined,
//                 five independent 16-byte loads per lane in flight (a lane without a key reads
//                 slot 0); the rare continued probes follow one by one. The dependent chain of a
//                 launch is three loads long: the row's arguments, the parent's context, the
//                 gathers.
//   seq logprob   one block of 64 threads per hypothesis row, a thread per position: a
//                 position's context comes straight from the three tokens before it, so all
//                 positions are independent; the per-token scores meet in LDS and thread 0 adds
//                 them in ascending position, float64.
//
// No atomics, every word one writer, every loop bounded by max_probe, K or T; every sum in the
// fixed order of the rule: bitwise reproducible, whichever slot holds a prefix.
#include <algorithm>
#include <numeric>
#include <vector>

#include "ob_launch.h"
#include "ob_ngram.h"

namespace ob {

using namespace ngram;

namespace {

constexpr int kNgRowLanes = 32;  // lanes per row of the step kernel (K <= 32)

__global__ __launch_bounds__(64) void ngram_step_kernel(
    const Entry* __restrict__ tab, uint64_t mask, int max_probe, int order, int V, double unk,
    const int* __restrict__ topi, const int64_t* __restrict__ tok, const int* __restrict__ len,
    const int* __restrict__ link, const uint8_t* __restrict__ skip, int64_t R, int K, int bos,
    const uint64_t* __restrict__ ctx_in, uint64_t* __restrict__ ctx_out,
    double* __restrict__ lmsc) {
  const int lane = threadIdx.x;
  const int sub = lane % kNgRowLanes;
  const int base = lane - sub;
  const int64_t row_raw = (int64_t)blockIdx.x * (64 / kNgRowLanes) + lane / kNgRowLanes;
  const int64_t row = row_raw < R ? row_raw : R - 1;
  // everything the row's context and candidates need, in flight together (plain reads of the
  // search's own arrays; a skipped row's values are not used)
  const uint8_t sk = skip[row];
  const int n = len[row];
  const int64_t tk = tok[row];
  int par = link[2 * row];
  const int wq = topi[row * K + (sub < K ? sub : 0)];
  // (the values are pinned here so that their loads leave together with skip's, ahead of the
  // branch, not one after the other behind it)
  asm volatile("" ::"v"(n), "v"(tk), "v"(par), "v"(wq));
  const bool live = row_raw < R && sk == 0;
  if (__ballot(live) == 0ull) return;

  // the row's context: [bos] for the empty prefix, [bos, tok] one step later, else the parent's
  // stored context and the row's last token
  const uint64_t root = ng_push(0ull, bos);
  uint64_t ctx = root;
  if (live && n >= 1) {
    uint64_t pc = root;
    if (n > 1) {
      par = par < 0 ? 0 : (par >= R ? (int)(R - 1) : par);
      pc = ctx_in[par];
    }
    ctx = ng_push(pc, tk);
  }
  if (live && sub == 0) ctx_out[row] = ctx;
  const int hl = ng_ctx_len(ctx, order);

  const bool cand = live && sub < K;
  const int w = cand ? wq : -1;
  const bool look = cand && w >= 0 && w < V && w <= kMaxId;
  const bool chain_lane = live && sub < kMaxOrder - 1 && sub + 1 <= hl;
  const uint64_t ckey = ctx & ng_fields(sub < kMaxOrder - 1 ? sub + 1 : 0);
  const uint64_t wf = (uint64_t)(look ? w : 0) + 1ull;

  // Every first gather of the lane before any is examined: the candidate's len(h) + 1 keys and
  // the lane's context key, five independent 16-byte loads. A lane without a key reads slot 0
  // and ignores it, so the loads are unconditional and leave together.
  Entry ce, e[kMaxOrder];
#pragma unroll
  for (int m = 0; m < kMaxOrder; ++m) {
    const uint64_t key = ((ctx & ng_fields(m)) << 16) | wf;
    e[m] = tab[(look && m <= hl) ? (ng_mix(key) & mask) : 0ull];
  }
  ce = tab[chain_lane ? (ng_mix(ckey) & mask) : 0ull];

  bool hit[kMaxOrder];
  float lp[kMaxOrder];
#pragma unroll
  for (int m = 0; m < kMaxOrder; ++m) {
    float bo = 0.0f;
    lp[m] = 0.0f;
    hit[m] = look && m <= hl &&
             ng_resolve(tab, mask, max_probe, ((ctx & ng_fields(m)) << 16) | wf, e[m], lp[m], bo,
                        nullptr);
  }
  float c_lp = 0.0f, c_bo = 0.0f;
  const bool c_has = chain_lane && ng_resolve(tab, mask, max_probe, ckey, ce, c_lp, c_bo, nullptr);
  Chain c;
  c.has[0] = false;
  c.bo[0] = 0.0f;
#pragma unroll
  for (int m = 1; m < kMaxOrder; ++m) {  // the chain, from the lanes that looked it up
    c.has[m] = __shfl((int)c_has, base + m - 1) != 0;
    c.bo[m] = __shfl(c_bo, base + m - 1);
  }
  if (cand) lmsc[row * K + sub] = w < 0 ? -(double)INFINITY : ng_combine(hl, hit, lp, c, unk);
}

__global__ __launch_bounds__(64) void ngram_seq_logprob_kernel(
    const Entry* __restrict__ tab, uint64_t mask, int max_probe, int order, int V, double unk,
    const int* __restrict__ hyp, const int* __restrict__ hyp_len, int T, int bos, int eos,
    double* __restrict__ lm, double* __restrict__ tok_lm) {
  __shared__ double s_sc[64];
  const int64_t row = blockIdx.x;
  const int lane = threadIdx.x;
  const int L = hyp_len[row];
  double* trow = tok_lm ? tok_lm + row * (int64_t)(T + 1) : nullptr;
  if (L < 0) {  // an absent row
    if (lane == 0) lm[row] = -(double)INFINITY;
    if (trow)
      for (int j = lane; j <= T; j += 64) trow[j] = 0.0;
    return;
  }
  const int n = L > T ? T : L;
  const int* y = hyp + row * (int64_t)T;
  double total = 0.0;  // (thread 0's)
  for (int j0 = 0; j0 <= n; j0 += 64) {
    const int j = j0 + lane;
    double sc = 0.0;
    if (j <= n) {
      uint64_t ctx = 0ull;
#pragma unroll
      for (int q = 3; q >= 1; --q) {  // the three ids before position j of [bos] + y
        const int p = j - q;
        if (p >= -1) ctx = ng_push(ctx, p < 0 ? bos : y[p]);
      }
      const int w = j < n ? y[j] : eos;
      const int hl = ng_ctx_len(ctx, order);
      const Chain c = ng_chain(tab, mask, max_probe, ctx, hl, nullptr);
      sc = ng_score(tab, mask, max_probe, order, V, unk, ctx, c, w, nullptr);
      if (trow) trow[j] = sc;
    }
    s_sc[lane] = sc;
    __syncthreads();
    if (lane == 0) {
      const int m = n + 1 - j0 < 64 ? n + 1 - j0 : 64;
      for (int q = 0; q < m; ++q) total += s_sc[q];
    }
    __syncthreads();
  }
  if (lane == 0) lm[row] = total;
  if (trow)
    for (int j = n + 1 + lane; j <= T; j += 64) trow[j] = 0.0;
}

}  // namespace

bool ngram_supported(int64_t order, int64_t V, int64_t K) {
  return order >= 1 && order <= kMaxOrder && V >= 1 && V <= kMaxId + 1 && K >= 1 &&
         K <= kNgRowLanes;
}

int64_t ngram_table_slots(int64_t n_entries) {
  if (n_entries < 0 || n_entries > (int64_t)1 << 40) return 0;
  int64_t s = 8;
  while (s < 2 * n_entries) s <<= 1;
  return s;
}

// -> 0 ok; 1 a key is 0, has a gap between its fields, or occurs twice; 2 the table is too
// small (*slots says what is needed)
int ngram_table_build(const uint64_t* keys, const float* vals, int64_t n, void* table,
                      size_t table_bytes, int64_t* slots, int* max_probe) {
  std::vector<int64_t> idx((size_t)n);
  std::iota(idx.begin(), idx.end(), (int64_t)0);
  std::sort(idx.begin(), idx.end(), [&](int64_t a, int64_t b) { return keys[a] < keys[b]; });
  for (int64_t i = 0; i < n; ++i) {
    const uint64_t k = keys[idx[i]];
    if (k == 0 || (i > 0 && k == keys[idx[i - 1]])) return 1;
    bool seen_zero = false;
    for (int f = 0; f < 4; ++f) {
      const bool z = ((k >> (16 * f)) & 0xFFFFull) == 0;
      if (!z && seen_zero) return 1;
      seen_zero = seen_zero || z;
    }
  }
  int64_t s = ngram_table_slots(n);
  std::vector<Entry> tab;
  int worst = 0;
  for (;; s <<= 1) {
    tab.assign((size_t)s, Entry{0ull, 0.0f, 0.0f});
    const uint64_t mask = (uint64_t)s - 1;
    worst = n > 0 ? 0 : 1;
    for (int64_t i = 0; i < n; ++i) {
      const int64_t e = idx[i];
      uint64_t p = ng_mix(keys[e]) & mask;
      int run = 1;
      while (tab[p].key != 0) {
        p = (p + 1) & mask;
        ++run;
      }
      tab[p] = Entry{keys[e], vals[2 * e], vals[2 * e + 1]};
      worst = std::max(worst, run);
    }
    if (worst <= kProbeLimit) break;
  }
  *slots = s;
  *max_probe = worst;
  if (!table || table_bytes < (size_t)s * sizeof(Entry)) return 2;
  std::copy(tab.begin(), tab.end(), static_cast<Entry*>(table));
  return 0;
}

void ngram_score_host(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                      double unk_logp, const uint64_t* ctx, const int* w, int64_t Q, double* out,
                      int* probes) {
  const Entry* tab = static_cast<const Entry*>(table);
  const uint64_t mask = (uint64_t)slots - 1;
  for (int64_t q = 0; q < Q; ++q) {
    int np = 0;
    const uint64_t c = ctx[q] & kCtxMask;
    const Chain ch = ng_chain(tab, mask, max_probe, c, ng_ctx_len(c, order), &np);
    out[q] = ng_score(tab, mask, max_probe, order, (int)V, unk_logp, c, ch, w[q], &np);
    if (probes) probes[q] = np;
  }
}

void launch_ngram_step(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                       double unk_logp, const int* topi, const int64_t* tok, const int* len,
                       const int* link, const uint8_t* skip, int64_t B, int64_t N, int64_t K,
                       int bos, const uint64_t* ctx_in, uint64_t* ctx_out, double* lmsc,
                       hipStream_t s) {
  const int64_t R = B * N;
  if (R == 0) return;
  constexpr int kRpw = 64 / kNgRowLanes;
  hipLaunchKernelGGL(ngram_step_kernel, dim3((unsigned)ceil_div(R, kRpw)), dim3(64), 0, s,
                     static_cast<const Entry*>(table), (uint64_t)slots - 1, max_probe, order,
                     (int)V, unk_logp, topi, tok, len, link, skip, R, (int)K, bos, ctx_in, ctx_out,
                     lmsc);
}

void launch_ngram_seq_logprob(const void* table, int64_t slots, int max_probe, int order,
                              int64_t V, double unk_logp, const int* hyp, const int* hyp_len,
                              int64_t R, int64_t T, int bos, int eos, double* lm, double* tok_lm,
                              hipStream_t s) {
  if (R == 0) return;
  hipLaunchKernelGGL(ngram_seq_logprob_kernel, dim3((unsigned)R), dim3(64), 0, s,
                     static_cast<const Entry*>(table), (uint64_t)slots - 1, max_probe, order,
                     (int)V, unk_logp, hyp, hyp_len, (int)T, bos, eos, lm, tok_lm);
}

}  // namespace ob
