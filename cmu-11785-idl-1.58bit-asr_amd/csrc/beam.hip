// beam.hip — batched CTC prefix beam search (eval path): without a language model, as the
// reference's, and with an n-gram LM inside the search ("LM fusion" below).
//
// Reference: onebit_asr/metrics.py:74-145 ``ctc_beam_search(logits [T, V], beam_size=10,
// blank_id=3, top_k_per_t=20)`` called per utterance by ``ctc_beam_search_batch``: a Python
// dict of prefix tuples -> (p_b, p_nb), rebuilt per frame from the 20 best tokens and pruned
// to the beam_size best totals. Here two launches decode a whole padded batch.
//
// The reference's transitions, for a live prefix with state (p_b, p_nb) and a frame's
// log-probabilities lp (all natural-log, fp64 here):
//   stay by blank          new[prefix].p_b      (+)= lse(p_b, p_nb) + lp[blank]
//   c == last(prefix)      new[prefix].p_nb     (+)= p_b + lp[c]      (p_b, NOT p_nb, and the
//                                                  repeated token is never appended: "a _ a"
//                                                  decodes to [a]; metrics.py:111-115)
//   otherwise              new[prefix + c].p_nb (+)= lse(p_b, p_nb) + lp[c]
// so no prefix ever holds two equal adjacent tokens, two different extensions never build the
// same tuple, and the only merge is an extension (i, c) whose result is a live prefix m:
// parent(m) == i and last(m) == c.
//
// frame kernel   one wave per (utterance, frame) row with t < lens[b]: row max, fp64 sum of
//                exp -> log-sum-exp, and the K = min(top_k, V) best logits in descending order
//                (ties to the lowest token index; selected on the raw fp32 logits, which is
//                monotone with lp; each lane offers the best of its own tokens and only the
//                round's winner scans again) as (token, fp64 lp). K == V: every token in
//                index order. Blank keeps its slot but is stored as token -1 (it is never a candidate);
//                lp[blank] goes to slot K. Output [B][T][K+1] fp64 + [B][T][K] int32, so the
//                serial phase never touches V.
// beam kernel    one wave per utterance, serial over its frames. The beam (<= 32 entries,
//                best first) lives in LDS: node id, parent id, last token, length, p_b, p_nb.
//                Per frame: item (i, 0) is "entry i stays", item (i, 1 + j) is "entry i
//                extended by candidate j"; an extension that equals a live entry m is folded
//                into m, and m's item moves to the smaller of the two item indices (the
//                reference's dict insertion order, which breaks exact score ties). beam_size
//                rounds of a wave arg-max over the item totals pick the survivors in order.
// prefix ids     a prefix's id is its slot in a per-utterance open-addressing table keyed by
//                (parent id, token), filled with 64-bit compare-and-swap: by induction from the
//                root, equal id <=> equal tuple, also for a prefix that was pruned and is built
//                again while one of its descendants is still live. The table is the trie: the
//                final walk reads (parent, token) back from the slots. At most L * beam keys
//                go into >= 2 * (L * beam + 1) slots; every probe loop is bounded by the table
//                size, and no loop here depends on data to end.
// n-best         ob_ctc_beam_search_nbest: the same two launches (one launcher for the three
//                forms, which picks the instantiation); the search kernel's other
//                instantiation ends by writing the first nbest entries of the final beam (which
//                LDS holds best first) instead of entry 0: lane e walks entry e's parents
//                through the table, the walks run in parallel. Entry 0 is the 1-best result.
// LM fusion      ob_ctc_beam_search_lm: the search kernel's third instantiation. Every entry also
//                carries its packed n-gram context, lm(y) (fp64, the rule's scores added in
//                ascending position) and the context's back-off chain (looked up once, when the
//                entry is created; all three move with the entry). Per frame the n * K extension
//                items are spread over the 64 lanes by item index; a live item (candidate >= 0 and
//                not the repeat) is scored with ob_ngram.h's ng_score, whose home-slot gathers
//                leave together, a dead one does no lookup; the result sits in a per-item array
//                beside s_val. The merges run on the CTC values as before; then every live item's
//                value becomes its key (ctc + lm_weight * lm) + ins_bonus * len, each operation
//                rounded, and the same arg-max rounds select on the keys. A survivor's p_nb is its
//                CTC value (computed again by the same addition), never the key. A merged item
//                keeps the live entry's LM value: lm(y) is a function of the tuple, the extension's
//                copy has the same bits. The epilogue adds the eos score, orders the final beam by
//                total (ties: the beam's order) and writes the first nbest entries.
// bias           ob_ctc_beam_search_bias: two more instantiations (with and without the LM) add the
//                phrase automaton of ob_bias.h. Every entry also carries its automaton state, kept
//                and bias(y) (all three move with the entry); the live extension items are stepped
//                spread over the 64 lanes as the LM items are and only the item's bias(y . c) sits
//                in LDS; a survivor steps its parent's (state, kept) again, as it rebuilds its
//                context. The key is the LM form's plus bias_weight * bias(y), the total closes
//                with bias_fin(y). Without an LM lm(y) is 0 and no table is read.
// Non-finite logits are outside the contract: NaN logits are never selected, NaN totals never
// survive, and every loop still has its fixed bound.
#include <math.h>

#include <type_traits>

#include "ob_bias.h"
#include "ob_launch.h"
#include "ob_ngram.h"

namespace ob {

namespace {

constexpr int kFrameWaves = 4;
constexpr int kMaxBeam = 32;
constexpr int kMaxTopK = 64;
constexpr int kRootId = 0x7fffffff;  // the empty prefix; table slots are < 2^30
constexpr int kNoId = 0x7ffffffe;    // never a live id
constexpr unsigned long long kEmptySlot = ~0ull;

__host__ __device__ inline unsigned beam_table_slots(int64_t frames, int beam) {
  const uint64_t need = 2ull * ((uint64_t)frames * (uint64_t)beam + 1ull);
  unsigned n = 2;
  for (int s = 1; s < 31 && n < need; ++s) n <<= 1;
  return n;
}

__global__ __launch_bounds__(64 * kFrameWaves) void beam_frame_kernel(
    const float* __restrict__ logits, const int64_t* __restrict__ lens, int64_t rows, int T, int V,
    int blank, int K, double* __restrict__ lp, int* __restrict__ tok) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * kFrameWaves + (threadIdx.x >> 6);
  if (row >= rows) return;
  const int64_t b = row / T;
  const int t = (int)(row - b * T);
  int64_t L = lens[b];
  L = L < 0 ? 0 : (L > T ? T : L);
  if (t >= L) return;  // the beam kernel reads frames below L only
  const float* x = logits + row * (int64_t)V;

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
  const double lse = (double)mx + log(sum);

  double* lrow = lp + row * (int64_t)(K + 1);
  int* trow = tok + row * (int64_t)K;
  if (lane == 0) lrow[K] = (double)x[blank] - lse;
  if (K == V) {  // no top-k limit: every token, in index order
    for (int j = lane; j < K; j += 64) {
      lrow[j] = (double)x[j] - lse;
      trow[j] = j == blank ? -1 : j;
    }
    return;
  }
  // Lane l owns tokens l, l + 64, ... and keeps its best one not taken yet; each of the K
  // rounds is a wave arg-max over the lanes' candidates (value descending, index ascending),
  // and only the lane whose candidate won scans its own tokens again, for its best one ranking
  // after the one it just gave away -- so the row is read about three times, not K times.
  float cv = 0.0f;
  int ci = V;  // V: this lane has nothing left
  for (int v = lane; v < V; v += 64) {
    const float e = x[v];
    if (e == e && (ci == V || e > cv)) {  // v ascends: the lowest index is kept on ties
      cv = e;
      ci = v;
    }
  }
  for (int r = 0; r < K; ++r) {
    float bv = cv;
    int bi = ci;
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi < V && (bi == V || ov > bv || (ov == bv && oi < bi))) {
        bv = ov;
        bi = oi;
      }
    }
    const bool found = bi < V;
    if (lane == 0) {
      trow[r] = (found && bi != blank) ? bi : -1;
      lrow[r] = found ? (double)bv - lse : -(double)INFINITY;
    }
    if (found && bi == ci) {  // mine was taken (token indices are unique to a lane)
      const float pv = cv;
      const int pi = ci;
      cv = 0.0f;
      ci = V;
      for (int v = lane; v < V; v += 64) {
        const float e = x[v];
        const bool after = e < pv || (e == pv && v > pi);  // false for NaN
        if (after && (ci == V || e > cv)) {
          cv = e;
          ci = v;
        }
      }
    }
  }
}

__device__ inline double lse2(double a, double b) {
  const double hi = a > b ? a : b;
  const double lo = a > b ? b : a;
  if (lo == -(double)INFINITY) return hi;
  return hi + log1p(exp(lo - hi));
}

// the LM arguments of the fused search (unused by the other instantiations)
struct BeamLm {
  const ngram::Entry* tab;
  uint64_t mask;
  int max_probe, order, V, bos, eos;
  double unk, lw, bonus;
  double *ctc, *lm, *total;
};

// (ctc + lw * lm) + bonus * n with the two products and the two sums rounded on their own
__device__ __forceinline__ double lm_key(double ctc, double lw, double lm, double bonus, int n) {
#pragma clang fp contract(off)
  const double pl = lw * lm;
  const double base = ctc + pl;
  const double pn = bonus * (double)n;
  return base + pn;
}

// the bias arguments of the biased search; the other instantiations take an empty struct
struct BeamBias {
  bias::Tables bt;
  double bw;
  double* out;
};
struct BeamNoBias {};

// key + bw * bias with the product and the sum rounded on their own
__device__ __forceinline__ double bias_key(double key, double bw, double bv) {
#pragma clang fp contract(off)
  const double pb = bw * bv;
  return key + pb;
}

// tokens of the prefix `id` (length len <= T) into dst[0..len), read back from the table
__device__ inline void walk_prefix(const unsigned long long* tab, unsigned tsize, int id, int len,
                                   int* dst) {
  for (int s = len - 1; s >= 0; --s) {
    int tk = -1;
    if ((unsigned)id < tsize) {
      const unsigned long long key =
          __hip_atomic_load(&tab[id], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
      tk = (int)(unsigned)(key & 0xffffffffull);
      id = (int)(unsigned)(key >> 32);
    }
    dst[s] = tk;
  }
}

// NBEST: the same search; the epilogue returns the first nbest entries of the final beam (in
// the beam's own order) through hyp / hyp_len / n_hyp / nscore instead of the best one.
// LM (with NBEST): the n-gram LM steers the pruning (see the head of the file); the epilogue
// orders the final beam by total and writes la.ctc / la.lm / la.total in place of nscore.
// BIAS (with NBEST; with or without LM): the phrase automaton adds bw * bias(y) to the LM form's
// key (lm(y) = 0 without LM) and bw * bias_fin(y) to its total, and ba.out receives bias_fin.
template <bool NBEST, bool LM = false, bool BIAS = false>
__global__ __launch_bounds__(64) void beam_search_kernel(
    const double* __restrict__ lp, const int* __restrict__ tok, const int64_t* __restrict__ lens,
    int T, int K, int beam, unsigned long long* __restrict__ table, int64_t table_stride,
    int* __restrict__ out, int* __restrict__ out_len, double* __restrict__ score, int nbest,
    int* __restrict__ hyp, int* __restrict__ hyp_len, int* __restrict__ n_hyp,
    double* __restrict__ nscore, BeamLm la,
    std::conditional_t<BIAS, BeamBias, BeamNoBias> ba) {
  static_assert(NBEST || !(LM || BIAS), "the fused search returns an n-best");
  constexpr bool KEYED = LM || BIAS;  // the pruning key is not the CTC value
  __shared__ int s_id[kMaxBeam], s_par[kMaxBeam], s_last[kMaxBeam], s_len[kMaxBeam];
  __shared__ int s_slot[kMaxBeam];  // the item index entry m's stay item sits at
  __shared__ double s_pb[kMaxBeam], s_pnb[kMaxBeam], s_tot[kMaxBeam];
  __shared__ double s_npb[kMaxBeam], s_npnb[kMaxBeam];
  __shared__ double s_lp[kMaxTopK];
  __shared__ int s_tok[kMaxTopK];
  __shared__ double s_val[kMaxBeam * (kMaxTopK + 1)];
  // LM: per entry the packed context, lm(y) and the context's back-off chain; per item the LM
  // value of the extension (one element each in the other instantiations)
  __shared__ unsigned long long s_ctx[LM ? kMaxBeam : 1];
  __shared__ double s_lm[LM ? kMaxBeam : 1];
  __shared__ ngram::Chain s_chain[LM ? kMaxBeam : 1];
  __shared__ double s_lmv[LM ? kMaxBeam * (kMaxTopK + 1) : 1];
  // BIAS: per entry the automaton state, kept and bias(y); per item bias(y . c)
  __shared__ int s_bst[BIAS ? kMaxBeam : 1];
  __shared__ double s_bkept[BIAS ? kMaxBeam : 1], s_bias[BIAS ? kMaxBeam : 1];
  __shared__ double s_bv[BIAS ? kMaxBeam * (kMaxTopK + 1) : 1];
  // the three per-item arrays are 16640 bytes each, the per-entry and per-candidate arrays
  // together below 8 KiB (54400 bytes in all with LM and BIAS)
  static_assert(3 * sizeof(double) * kMaxBeam * (kMaxTopK + 1) + 8192 <= 64 * 1024,
                "static LDS of the LM + bias instantiation within the 64 KiB limit");

  const int b = blockIdx.x;
  const int lane = threadIdx.x;
  int64_t L64 = lens[b];
  const int L = (int)(L64 < 0 ? 0 : (L64 > T ? T : L64));
  const int K1 = K + 1;
  const double kNaN = __longlong_as_double(0x7ff8000000000000ll);
  const double kNegInf = -(double)INFINITY;

  const unsigned tsize = beam_table_slots(L, beam);
  int shift = 64;
  for (unsigned n = tsize; n > 1; n >>= 1) --shift;  // <= 31 steps
  unsigned long long* tab = table + (int64_t)b * table_stride;
  for (unsigned i = lane; i < tsize; i += 64) tab[i] = kEmptySlot;
  if (lane == 0) {
    s_id[0] = kRootId;
    s_par[0] = kNoId;
    s_last[0] = -1;
    s_len[0] = 0;
    s_pb[0] = 0.0;
    s_pnb[0] = kNegInf;
    if constexpr (LM) {
      const uint64_t root = ngram::ng_push(0ull, la.bos);
      s_ctx[0] = root;
      s_lm[0] = 0.0;
      s_chain[0] = ngram::ng_chain(la.tab, la.mask, la.max_probe, root,
                                   ngram::ng_ctx_len(root, la.order), nullptr);
    }
    if constexpr (BIAS) {
      s_bst[0] = 0;
      s_bkept[0] = 0.0;
      s_bias[0] = bias::bs_bias(ba.bt, 0, 0.0);
    }
  }
  int n = 1;
  double best = 0.0;  // the best total after the last frame; 0 for L == 0
  const int64_t row0 = (int64_t)b * T;
  // frame t's candidates travel in registers while frame t-1 is worked on
  double c_lp = 0.0, c_lpb = 0.0;
  int c_tok = -1;
  if (L > 0) {
    if (lane < K) {
      c_lp = lp[row0 * K1 + lane];
      c_tok = tok[row0 * K + lane];
    }
    c_lpb = lp[row0 * K1 + K];
  }
  __syncthreads();  // the table's empty marks have landed before the first compare-and-swap

  for (int t = 0; t < L; ++t) {
    if (lane < K) {
      s_lp[lane] = c_lp;
      s_tok[lane] = c_tok;
    }
    const double lpb = c_lpb;
    if (t + 1 < L) {
      const int64_t row = row0 + t + 1;
      if (lane < K) {
        c_lp = lp[row * K1 + lane];
        c_tok = tok[row * K + lane];
      }
      c_lpb = lp[row * K1 + K];
    }
    if (lane < n) s_tot[lane] = lse2(s_pb[lane], s_pnb[lane]);
    __syncthreads();

    // extension items
    if (lane < K) {
      const int c = s_tok[lane];
      const double l = s_lp[lane];
      for (int i = 0; i < n; ++i)
        s_val[i * K1 + 1 + lane] = (c >= 0 && c != s_last[i]) ? s_tot[i] + l : kNaN;
    }
    if constexpr (LM) {
      // the LM value of every live extension item, the items spread over the lanes
      const int next = n * K;
      for (int q = lane; q < next; q += 64) {
        const int i = q / K;
        const int j = q - i * K;
        const int c = s_tok[j];
        if (c >= 0 && c != s_last[i])
          s_lmv[i * K1 + 1 + j] =
              s_lm[i] + ngram::ng_score(la.tab, la.mask, la.max_probe, la.order, la.V, la.unk,
                                        s_ctx[i], s_chain[i], c, nullptr);
      }
    }
    if constexpr (BIAS) {
      // bias(y . c) of every live extension item, the items spread over the lanes
      const int next = n * K;
      for (int q = lane; q < next; q += 64) {
        const int i = q / K;
        const int j = q - i * K;
        const int c = s_tok[j];
        if (c >= 0 && c != s_last[i]) {
          double kk = s_bkept[i];
          const int st = bias::bs_step(ba.bt, s_bst[i], c, kk);
          s_bv[i * K1 + 1 + j] = bias::bs_bias(ba.bt, st, kk);
        }
      }
    }
    __syncthreads();

    // stay items; the one extension that equals live entry m folds into it
    if (lane < n) {
      const int m = lane;
      const double pb_new = s_tot[m] + lpb;
      double pnb_new = kNegInf;
      int slot = m * K1;
      const int last = s_last[m];
      int jm = -1;
      for (int j = 0; j < K; ++j)
        if (last >= 0 && s_tok[j] == last) jm = j;
      if (jm >= 0) {
        pnb_new = s_pb[m] + s_lp[jm];
        const int par = s_par[m];
        int im = -1;
        for (int i = 0; i < n; ++i)
          if (s_id[i] == par) im = i;
        if (im >= 0) {
          const int e = im * K1 + 1 + jm;
          const double add = s_val[e];
          if (add == add) {
            pnb_new = lse2(pnb_new, add);
            s_val[e] = kNaN;
            if (e < slot) {  // inserted by entry im's turn, before m's own
              s_val[slot] = kNaN;
              slot = e;
            }
          }
        }
      }
      s_val[slot] = lse2(pb_new, pnb_new);
      s_slot[m] = slot;
      s_npb[m] = pb_new;
      s_npnb[m] = pnb_new;
      if constexpr (LM)
        if (slot != m * K1) s_lmv[slot] = s_lm[m];  // one LM value per tuple: the live entry's
      if constexpr (BIAS)
        if (slot != m * K1) s_bv[slot] = s_bias[m];  // and one bias value
    }
    __syncthreads();

    const int nitems = n * K1;
    if constexpr (LM && !BIAS) {
      // every live item's CTC value becomes its pruning key
      for (int e = lane; e < nitems; e += 64) {
        const double v = s_val[e];
        if (v == v) {
          const int i = e / K1;
          const bool ext = e != i * K1;
          s_val[e] = lm_key(v, la.lw, ext ? s_lmv[e] : s_lm[i], la.bonus, s_len[i] + (ext ? 1 : 0));
        }
      }
      __syncthreads();
    }
    if constexpr (BIAS) {
      // the same key (lm(y) = 0 without LM) plus the bias term
      for (int e = lane; e < nitems; e += 64) {
        const double v = s_val[e];
        if (v == v) {
          const int i = e / K1;
          const bool ext = e != i * K1;
          double lmv = 0.0;
          if constexpr (LM) lmv = ext ? s_lmv[e] : s_lm[i];
          const double key = lm_key(v, la.lw, lmv, la.bonus, s_len[i] + (ext ? 1 : 0));
          s_val[e] = bias_key(key, ba.bw, ext ? s_bv[e] : s_bias[i]);
        }
      }
      __syncthreads();
    }

    // the beam best items, in order: (total descending, item index ascending)
    double pv = 0.0, my_v = 0.0;
    int pe = -1, my_e = -1, n_new = 0;
    for (int r = 0; r < beam; ++r) {
      double bv = 0.0;
      int be = -1;
      for (int e = lane; e < nitems; e += 64) {
        const double v = s_val[e];
        const bool after = v == v && (r == 0 || v < pv || (v == pv && e > pe));
        if (after && (be < 0 || v > bv)) {
          bv = v;
          be = e;
        }
      }
#pragma unroll
      for (int o = 32; o > 0; o >>= 1) {
        const double ov = __shfl_xor(bv, o);
        const int oe = __shfl_xor(be, o);
        if (oe >= 0 && (be < 0 || ov > bv || (ov == bv && oe < be))) {
          bv = ov;
          be = oe;
        }
      }
      if (be < 0) break;  // the same in every lane
      if (lane == r) {
        my_v = bv;
        my_e = be;
      }
      pv = bv;
      pe = be;
      ++n_new;
    }

    int nid = kNoId, npar = kNoId, nlast = -1, nlen = 0;
    double npb = kNegInf, npnb = kNegInf;
    [[maybe_unused]] uint64_t nctx = 0ull;
    [[maybe_unused]] double nlm = 0.0;
    [[maybe_unused]] ngram::Chain nch;
    [[maybe_unused]] int nbst = 0;
    [[maybe_unused]] double nbkept = 0.0, nbias = 0.0;
    if (lane < n_new) {
      const int i = my_e / K1;
      const int pos = my_e - i * K1;
      int m = -1;
      for (int q = 0; q < n; ++q)
        if (s_slot[q] == my_e) m = q;
      if (m >= 0) {
        nid = s_id[m];
        npar = s_par[m];
        nlast = s_last[m];
        nlen = s_len[m];
        npb = s_npb[m];
        npnb = s_npnb[m];
        if constexpr (LM) {
          nctx = s_ctx[m];
          nlm = s_lm[m];
          nch = s_chain[m];
        }
        if constexpr (BIAS) {
          nbst = s_bst[m];
          nbkept = s_bkept[m];
          nbias = s_bias[m];
        }
      } else {
        const int c = s_tok[pos > 0 ? pos - 1 : 0];  // pos == 0 is always some entry's stay item
        npar = s_id[i];
        nlast = c;
        nlen = s_len[i] + 1;
        if constexpr (KEYED)
          npnb = s_tot[i] + s_lp[pos > 0 ? pos - 1 : 0];  // the item's CTC value; my_v is its key
        else
          npnb = my_v;
        if constexpr (BIAS) {  // the parent's pair, stepped again
          nbkept = s_bkept[i];
          nbst = bias::bs_step(ba.bt, s_bst[i], c, nbkept);
          nbias = s_bv[my_e];
        }
        if constexpr (LM) {
          nctx = ngram::ng_push(s_ctx[i], c);
          nlm = s_lmv[my_e];
          nch = ngram::ng_chain(la.tab, la.mask, la.max_probe, nctx,
                                ngram::ng_ctx_len(nctx, la.order), nullptr);
        }
        const unsigned long long key = ((unsigned long long)(unsigned)npar << 32) | (unsigned)c;
        const unsigned h = (unsigned)((key * 0x9E3779B97F4A7C15ull) >> shift);
        for (unsigned p = 0; p < tsize; ++p) {
          const unsigned sl = (h + p) & (tsize - 1);
          const unsigned long long old = atomicCAS(&tab[sl], kEmptySlot, key);
          if (old == kEmptySlot || old == key) {
            nid = (int)sl;
            break;
          }
        }
      }
    }
    __syncthreads();
    if (lane < n_new) {
      s_id[lane] = nid;
      s_par[lane] = npar;
      s_last[lane] = nlast;
      s_len[lane] = nlen;
      s_pb[lane] = npb;
      s_pnb[lane] = npnb;
      if constexpr (LM) {
        s_ctx[lane] = nctx;
        s_lm[lane] = nlm;
        s_chain[lane] = nch;
      }
      if constexpr (BIAS) {
        s_bst[lane] = nbst;
        s_bkept[lane] = nbkept;
        s_bias[lane] = nbias;
      }
    }
    n = n_new;
    if (lane == 0) best = my_v;
    __syncthreads();
  }

  if constexpr (KEYED) {
    // lane e closes entry e with the eos score and its total; the entries are then ranked by
    // (total descending, beam position ascending; a NaN total, outside the contract, after
    // every number) -- a permutation of 0..n-1, so every output position has one writer -- and
    // the entry of rank r < nbest is written to position r; positions n..nbest-1 are absent
    const int64_t hb = (int64_t)b * nbest;
    const bool live = lane < n;
    double ctc = kNegInf, lmf = kNegInf, tot = kNegInf;
    [[maybe_unused]] double bfin = kNegInf;
    if (live) {
      ctc = lse2(s_pb[lane], s_pnb[lane]);
      if constexpr (LM)
        lmf = s_lm[lane] + ngram::ng_score(la.tab, la.mask, la.max_probe, la.order, la.V, la.unk,
                                           s_ctx[lane], s_chain[lane], la.eos, nullptr);
      else
        lmf = 0.0;
      tot = lm_key(ctc, la.lw, lmf, la.bonus, s_len[lane]);
      if constexpr (BIAS) {
        bfin = bias::bs_bias_fin(ba.bt, s_bst[lane], s_bkept[lane]);
        tot = bias_key(tot, ba.bw, bfin);
      }
      s_tot[lane] = tot;
    }
    __syncthreads();
    int pos = lane;  // an absent position is its own
    if (live) {
      pos = 0;
      const bool mn = tot != tot;
      for (int q = 0; q < n; ++q) {
        const double tq = s_tot[q];
        const bool qn = tq != tq;
        const bool before = mn ? (!qn || q < lane) : (!qn && (tq > tot || (tq == tot && q < lane)));
        if (q != lane && before) ++pos;
      }
    }
    if (pos < nbest) {
      int len = live ? s_len[lane] : 0;
      len = len > T ? T : len;
      walk_prefix(tab, tsize, live ? s_id[lane] : kNoId, len, hyp + (hb + pos) * T);
      hyp_len[hb + pos] = len;
      la.ctc[hb + pos] = ctc;
      la.lm[hb + pos] = lmf;
      la.total[hb + pos] = tot;
      if constexpr (BIAS) ba.out[hb + pos] = bfin;
      s_slot[pos] = len;
    }
    if (lane == 0) n_hyp[b] = n < nbest ? n : nbest;
    __syncthreads();
    for (int e = 0; e < nbest; ++e) {
      int* dst = hyp + (hb + e) * T;
      for (int t = s_slot[e] + lane; t < T; t += 64) dst[t] = -1;
    }
    return;
  }
  if constexpr (NBEST) {
    // lane e walks entry e's parents (each walk bounded by its length <= T): tokens into
    // hyp[b][e][0..len), -1 after them; entries past the live ones are empty with score -inf
    const int64_t hb = (int64_t)b * nbest;
    if (lane < nbest) {
      const bool live = lane < n;
      int len = live ? s_len[lane] : 0;
      len = len > T ? T : len;
      walk_prefix(tab, tsize, live ? s_id[lane] : kNoId, len, hyp + (hb + lane) * T);
      hyp_len[hb + lane] = len;
      // entry 0: the value the 1-best path reports
      nscore[hb + lane] = !live ? kNegInf : lane == 0 ? best : lse2(s_pb[lane], s_pnb[lane]);
    }
    if (lane == 0) n_hyp[b] = n < nbest ? n : nbest;
    for (int e = 0; e < nbest; ++e) {
      int len = e < n ? s_len[e] : 0;
      len = len > T ? T : len;
      int* dst = hyp + (hb + e) * T;
      for (int t = len + lane; t < T; t += 64) dst[t] = -1;
    }
    return;
  }
  // walk the best entry's parents: tokens into out[b][0..cnt), -1 after them
  int cnt = n > 0 ? s_len[0] : 0;
  cnt = cnt > T ? T : cnt;
  int* dst = out + row0;
  if (lane == 0) {
    walk_prefix(tab, tsize, n > 0 ? s_id[0] : kNoId, cnt, dst);
    out_len[b] = cnt;
    if (score) score[b] = best;
  }
  for (int t = cnt + lane; t < T; t += 64) dst[t] = -1;
}

}  // namespace

// workspace: [rows][K+1] fp64 lp | [rows][K] int32 tokens (padded to 8 bytes) | B prefix tables
static inline unsigned __int128 beam_tok_bytes(unsigned __int128 rows, int64_t K) {
  return (rows * (unsigned)K * 4 + 7) / 8 * 8;
}

size_t ctc_beam_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k) {
  const int64_t K = V < top_k ? V : top_k;
  const unsigned __int128 rows = (unsigned __int128)B * (unsigned __int128)T;
  const unsigned __int128 bytes = rows * (unsigned)(K + 1) * 8 + beam_tok_bytes(rows, K) +
                                  (unsigned __int128)B * beam_table_slots(T, beam) * 8;
  return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : (size_t)bytes;
}

void launch_ctc_beam(const float* logits, const int64_t* lens, int64_t B, int64_t T, int64_t V,
                     int blank, int beam, int top_k, int stages, void* ws, int* hyp, int* hyp_len,
                     int* n_hyp, double* score, int nbest, const CtcBeamLm* lm, hipStream_t s,
                     const CtcBeamBias* bias) {
  if (B == 0) return;
  const int K = (int)(V < top_k ? V : top_k);
  const int64_t rows = B * T;
  const int64_t slots = beam_table_slots(T, beam);
  double* lp = static_cast<double*>(ws);
  int* tok = reinterpret_cast<int*>(lp + rows * (K + 1));
  unsigned long long* table = reinterpret_cast<unsigned long long*>(
      reinterpret_cast<char*>(tok) + (size_t)beam_tok_bytes((unsigned __int128)rows, K));
  if ((stages & 1) && T > 0)
    hipLaunchKernelGGL(beam_frame_kernel, dim3((unsigned)ceil_div(rows, kFrameWaves)),
                       dim3(64 * kFrameWaves), 0, s, logits, lens, rows, (int)T, (int)V, blank, K,
                       lp, tok);
  if (!(stages & 2)) return;
  const dim3 grid((unsigned)B), block(64);
  if (nbest == 0) {  // the 1-best form: hyp / hyp_len are the kernel's out / out_len
    hipLaunchKernelGGL(beam_search_kernel<false>, grid, block, 0, s, lp, tok, lens, (int)T, K, beam,
                       table, slots, hyp, hyp_len, score, 0, nullptr, nullptr, nullptr, nullptr,
                       BeamLm{}, BeamNoBias{});
    return;
  }
  BeamLm la{};
  if (lm)
    la = BeamLm{static_cast<const ngram::Entry*>(lm->table), (uint64_t)lm->slots - 1,
                lm->max_probe, lm->order, (int)V, lm->bos, lm->eos, lm->unk_logp, lm->lm_weight,
                lm->ins_bonus, lm->ctc, lm->lm, lm->total};
  if (bias) {  // (with lm; a null table is the search without an LM)
    const BeamBias ba{bias::Tables{static_cast<const bias::Node*>(bias->nodes),
                                   static_cast<const bias::Edge*>(bias->edges),
                                   (uint64_t)bias->slots - 1, bias->max_probe, (int)bias->n_nodes},
                      bias->bias_weight, bias->bias};
    const auto kernel =
        lm->table ? beam_search_kernel<true, true, true> : beam_search_kernel<true, false, true>;
    hipLaunchKernelGGL(kernel, grid, block, 0, s, lp, tok, lens, (int)T, K, beam, table, slots,
                       nullptr, nullptr, nullptr, nbest, hyp, hyp_len, n_hyp, score, la, ba);
    return;
  }
  const auto kernel = !lm ? beam_search_kernel<true> : beam_search_kernel<true, true>;
  hipLaunchKernelGGL(kernel, grid, block, 0, s, lp, tok, lens, (int)T, K, beam, table, slots,
                     nullptr, nullptr, nullptr, nbest, hyp, hyp_len, n_hyp, score, la,
                     BeamNoBias{});
}

}  // namespace ob
