// ob_ngram.h — the back-off n-gram language model of the shallow fusion: the table layout, the
// one probe routine and the scoring rule, shared by the kernels of ngram.hip, the host table
// builder and the host scorer (ob_ngram_score_host), so that a CPU test runs the real table.
//
// Table: one open-addressed hash table of `slots` (a power of two, >= 2 x the entry count)
// 16-byte entries (key, logp, backoff). A key packs the n-gram (w_1 .. w_n), 1 <= n <= 4, as four
// 16-bit fields of (id + 1), w_n in field 0 (bits 0..15), w_{n-1} in field 1, ...; unused fields
// are 0, so the number of non-zero fields is the n-gram's order, ids are 0..65534, and key 0 is
// the empty slot. Home slot = ng_mix(key) & (slots - 1), linear probing. The builder places every
// entry within max_probe slots of its home, so a lookup ends at the key, at an empty slot or
// after max_probe slots, whichever comes first: a miss never probes further than a hit can.
//
// A row's context state is the same packing of the last three ids of its prefix [bos] + tokens
// (the newest id in field 0): the key of (h[-m:], w) is ((ctx & mask(m)) << 16) | (w + 1) and the
// key of the context h[-m:] itself is ctx & mask(m), no id is unpacked.
//
// Scoring rule (the contract of ob_ngram_step / ob_ngram_seq_logprob / ob_ngram_score_host): with
// h the last min(order - 1, len(prefix)) ids of the prefix [bos] + tokens and candidate w,
//     acc = 0 (fp64)
//     for m = len(h) .. 0:
//         if (h[-m:], w) is an entry:         return acc + logp
//         if m >= 1 and h[-m:] is an entry:   acc += backoff
//     return acc + unk_logp                   (w has no unigram)
// Table values are float32, the sum is float64 in this order: the result is a function of (h, w)
// alone, the same bits on the host, on the device and in every slot. eos is scored as </s> (the
// entry of its id). A candidate id < 0 is an absent candidate and scores -inf, as
// ob_ctc_prefix_step writes -inf for c == -1; an id >= V (or > 65534) has no entry at any order
// and scores the full back-off chain + unk_logp.
#ifndef OB_NGRAM_H_
#define OB_NGRAM_H_

#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define OB_NG_HD __host__ __device__ __forceinline__
#else
#define OB_NG_HD inline
#endif

namespace ob {
namespace ngram {

constexpr int kMaxOrder = 4;
constexpr int kMaxId = 65534;        // (id + 1) fits 16 bits
constexpr int kProbeLimit = 64;      // the builder grows the table until max_probe <= this
constexpr uint64_t kCtxMask = 0xFFFFFFFFFFFFull;  // three fields

struct __attribute__((aligned(16))) Entry {
  uint64_t key;
  float logp, backoff;
};
static_assert(sizeof(Entry) == 16, "one 16-byte gather per probe");

// the fixed 64-bit mix that picks the home slot (the splitmix64 finaliser)
OB_NG_HD uint64_t ng_mix(uint64_t z) {
  z ^= z >> 30;
  z *= 0xbf58476d1ce4e5b9ull;
  z ^= z >> 27;
  z *= 0x94d049bb133111ebull;
  z ^= z >> 31;
  return z;
}

// the low m fields, m = 0..3
OB_NG_HD uint64_t ng_fields(int m) { return (1ull << (16 * m)) - 1ull; }

// the context after one more id (ids outside 0..65534 are clamped into it)
OB_NG_HD uint64_t ng_push(uint64_t ctx, int64_t id) {
  const uint64_t f = (uint64_t)(id < 0 ? 0 : (id > kMaxId ? kMaxId : id)) + 1ull;
  return ((ctx << 16) | f) & kCtxMask;
}

// len(h): the context's ids that an LM of this order uses
OB_NG_HD int ng_ctx_len(uint64_t ctx, int order) {
  int have = 0;  // the non-zero fields are contiguous from field 0
#pragma unroll
  for (int m = 0; m < 3; ++m) have += ((ctx >> (16 * m)) & 0xFFFFull) != 0 ? 1 : 0;
  return have < order - 1 ? have : order - 1;
}

// The probe routine, in two halves so that a caller can have the home-slot loads of several keys
// in flight before it looks at any of them: ng_home is the first gather, ng_resolve finishes the
// lookup from it. *probes (may be null) is advanced by the slots examined, the home slot included.
OB_NG_HD Entry ng_home(const Entry* tab, uint64_t mask, uint64_t key) {
  return tab[ng_mix(key) & mask];
}

OB_NG_HD bool ng_resolve(const Entry* tab, uint64_t mask, int max_probe, uint64_t key, Entry e,
                         float& logp, float& backoff, int* probes) {
  uint64_t s = ng_mix(key) & mask;
  int n = 1;
  bool hit = e.key == key;
  while (!hit && e.key != 0 && n < max_probe) {
    s = (s + 1) & mask;
    e = tab[s];
    ++n;
    hit = e.key == key;
  }
  if (probes) *probes += n;
  if (hit) {
    logp = e.logp;
    backoff = e.backoff;
  }
  return hit;
}

// the back-off chain of one context: has[m] / bo[m] for the context h[-m:], m = 1..3
struct Chain {
  bool has[kMaxOrder];
  float bo[kMaxOrder];
};

OB_NG_HD Chain ng_chain(const Entry* tab, uint64_t mask, int max_probe, uint64_t ctx, int hl,
                        int* probes) {
  Chain c;
  Entry e[kMaxOrder];
#pragma unroll
  for (int m = 1; m < kMaxOrder; ++m)
    if (m <= hl) e[m] = ng_home(tab, mask, ctx & ng_fields(m));
#pragma unroll
  for (int m = 1; m < kMaxOrder; ++m) {
    float lp = 0.0f, bo = 0.0f;
    c.has[m] = m <= hl &&
               ng_resolve(tab, mask, max_probe, ctx & ng_fields(m), e[m], lp, bo, probes);
    c.bo[m] = bo;
  }
  c.has[0] = false;
  c.bo[0] = 0.0f;
  return c;
}

// the candidate's entries (h[-m:], w) for m = 0..hl, all home slots loaded before any is examined
OB_NG_HD void ng_candidate(const Entry* tab, uint64_t mask, int max_probe, uint64_t ctx, int hl,
                           int w, bool hit[kMaxOrder], float lp[kMaxOrder], int* probes) {
  Entry e[kMaxOrder];
  const uint64_t wf = (uint64_t)w + 1ull;
#pragma unroll
  for (int m = 0; m < kMaxOrder; ++m)
    if (m <= hl) e[m] = ng_home(tab, mask, ((ctx & ng_fields(m)) << 16) | wf);
#pragma unroll
  for (int m = 0; m < kMaxOrder; ++m) {
    float bo = 0.0f;
    lp[m] = 0.0f;
    hit[m] = m <= hl && ng_resolve(tab, mask, max_probe, ((ctx & ng_fields(m)) << 16) | wf, e[m],
                                   lp[m], bo, probes);
  }
}

// the rule's sum, in its fixed order
OB_NG_HD double ng_combine(int hl, const bool hit[kMaxOrder], const float lp[kMaxOrder],
                           const Chain& c, double unk_logp) {
  double acc = 0.0;
#pragma unroll
  for (int m = kMaxOrder - 1; m >= 0; --m) {
    if (m > hl) continue;
    if (hit[m]) return acc + (double)lp[m];
    if (m >= 1 && c.has[m]) acc += (double)c.bo[m];
  }
  return acc + unk_logp;
}

// score of candidate w after context ctx, given the context's chain
OB_NG_HD double ng_score(const Entry* tab, uint64_t mask, int max_probe, int order, int V,
                         double unk_logp, uint64_t ctx, const Chain& c, int w, int* probes) {
  if (w < 0) return -(double)INFINITY;
  const int hl = ng_ctx_len(ctx, order);
  bool hit[kMaxOrder] = {false, false, false, false};
  float lp[kMaxOrder] = {0.0f, 0.0f, 0.0f, 0.0f};
  if (w < V && w <= kMaxId) ng_candidate(tab, mask, max_probe, ctx, hl, w, hit, lp, probes);
  return ng_combine(hl, hit, lp, c, unk_logp);
}

}  // namespace ngram
}  // namespace ob

#endif  // OB_NGRAM_H_
