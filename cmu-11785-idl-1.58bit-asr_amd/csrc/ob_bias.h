// ob_bias.h — phrase-list contextual biasing: the automaton's layout, the one edge lookup and the
// step rule, shared by the kernels of bias.hip, the beam search of beam.hip, the host builder and
// the host walker (ob_bias_walk_host), so that a CPU test runs the real tables.
//
// Automaton: the phrases (1..16 token ids in 0..65534, a float32 boost > 0 per token) form a trie.
// Node 0 is the root; the other nodes are numbered breadth-first by depth, within a depth by
// (parent number, token) ascending, so the same phrases in any order give the same bytes. With
// val(n, b) = float32 of the float64 product n * b, node p (a token path) carries
//     commit(p) = max val(len q, b_q) over phrases q that are a prefix of p (q == p included), or 0
//     phi(p)    = max of commit(p) and val(len p, b_q) over phrases q that p is a prefix of
//     fail(p)   = the longest proper suffix of p that is a node (the root if none)
//     flags     = bit 0: p has children
// in one 16-byte record {int32 fail, int32 flags, float phi, float commit}.
//
// Edges: one open-addressed hash table of `slots` (a power of two, >= 2 x the edge count) 16-byte
// entries {uint64 key, int32 child, int32 0}, key = ((node + 1) << 16) | (tok + 1), key 0 the empty
// slot. Home slot = ng_mix(key) & (slots - 1) (the splitmix64 finaliser of ob_ngram.h), linear
// probing; the builder inserts in key order into a zeroed table and places every edge within
// max_probe <= 64 slots of its home, so a lookup ends at the key, at an empty slot or after
// max_probe slots.
//
// Step rule (the contract of ob_bias_step / ob_bias_seq_score / ob_bias_walk_host and of the biased
// searches). A hypothesis y carries (state, kept), a node and a float64, (root, 0.0) for the empty
// y. Extending by token w:
//     u = state
//     loop:  if child(u, w) exists:  t = child(u, w); break
//            if commit(u) > 0:       kept += commit(u); t = child(root, w) or root; break
//            if u == root:           t = root; break
//            u = fail(u)
//     if t != root and not has_children(t):   kept += commit(t); t = root
//     state = t
// The loop makes at most 17 lookups (a fail link shortens the path). Matches are left to right and
// never overlap. bias(y) = kept + (double)phi(state), the running value with the partial match
// counted; bias_fin(y) = kept + (double)commit(state), the closed value with an unfinished partial
// match taken back. kept is a float64 sum of float32 values in a fixed order: a function of the
// token tuple alone, the same bits on the host, on the device and in every beam slot.
#ifndef OB_BIAS_H_
#define OB_BIAS_H_

#include <stdint.h>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>  // (ob_ngram.h's function qualifiers)
#endif

#include "ob_ngram.h"

namespace ob {
namespace bias {

constexpr int kMaxPhraseLen = 16;
constexpr int kMaxId = ngram::kMaxId;
constexpr int kProbeLimit = ngram::kProbeLimit;
constexpr int64_t kMaxNodes = (int64_t)1 << 30;

struct __attribute__((aligned(16))) Node {
  int32_t fail, flags;
  float phi, commit;
};
static_assert(sizeof(Node) == 16, "one 16-byte gather per node");

struct __attribute__((aligned(16))) Edge {
  uint64_t key;
  int32_t child, pad;
};
static_assert(sizeof(Edge) == 16, "one 16-byte gather per probe");

// the tables of one phrase list, as every scorer takes them
struct Tables {
  const Node* nodes;
  const Edge* edges;
  uint64_t mask;  // slots - 1
  int max_probe;
  int n_nodes;
};

OB_NG_HD uint64_t bs_key(int node, int tok) {
  return ((uint64_t)(node + 1) << 16) | (uint64_t)(tok + 1);
}

// child(node, tok), -1 if there is none (a token outside 0..65534 has no edge)
OB_NG_HD int bs_child(const Tables& bt, int node, int tok) {
  if (tok < 0 || tok > kMaxId) return -1;
  const uint64_t key = bs_key(node, tok);
  uint64_t s = ngram::ng_mix(key) & bt.mask;
  Edge e = bt.edges[s];
  int n = 1;
  while (e.key != key && e.key != 0 && n < bt.max_probe) {
    s = (s + 1) & bt.mask;
    e = bt.edges[s];
    ++n;
  }
  if (e.key != key) return -1;
  // (a table that is not the builder's cannot index outside the nodes)
  return e.child > 0 && e.child < bt.n_nodes ? e.child : -1;
}

OB_NG_HD int bs_state(const Tables& bt, int state) {
  return state >= 0 && state < bt.n_nodes ? state : 0;
}

// the step rule: (state, kept) of y -> those of y . w
OB_NG_HD int bs_step(const Tables& bt, int state, int w, double& kept) {
  int u = bs_state(bt, state);
  int t = 0;
  for (int it = 0; it <= kMaxPhraseLen; ++it) {
    const int c = bs_child(bt, u, w);
    if (c >= 0) {
      t = c;
      break;
    }
    const Node nu = bt.nodes[u];
    if (nu.commit > 0.0f) {
      kept += (double)nu.commit;
      const int r = bs_child(bt, 0, w);
      t = r >= 0 ? r : 0;
      break;
    }
    if (u == 0) break;
    u = bs_state(bt, nu.fail);
  }
  if (t != 0) {
    const Node nt = bt.nodes[t];
    if (!(nt.flags & 1)) {
      kept += (double)nt.commit;
      t = 0;
    }
  }
  return t;
}

OB_NG_HD double bs_bias(const Tables& bt, int state, double kept) {
  return kept + (double)bt.nodes[bs_state(bt, state)].phi;
}

OB_NG_HD double bs_bias_fin(const Tables& bt, int state, double kept) {
  return kept + (double)bt.nodes[bs_state(bt, state)].commit;
}

}  // namespace bias
}  // namespace ob

#endif  // OB_BIAS_H_
