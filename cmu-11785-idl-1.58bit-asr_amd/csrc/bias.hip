// bias.hip — phrase-list contextual biasing (layout, lookup and step rule: ob_bias.h): the host
// automaton builder and host walker, and the two device scorers.
//
//   builder     host C. The trie is built level by level: at depth d the (parent number, token)
//               pairs of every phrase longer than d are sorted and numbered, which is the
//               breadth-first numbering of the contract whatever the phrases' order. commit comes
//               down from the parent, the largest boost of a subtree comes up from the children
//               (val(n, b) is monotone in b, so phi needs only that maximum), fail is the
//               Aho-Corasick link. The edges are already in key order; they go into a zeroed table
//               that starts at the smallest power of two >= 2 x the edge count and doubles until
//               every edge sits within 64 slots of its home.
//   step        per search step, one launch: two rows per wave, a row on 32 lanes. Every lane of a
//               row rebuilds the row's (state, kept) from its parent's stored pair and its own last
//               token (the same addresses in all 32 lanes: one broadcast load each), lane 0 stores
//               it; lanes 0..K-1 then extend it by one candidate each and write the running value,
//               or the closed value for eos.
//   seq score   a thread per hypothesis row walks its tokens in order.
//
// No atomics, every word one writer, every loop bounded by max_probe, the phrase length, K or T;
// kept is added in the rule's order: bitwise reproducible, whichever slot holds a prefix.
#include <math.h>

#include <algorithm>
#include <numeric>
#include <vector>

#include "ob_bias.h"
#include "ob_launch.h"

namespace ob {

using namespace bias;

namespace {

constexpr int kBsRowLanes = 32;  // lanes per row of the step kernel (K <= 32)

__global__ __launch_bounds__(64) void bias_step_kernel(
    Tables bt, const int* __restrict__ topi, const int64_t* __restrict__ tok,
    const int* __restrict__ len, const int* __restrict__ link, const uint8_t* __restrict__ skip,
    int64_t R, int K, int eos, const int* __restrict__ st_in, int* __restrict__ st_out,
    const double* __restrict__ kept_in, double* __restrict__ kept_out, double* __restrict__ bsc) {
  const int lane = threadIdx.x;
  const int sub = lane % kBsRowLanes;
  const int64_t row_raw = (int64_t)blockIdx.x * (64 / kBsRowLanes) + lane / kBsRowLanes;
  const int64_t row = row_raw < R ? row_raw : R - 1;
  if (row_raw >= R || skip[row] != 0) return;
  const int n = len[row];
  int state = 0;
  double kept = 0.0;
  if (n >= 1) {
    if (n > 1) {
      int par = link[2 * row];
      par = par < 0 ? 0 : (par >= R ? (int)(R - 1) : par);
      state = st_in[par];
      kept = kept_in[par];
    }
    const int64_t tk = tok[row];
    state = bs_step(bt, state, tk < 0 || tk > kMaxId ? -1 : (int)tk, kept);
  }
  if (sub == 0) {
    st_out[row] = state;
    kept_out[row] = kept;
  }
  if (sub >= K) return;
  const int c = topi[row * K + sub];
  double v;
  if (c < 0) {
    v = -(double)INFINITY;
  } else if (c == eos) {
    v = bs_bias_fin(bt, state, kept);
  } else {
    double kk = kept;
    const int t = bs_step(bt, state, c, kk);
    v = bs_bias(bt, t, kk);
  }
  bsc[row * K + sub] = v;
}

__global__ __launch_bounds__(64) void bias_seq_score_kernel(Tables bt, const int* __restrict__ hyp,
                                                            const int* __restrict__ hyp_len,
                                                            int64_t R, int T,
                                                            double* __restrict__ out) {
  const int64_t row = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (row >= R) return;
  const int L = hyp_len[row];
  if (L < 0) {  // an absent row
    out[row] = -(double)INFINITY;
    return;
  }
  const int n = L > T ? T : L;
  const int* y = hyp + row * (int64_t)T;
  int state = 0;
  double kept = 0.0;
  for (int j = 0; j < n; ++j) state = bs_step(bt, state, y[j], kept);
  out[row] = bs_bias_fin(bt, state, kept);
}

inline float bias_val(int n, float b) { return (float)((double)n * (double)b); }

inline int64_t bias_min_slots(int64_t n_edges) {
  int64_t s = 8;
  while (s < 2 * n_edges) s <<= 1;
  return s;
}

}  // namespace

bool bias_supported(int64_t V, int64_t K, int64_t n_nodes) {
  return V >= 1 && V <= kMaxId + 1 && K >= 1 && K <= kBsRowLanes && n_nodes >= 1 &&
         n_nodes <= kMaxNodes;
}

bool bias_sizes(int64_t n_phrases, int64_t total_tokens, int64_t* max_nodes, int64_t* min_slots) {
  if (n_phrases < 0 || total_tokens < n_phrases || total_tokens > n_phrases * kMaxPhraseLen ||
      total_tokens + 1 > kMaxNodes)
    return false;
  *max_nodes = total_tokens + 1;
  *min_slots = bias_min_slots(total_tokens);
  return true;
}

// -> 0 ok; 1 a phrase is empty or too long, an id out of range, a boost not finite or not
// positive; 2 a buffer is too small (*n_nodes / *slots say what is needed)
int bias_build(const int* tokens, const int* lengths, const float* boosts, int64_t P, void* nodes,
               size_t nodes_bytes, void* edges, size_t edges_bytes, int64_t* n_nodes,
               int64_t* slots, int* max_probe) {
  std::vector<int64_t> off((size_t)P + 1, 0);
  for (int64_t p = 0; p < P; ++p) {
    const int n = lengths[p];
    if (n < 1 || n > kMaxPhraseLen) return 1;
    const float b = boosts[p];
    if (!(b > 0.0f) || !(b <= 3.4028234663852886e38f)) return 1;
    off[(size_t)p + 1] = off[(size_t)p] + n;
  }
  for (int64_t i = 0; i < off[(size_t)P]; ++i)
    if (tokens[i] < 0 || tokens[i] > kMaxId) return 1;

  // the trie, level by level
  struct Item {
    int par, tok;
    int64_t p;
  };
  std::vector<int> cur((size_t)P, 0), parent(1, -1), ptok(1, -1), depth(1, 0);
  std::vector<float> endv(1, 0.0f), subb(1, 0.0f);
  std::vector<Item> items;
  for (int d = 0; d < kMaxPhraseLen; ++d) {
    items.clear();
    for (int64_t p = 0; p < P; ++p)
      if (lengths[p] > d) items.push_back(Item{cur[(size_t)p], tokens[off[(size_t)p] + d], p});
    if (items.empty()) break;
    std::sort(items.begin(), items.end(), [](const Item& a, const Item& b) {
      return a.par != b.par ? a.par < b.par : (a.tok != b.tok ? a.tok < b.tok : a.p < b.p);
    });
    for (size_t i = 0; i < items.size(); ++i) {
      const Item& it = items[i];
      if (i == 0 || it.par != items[i - 1].par || it.tok != items[i - 1].tok) {
        parent.push_back(it.par);
        ptok.push_back(it.tok);
        depth.push_back(d + 1);
        endv.push_back(0.0f);
        subb.push_back(0.0f);
      }
      const int id = (int)parent.size() - 1;
      cur[(size_t)it.p] = id;
      subb[(size_t)id] = std::max(subb[(size_t)id], boosts[it.p]);
      if (lengths[it.p] == d + 1)  // the same phrase twice keeps the larger boost
        endv[(size_t)id] = std::max(endv[(size_t)id], bias_val(d + 1, boosts[it.p]));
    }
  }
  const int64_t M = (int64_t)parent.size();
  for (int64_t v = M - 1; v >= 1; --v)  // children are numbered after their parents
    subb[(size_t)parent[(size_t)v]] = std::max(subb[(size_t)parent[(size_t)v]], subb[(size_t)v]);

  // the edges (node v's, for v = 1..M-1) are in key order as numbered
  const int64_t E = M - 1;
  std::vector<uint64_t> keys((size_t)E);
  for (int64_t v = 1; v < M; ++v) keys[(size_t)v - 1] = bs_key(parent[(size_t)v], ptok[(size_t)v]);
  auto child = [&](int u, int w) -> int {
    const uint64_t k = bs_key(u, w);
    const auto it = std::lower_bound(keys.begin(), keys.end(), k);
    return it != keys.end() && *it == k ? (int)(it - keys.begin()) + 1 : -1;
  };
  std::vector<Node> nd((size_t)M);
  nd[0] = Node{0, 0, 0.0f, 0.0f};
  for (int64_t v = 1; v < M; ++v) {
    const int par = parent[(size_t)v], w = ptok[(size_t)v];
    nd[(size_t)par].flags |= 1;
    int f = 0;
    if (par != 0) {
      int u = nd[(size_t)par].fail;
      for (;;) {
        const int c = child(u, w);
        if (c >= 0) {
          f = c;
          break;
        }
        if (u == 0) break;
        u = nd[(size_t)u].fail;
      }
    }
    const float commit = std::max(nd[(size_t)par].commit, endv[(size_t)v]);
    const float phi = std::max(commit, bias_val(depth[(size_t)v], subb[(size_t)v]));
    nd[(size_t)v] = Node{f, 0, phi, commit};
  }

  int64_t s = bias_min_slots(E);
  std::vector<Edge> tab;
  int worst = 1;
  for (;; s <<= 1) {
    tab.assign((size_t)s, Edge{0ull, 0, 0});
    const uint64_t mask = (uint64_t)s - 1;
    worst = 1;
    for (int64_t e = 0; e < E; ++e) {
      uint64_t p = ngram::ng_mix(keys[(size_t)e]) & mask;
      int run = 1;
      while (tab[p].key != 0) {
        p = (p + 1) & mask;
        ++run;
      }
      tab[p] = Edge{keys[(size_t)e], (int)e + 1, 0};
      worst = std::max(worst, run);
    }
    if (worst <= kProbeLimit) break;
  }
  *n_nodes = M;
  *slots = s;
  *max_probe = worst;
  if (!nodes || nodes_bytes < (size_t)M * sizeof(Node) || !edges ||
      edges_bytes < (size_t)s * sizeof(Edge))
    return 2;
  std::copy(nd.begin(), nd.end(), static_cast<Node*>(nodes));
  std::copy(tab.begin(), tab.end(), static_cast<Edge*>(edges));
  return 0;
}

static Tables bias_tables(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                          int max_probe) {
  return Tables{static_cast<const Node*>(nodes), static_cast<const Edge*>(edges),
                (uint64_t)slots - 1, max_probe, (int)n_nodes};
}

void bias_walk_host(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                    int max_probe, const int* tokens, const int* lens, int64_t Q, int64_t T,
                    int* state, double* kept, double* bias, double* bias_fin) {
  const Tables bt = bias_tables(nodes, n_nodes, edges, slots, max_probe);
  for (int64_t q = 0; q < Q; ++q) {
    int64_t n = lens[q];
    n = n < 0 ? 0 : (n > T ? T : n);
    int st = 0;
    double kp = 0.0;
    for (int64_t j = 0; j < n; ++j) st = bs_step(bt, st, tokens[q * T + j], kp);
    state[q] = st;
    kept[q] = kp;
    bias[q] = bs_bias(bt, st, kp);
    bias_fin[q] = bs_bias_fin(bt, st, kp);
  }
}

void launch_bias_step(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                      int max_probe, const int* topi, const int64_t* tok, const int* len,
                      const int* link, const uint8_t* skip, int64_t B, int64_t N, int64_t K,
                      int eos, const int* st_in, int* st_out, const double* kept_in,
                      double* kept_out, double* bsc, hipStream_t s) {
  const int64_t R = B * N;
  if (R == 0) return;
  constexpr int kRpw = 64 / kBsRowLanes;
  hipLaunchKernelGGL(bias_step_kernel, dim3((unsigned)ceil_div(R, kRpw)), dim3(64), 0, s,
                     bias_tables(nodes, n_nodes, edges, slots, max_probe), topi, tok, len, link,
                     skip, R, (int)K, eos, st_in, st_out, kept_in, kept_out, bsc);
}

void launch_bias_seq_score(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                           int max_probe, const int* hyp, const int* hyp_len, int64_t R, int64_t T,
                           double* out, hipStream_t s) {
  if (R == 0) return;
  hipLaunchKernelGGL(bias_seq_score_kernel, dim3((unsigned)ceil_div(R, (int64_t)64)), dim3(64), 0,
                     s, bias_tables(nodes, n_nodes, edges, slots, max_probe), hyp, hyp_len, R,
                     (int)T, out);
}

}  // namespace ob
