// attdec.hip — autoregressive beam search with the attention decoder, KV-cached, at static
// shapes and without host synchronisation (decoder="attention").
//
//   step attention   one query (position t) per (row, head) over positions 0..t of the row's
//                    own ancestry. K/V of position j live in cache [L][R][2e] (k | v) at the
//                    slot that produced them; anc [R][L] names that slot. The kernel appends
//                    the row's K/V at (t, r) and reads (j, anc[r][j]) for j < t: a beam reorder
//                    rewrites anc only, K/V never move.
//   output layer     per hidden row the float64 log-sum-exp over all V and the K largest
//                    logits among the non-banned ids, without the [R][V] logits: the GEMM tile
//                    of ob_scorer.h (exact fp32 products) leaves per (row, 64-column tile) a
//                    (max, sum of exp) pair and the tile's K best (value, column) in order; the
//                    merge kernel (one wave per row) joins the tiles in index order. No
//                    atomics, every word one writer, every sum a fixed order.
//   beam step        per utterance the N x K row candidates and the carried finished slots,
//                    key = score / norm[n], the N largest (ties: smaller slot, then smaller
//                    token); writes the next input tokens, scores, lengths, flags, the trace
//                    and the new anc rows. init / finalize set the state up and walk the trace
//                    back into the n-best layout. Bookkeeping in float64 and integers.
//
// Step-attention arithmetic follows decattn.hip's forward: fp32 fma chains (four per dot
// product, two per context column), scores scaled by 1/sqrt(dh), softmax = exp(s - max) / sum
// with IEEE exp and division. Its order depends on the position j alone, never on the slot, so
// a permuted slot assignment gives the same bits.
#include <math.h>

#include <algorithm>
#include <type_traits>

#include "ob_launch.h"
#include "ob_scorer.h"

namespace ob {

namespace {

using namespace scorer;

constexpr int kAdMaxPos = 256;   // positions per row of the step attention (L + 1 <= 256)
constexpr int kAdMaxN = 32;      // beam slots per utterance; also the top-k limit
constexpr int kAdMaxCand = kAdMaxN * kAdMaxN + kAdMaxN;

// ------------------------------------------------------------------------------------------
// cached single-query self-attention: block = (row r, head h), one wave
// ------------------------------------------------------------------------------------------
template <int DH>
__global__ __launch_bounds__(64) void decattn_step_kernel(
    const float* __restrict__ qkv, int64_t sq, float* __restrict__ cache,
    const int* __restrict__ anc, const uint8_t* __restrict__ skip, int R, int H, int L, int t,
    float scale, float* __restrict__ ctx) {
  __shared__ __attribute__((aligned(16))) float qs[DH];
  __shared__ float ps[kAdMaxPos];
  __shared__ int as[kAdMaxPos];
  const int r = (int)blockIdx.x / H, h = (int)blockIdx.x - r * H;
  if (skip && skip[r]) return;
  const int lane = threadIdx.x;
  const int e = H * DH;
  const int64_t prow = 2 * (int64_t)e;  // floats per cache row (k | v)
  const float* row = qkv + (int64_t)r * sq;
  if (lane < DH) {
    float* own = cache + ((int64_t)t * R + r) * prow + h * DH;
    own[lane] = row[e + h * DH + lane];
    own[e + lane] = row[2 * e + h * DH + lane];
    qs[lane] = row[h * DH + lane];
  }
  __syncthreads();
  const int n = t + 1;
  for (int j = lane; j < n; j += 64) {
    int a = r;
    if (j < t) {
      a = anc[(int64_t)r * L + j];
      a = a < 0 ? 0 : (a >= R ? R - 1 : a);  // (never leaves the cache, whatever anc holds)
    }
    as[j] = a;
    const float* kp = j == t ? row + e + h * DH : cache + ((int64_t)j * R + a) * prow + h * DH;
    float d0 = 0.f, d1 = 0.f, d2 = 0.f, d3 = 0.f;
#pragma unroll
    for (int c = 0; c < DH; c += 4) {
      const f32x4 k4 = *reinterpret_cast<const f32x4*>(kp + c);
      const f32x4 q4 = *reinterpret_cast<const f32x4*>(qs + c);
      d0 = fmaf(k4[0], q4[0], d0);
      d1 = fmaf(k4[1], q4[1], d1);
      d2 = fmaf(k4[2], q4[2], d2);
      d3 = fmaf(k4[3], q4[3], d3);
    }
    ps[j] = ((d0 + d1) + (d2 + d3)) * scale;
  }
  __syncthreads();
  float mx = -INFINITY;
  for (int j = lane; j < n; j += 64) mx = fmaxf(mx, ps[j]);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) mx = fmaxf(mx, __shfl_xor(mx, o));
  float sum = 0.0f;
  for (int j = lane; j < n; j += 64) {
    const float ex = expf(ps[j] - mx);
    ps[j] = ex;
    sum += ex;
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) sum += __shfl_xor(sum, o);
  __syncthreads();
  for (int j = lane; j < n; j += 64) ps[j] = ps[j] / sum;
  __syncthreads();
  if (lane < DH) {
    // two interleaved partial sums (even / odd position inside each group of four), added last
    float a0 = 0.f, a1 = 0.f;
    auto vrow = [&](int j) {
      return j == t ? row[2 * e + h * DH + lane]
                    : cache[((int64_t)j * R + as[j]) * prow + e + h * DH + lane];
    };
    int j = 0;
    for (; j + 4 <= n; j += 4) {
      const float v0 = vrow(j), v1 = vrow(j + 1), v2 = vrow(j + 2), v3 = vrow(j + 3);
      a0 = fmaf(ps[j], v0, a0);
      a1 = fmaf(ps[j + 1], v1, a1);
      a0 = fmaf(ps[j + 2], v2, a0);
      a1 = fmaf(ps[j + 3], v3, a1);
    }
    for (; j < n; ++j) a0 = fmaf(ps[j], vrow(j), a0);
    ctx[(int64_t)r * e + h * DH + lane] = a0 + a1;
  }
}

// ------------------------------------------------------------------------------------------
// output layer with top-k
// ------------------------------------------------------------------------------------------
struct BanList {
  int id[kSeqTopkMaxBanned];
};

// (value, column) order of the candidates: larger value first, then the smaller column
__device__ __forceinline__ bool cand_before(float v, int c, float bv, int bc) {
  return v > bv || (v == bv && c < bc);
}

// The best (value, column) of the 16 lanes that hold one row of a D fragment, in every one of
// them: the 16 lanes are one DPP row, so four rotate-and-keep-the-better steps (row_ror 8, 4, 2,
// 1) on the VALU replace an LDS-crossbar butterfly. The order is total (columns are distinct),
// so the winner does not depend on the order of the steps.
template <int ROT>
__device__ __forceinline__ void row_best(float& bv, int& bc) {
  constexpr int kRowRor = 0x120 + ROT;  // DPP control: rotate right by ROT inside each row of 16
  const float ov =
      __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(bv), kRowRor, 0xf, 0xf, false));
  const int oc = __builtin_amdgcn_update_dpp(0, bc, kRowRor, 0xf, 0xf, false);
  if (cand_before(ov, oc, bv, bc)) {
    bv = ov;
    bc = oc;
  }
}

__global__ __launch_bounds__(64 * kScWaves) void seq_topk_tile_kernel(
    const float* __restrict__ Hd, int64_t R, int K, const float* __restrict__ W, int V,
    const float* __restrict__ bias, const uint8_t* __restrict__ skip, BanList ban, int n_ct,
    int n16, int rgroups, int Kt, float2* __restrict__ part, float* __restrict__ cval,
    uint8_t* __restrict__ ccol) {
  constexpr int kThr = 64 * kScWaves;
  extern __shared__ __attribute__((aligned(16))) char smem[];
  __bf16* bimg = reinterpret_cast<__bf16*>(smem);
  const int cpitch = 3 * (sc_kpad(K) + 8);
  const int ct = blockIdx.x % n_ct;
  const int rg = blockIdx.x / n_ct;
  const int n0 = ct * kScBN;
  const int s0 = (int)((int64_t)rg * n16 / rgroups), s1 = (int)((int64_t)(rg + 1) * n16 / rgroups);
  const int lane = threadIdx.x & 63;
  const int wave = threadIdx.x >> 6;
  const int r = lane & 15;
  const int g = lane >> 4;
  const int kg = 8 * g;

  if (skip) {  // no live row in this block's share: leave before W is read
    const int64_t lo = (int64_t)16 * s0, hi = (int64_t)16 * s1 < R ? (int64_t)16 * s1 : R;
    int any = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += kThr) any |= skip[i] == 0;
    if (!__syncthreads_or(any)) return;
  }

  sc_build_image(bimg, W, K, V, n0);
  __syncthreads();

  const __bf16* brow = bimg + r * cpitch + kg;
  float bcol[kScNT];
  bool cvalid[kScNT], cand[kScNT];
#pragma unroll
  for (int t = 0; t < kScNT; ++t) {
    const int col = n0 + 16 * t + r;
    cvalid[t] = col < V;
    bcol[t] = (bias && cvalid[t]) ? bias[col] : 0.0f;
    bool banned = false;  // (unused entries of the list hold -1)
#pragma unroll
    for (int q = 0; q < kSeqTopkMaxBanned; ++q) banned = banned || ban.id[q] == col;
    cand[t] = cvalid[t] && !banned;
  }

  for (int j = s0 + wave; j < s1; j += kScWaves) {
    const int64_t m0 = (int64_t)16 * j;
    const int live_r = m0 + r < R && !(skip && skip[m0 + r]);
    if (__ballot(live_r) == 0ull) continue;
    const int64_t arow_i = m0 + r < R ? m0 + r : R - 1;
    const float* arow = Hd + arow_i * (int64_t)K;

    f32x4 acc[kScNT];
    sc_subtile_mma(arow, brow, K, kg, acc);

    // D[row = 4g + reg][col = r]: per row the tile's max and sum of exp, as the sequence scorer
    float x[4][kScNT];
    bool wr[4];
#pragma unroll
    for (int reg = 0; reg < 4; ++reg) {
      const int64_t row = m0 + 4 * g + reg;
      const int live_row = __shfl(live_r, 4 * g + reg);  // lane (r' = 4g + reg, g' = 0) holds it
      wr[reg] = row < R && live_row;
      float m = -INFINITY;
#pragma unroll
      for (int t = 0; t < kScNT; ++t) {
        x[reg][t] = acc[t][reg] + bcol[t];
        if (cvalid[t]) m = fmaxf(m, x[reg][t]);
      }
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) m = fmaxf(m, __shfl_xor(m, o));
      float s = 0.0f;
#pragma unroll
      for (int t = 0; t < kScNT; ++t) s += cvalid[t] ? expf(x[reg][t] - m) : 0.0f;
#pragma unroll
      for (int o = 8; o >= 1; o >>= 1) s += __shfl_xor(s, o);
      if (wr[reg] && r == 0) part[row * n_ct + ct] = make_float2(m, s);
    }
    // the tile's Kt best candidates per row, in order: Kt rounds of (lane-local best of the
    // columns not taken yet, the best of the row's 16 lanes); the four rows of a lane group
    // run side by side
    unsigned taken[4] = {0u, 0u, 0u, 0u};
    for (int k = 0; k < Kt; ++k) {
#pragma unroll
      for (int reg = 0; reg < 4; ++reg) {
        float bv = -INFINITY;
        int bc = 255;  // 255 = none
#pragma unroll
        for (int t = 0; t < kScNT; ++t) {
          const bool free_t = cand[t] && !((taken[reg] >> t) & 1u);
          if (free_t && cand_before(x[reg][t], 16 * t + r, bv, bc)) {
            bv = x[reg][t];
            bc = 16 * t + r;
          }
        }
        row_best<8>(bv, bc);
        row_best<4>(bv, bc);
        row_best<2>(bv, bc);
        row_best<1>(bv, bc);
        if (bc != 255 && (bc & 15) == r) taken[reg] |= 1u << (bc >> 4);
        if (wr[reg] && r == 0) {
          const int64_t o = ((m0 + 4 * g + reg) * n_ct + ct) * Kt + k;
          cval[o] = bv;
          ccol[o] = (uint8_t)bc;
        }
      }
    }
  }
}

// one wave per row: lse from the tiles' (m, s) pairs in index order (as the sequence scorer's
// merge), then K rounds over the tiles' candidates: the best one after the previous winner
__global__ __launch_bounds__(256) void seq_topk_merge_kernel(
    const float2* __restrict__ part, const float* __restrict__ cval,
    const uint8_t* __restrict__ ccol, const uint8_t* __restrict__ skip, int64_t R, int n_ct,
    int Kt, int K, double* __restrict__ lse, float* __restrict__ topv, int* __restrict__ topi) {
  const int lane = threadIdx.x & 63;
  const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (row >= R) return;
  if (skip && skip[row]) return;  // a skipped row's outputs stay as they are
  const float2* p = part + row * n_ct;
  float M = -INFINITY;
  for (int c = lane; c < n_ct; c += 64) M = fmaxf(M, p[c].x);
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) M = fmaxf(M, __shfl_xor(M, o));
  double S = 0.0;
  for (int c = lane; c < n_ct; c += 64) {
    const float2 v = p[c];
    S += (double)v.y * exp((double)v.x - (double)M);
  }
#pragma unroll
  for (int o = 32; o >= 1; o >>= 1) S += __shfl_xor(S, o);  // the same bits in every lane
  if (lane == 0) lse[row] = (double)M + log(S);

  const int64_t nc = (int64_t)n_ct * Kt;
  const float* cv = cval + row * nc;
  const uint8_t* cc = ccol + row * nc;
  constexpr int kNone = 0x7fffffff;
  // a lane's share of the candidates is read once into registers when it fits (V = 5004, K = 10:
  // 13 per lane); larger lists are rescanned from memory every round
  constexpr int kKeep = 16;
  const bool kept = nc <= 64 * kKeep;
  float rv[kKeep];
  int ri[kKeep];
  if (kept) {
#pragma unroll
    for (int u = 0; u < kKeep; ++u) {
      const int64_t i = lane + 64 * u;
      const int col = i < nc ? cc[i] : 255;
      rv[u] = col != 255 ? cv[i] : -INFINITY;
      ri[u] = col != 255 ? (int)(i / Kt) * kScBN + col : kNone;
    }
  }
  float pv = INFINITY;
  int pi = -1;
  for (int k = 0; k < K; ++k) {
    float bv = -INFINITY;
    int bi = kNone;
    auto consider = [&](float v, int idx) {
      const bool after = pi < 0 || v < pv || (v == pv && idx > pi);
      if (idx != kNone && after && (bi == kNone || cand_before(v, idx, bv, bi))) {
        bv = v;
        bi = idx;
      }
    };
    if (kept) {
#pragma unroll
      for (int u = 0; u < kKeep; ++u) consider(rv[u], ri[u]);
    } else {
      for (int64_t i = lane; i < nc; i += 64) {
        const int col = cc[i];
        consider(cv[i], col != 255 ? (int)(i / Kt) * kScBN + col : kNone);
      }
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      const float ov = __shfl_xor(bv, o);
      const int oi = __shfl_xor(bi, o);
      if (oi != kNone && (bi == kNone || cand_before(ov, oi, bv, bi))) {
        bv = ov;
        bi = oi;
      }
    }
    if (bi == kNone) {  // fewer than K candidates: (-inf, -1) from here on
      for (int q = k + lane; q < K; q += 64) {
        topv[row * K + q] = -INFINITY;
        topi[row * K + q] = -1;
      }
      break;
    }
    if (lane == 0) {
      topv[row * K + k] = bv;
      topi[row * K + k] = bi;
    }
    pv = bv;
    pi = bi;
  }
}

// ------------------------------------------------------------------------------------------
// beam bookkeeping: block = utterance, one wave
// ------------------------------------------------------------------------------------------
__global__ __launch_bounds__(64) void attdec_init_kernel(const uint8_t* __restrict__ kmask, int N,
                                                         int Lk, int L, int bos, AttdecState st,
                                                         int* __restrict__ anc) {
  const int b = blockIdx.x, lane = threadIdx.x;
  int any = kmask ? 0 : 1;
  if (kmask)
    for (int j = lane; j < Lk; j += 64) any |= kmask[(int64_t)b * Lk + j] == 0;
  const bool valid = __ballot(any) != 0ull;
  if (lane < N) {
    const int64_t row = (int64_t)b * N + lane;
    const bool live = valid && lane == 0;
    st.score[row] = live ? 0.0 : -(double)INFINITY;
    st.len[row] = 0;
    st.fin[row] = live ? 0 : 2;
    st.tok[row] = bos;
    st.skip[row] = live ? 0 : 1;
  }
  for (int e = lane; e < N * L; e += 64) anc[(int64_t)b * N * L + e] = b * N + e / L;
}

struct BeamPick {
  double key;
  int slot, tok, c;  // c < 0: none
};

__device__ __forceinline__ bool pick_before(const BeamPick& a, const BeamPick& b) {
  if (a.c < 0) return false;
  if (b.c < 0) return true;
  return a.key > b.key ||
         (a.key == b.key && (a.slot < b.slot || (a.slot == b.slot && a.tok < b.tok)));
}

// JOINT: the joint CTC/attention step. A slot carries att (the attention sum, what score is
// without it), ctc (the CTC score of its prefix) and score = (1 - w) * att + w * ctc, each product
// and the sum rounded on its own; a candidate's ctc is cpsi[r][q], and one with cpsi = -inf is no
// candidate when w > 0. link [R][2] receives, per new row, its parent's row and the parent's last
// token (-1: the parent's prefix is empty), which the CTC prefix scorer of the next step reads.
struct JointArgs {
  const double* cpsi;
  double w;
  double* att;
  double* ctc;
  int* link;
};

// FUSED: the joint step with an n-gram LM term. A slot also carries lm (the LM score of its
// prefix); a candidate's is lm[r] + lmsc[r][q] and its score ((1 - w) * att + w * ctc) + lw * lm,
// the LM product and the last sum rounded on their own as well. cpsi may be null when w == 0.
struct LmArgs {
  const double* lmsc;
  double lw;
  double* lm;
};

// BIASED: the fused step with the contextual-bias term. A slot also carries bias (bias(y) of its
// prefix, bias_fin once finished); a candidate's is bsc[r][q] itself, an absolute value, and its
// score (((1 - w) * att + w * ctc) + lw * lm) + bw * bias. lmsc may be null: the LM term is 0 and
// the slots' lm is neither read nor written. The other modes take an empty struct.
struct BiasArgs {
  const double* bsc;
  double bw;
  double* bias;
};
struct NoBiasArgs {};

// (1 - w) * a + w * c with both products and the sum rounded: no contraction into an fma
__device__ __forceinline__ double joint_score(double w, double a, double c) {
#pragma clang fp contract(off)
  const double pa = (1.0 - w) * a;
  const double pc = w * c;
  return pa + pc;
}

// base + lw * l with the product and the sum rounded
__device__ __forceinline__ double fused_score(double base, double lw, double l) {
#pragma clang fp contract(off)
  const double pl = lw * l;
  return base + pl;
}

template <int MODE>
__global__ __launch_bounds__(64) void attdec_beam_step_kernel(
    const double* __restrict__ lse, const float* __restrict__ topv, const int* __restrict__ topi,
    int N, int K, int L, int t, int eos, int pad, const double* __restrict__ norm,
    const int* __restrict__ anc_in, int* __restrict__ anc_out, AttdecState st,
    int* __restrict__ tr_parent, int* __restrict__ tr_token, double* __restrict__ tr_score,
    int B, JointArgs jt, LmArgs la,
    std::conditional_t<MODE == kStepBiased, BiasArgs, NoBiasArgs> ba) {
  constexpr bool JOINT = MODE != kStepBeam;
  constexpr bool BIASED = MODE == kStepBiased;
  constexpr bool FUSED = MODE == kStepFused || BIASED;
  __shared__ double s_key[kAdMaxCand], s_sc[kAdMaxCand];
  __shared__ int s_tok[kAdMaxCand];
  __shared__ uint8_t s_ok[kAdMaxCand];
  __shared__ double s_score[kAdMaxN];
  __shared__ int s_len[kAdMaxN], s_fin[kAdMaxN], s_sel[kAdMaxN], s_par[kAdMaxN];
  __shared__ double s_ca[JOINT ? kAdMaxCand : 1], s_cc[JOINT ? kAdMaxCand : 1];
  __shared__ double s_att[JOINT ? kAdMaxN : 1], s_ctc[JOINT ? kAdMaxN : 1];
  __shared__ int s_last[JOINT ? kAdMaxN : 1];
  __shared__ double s_cl[FUSED ? kAdMaxCand : 1], s_lm[FUSED ? kAdMaxN : 1];
  __shared__ double s_cb[BIASED ? kAdMaxCand : 1], s_bias[BIASED ? kAdMaxN : 1];
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t r0 = (int64_t)b * N;
  if (lane < N) {
    s_score[lane] = st.score[r0 + lane];
    s_len[lane] = st.len[r0 + lane];
    s_fin[lane] = st.fin[r0 + lane];
    if constexpr (JOINT) {
      s_att[lane] = jt.att[r0 + lane];
      s_ctc[lane] = jt.ctc[r0 + lane];
      s_last[lane] = s_len[lane] > 0 ? (int)st.tok[r0 + lane] : -1;
    }
    if constexpr (BIASED) {
      s_lm[lane] = la.lmsc ? la.lm[r0 + lane] : 0.0;
      s_bias[lane] = ba.bias[r0 + lane];
    } else if constexpr (FUSED) {
      s_lm[lane] = la.lm[r0 + lane];
    }
  }
  __syncthreads();
  const int nk = N * K, nc = nk + N;
  for (int c = lane; c < nc; c += 64) {
    bool ok;
    double sc = 0.0, key = 0.0;
    int tok = -1;
    if (c < nk) {
      const int r = c / K;
      const int64_t o = (r0 + r) * K + (c - r * K);
      ok = s_fin[r] == 0;
      if (ok) {
        tok = topi[o];
        ok = tok >= 0;
      }
      if constexpr (JOINT) {
        if (ok) {
          const double a = s_att[r] + ((double)topv[o] - lse[r0 + r]);
          double cc;
          if constexpr (FUSED)
            cc = jt.cpsi ? jt.cpsi[o] : 0.0;
          else
            cc = jt.cpsi[o];
          s_ca[c] = a;
          s_cc[c] = cc;
          if (jt.w > 0.0) {
            ok = cc != -(double)INFINITY;
            sc = joint_score(jt.w, a, cc);
          } else {
            sc = a;
          }
          if constexpr (BIASED) {
            const double l = la.lmsc ? s_lm[r] + la.lmsc[o] : 0.0;
            const double bv = ba.bsc[o];
            s_cl[c] = l;
            s_cb[c] = bv;
            sc = fused_score(fused_score(sc, la.lw, l), ba.bw, bv);
          } else if constexpr (FUSED) {
            const double l = s_lm[r] + la.lmsc[o];
            s_cl[c] = l;
            sc = fused_score(sc, la.lw, l);
          }
        }
        if (ok) {
          const int n = s_len[r] + 1;
          key = sc / norm[n < L ? n : L];
        }
      } else if (ok) {
        sc = s_score[r] + ((double)topv[o] - lse[r0 + r]);
        const int n = s_len[r] + 1;
        key = sc / norm[n < L ? n : L];
      }
    } else {
      const int r = c - nk;
      ok = s_fin[r] == 1;
      if (ok) {
        sc = s_score[r];
        const int n = s_len[r];
        key = sc / norm[n < L ? n : L];
      }
    }
    s_ok[c] = ok ? 1 : 0;
    s_sc[c] = sc;
    s_key[c] = key;
    s_tok[c] = tok;
  }
  __syncthreads();
  for (int k = 0; k < N; ++k) {
    BeamPick best{0.0, 0, 0, -1};
    for (int c = lane; c < nc; c += 64) {
      if (!s_ok[c]) continue;
      const BeamPick p{s_key[c], c < nk ? c / K : c - nk, s_tok[c], c};
      if (pick_before(p, best)) best = p;
    }
#pragma unroll
    for (int o = 32; o >= 1; o >>= 1) {
      BeamPick q;
      q.key = __shfl_xor(best.key, o);
      q.slot = __shfl_xor(best.slot, o);
      q.tok = __shfl_xor(best.tok, o);
      q.c = __shfl_xor(best.c, o);
      if (pick_before(q, best)) best = q;
    }
    if (lane == 0) {
      s_sel[k] = best.c;
      if (best.c >= 0) s_ok[best.c] = 0;
    }
    __syncthreads();
  }
  if (lane < N) {
    const int c = s_sel[lane];
    const int64_t row = r0 + lane;
    const int64_t to = ((int64_t)t * B + b) * N + lane;
    double sc = -(double)INFINITY;
    int len = 0, fin = 2, par = -1, token = -2;
    if (c >= nk) {  // a finished slot, carried over unchanged
      par = c - nk;
      sc = s_score[par];
      len = s_len[par];
      fin = 1;
      token = -1;
    } else if (c >= 0) {
      par = c / K;
      token = s_tok[c];
      sc = s_sc[c];
      len = s_len[par] + 1;
      fin = token == eos ? 1 : 0;
    }
    if constexpr (JOINT) {
      double a = -(double)INFINITY, cc = -(double)INFINITY;
      if (c >= nk) {
        a = s_att[par];
        cc = s_ctc[par];
      } else if (c >= 0) {
        a = s_ca[c];
        cc = s_cc[c];
      }
      jt.att[row] = a;
      jt.ctc[row] = cc;
      if constexpr (FUSED) {
        double l = -(double)INFINITY;
        if (c >= nk)
          l = s_lm[par];
        else if (c >= 0)
          l = s_cl[c];
        if constexpr (BIASED) {
          if (la.lmsc) la.lm[row] = l;
          double bv = -(double)INFINITY;
          if (c >= nk)
            bv = s_bias[par];
          else if (c >= 0)
            bv = s_cb[c];
          ba.bias[row] = bv;
        } else {
          la.lm[row] = l;
        }
      }
      jt.link[2 * row] = (int)r0 + (par < 0 ? lane : par);
      jt.link[2 * row + 1] = (c >= 0 && c < nk) ? s_last[par] : -1;
    }
    st.score[row] = sc;
    st.len[row] = len;
    st.fin[row] = (uint8_t)fin;
    st.tok[row] = fin == 0 ? token : pad;
    st.skip[row] = fin == 0 ? 0 : 1;
    tr_parent[to] = par;
    tr_token[to] = token;
    tr_score[to] = sc;
    s_par[lane] = par;
  }
  __syncthreads();
  // the new rows of the ancestry table: the parent's positions 0..t-1, then the parent itself
  const int t1 = t + 1;
  for (int e = lane; e < N * t1; e += 64) {
    const int k = e / t1, j = e - k * t1;
    const int par = s_par[k] < 0 ? k : s_par[k];
    anc_out[(r0 + k) * L + j] = j < t ? anc_in[(r0 + par) * L + j] : (int)r0 + par;
  }
}

__global__ __launch_bounds__(64) void attdec_finalize_kernel(
    const int* __restrict__ tr_parent, const int* __restrict__ tr_token, AttdecState st, int B,
    int N, int L, int eos, int* __restrict__ hyp, int* __restrict__ hyp_len,
    int* __restrict__ n_hyp, double* __restrict__ score, uint8_t* __restrict__ finished) {
  const int b = blockIdx.x, lane = threadIdx.x;
  const int64_t r0 = (int64_t)b * N;
  for (int e = lane; e < N * L; e += 64) hyp[r0 * L + e] = -1;
  __syncthreads();
  int fin = 2;
  if (lane < N) {
    const int64_t row = r0 + lane;
    fin = st.fin[row];
    int hl = fin == 2 ? 0 : st.len[row] - (fin == 1 ? 1 : 0);
    hl = hl < 0 ? 0 : (hl > L ? L : hl);
    hyp_len[row] = hl;
    score[row] = fin == 2 ? -(double)INFINITY : st.score[row];
    finished[row] = fin == 1 ? 1 : 0;
    int cur = lane, pos = hl - 1;
    for (int t = L - 1; t >= 0 && fin != 2; --t) {
      const int64_t o = ((int64_t)t * B + b) * N + cur;
      const int tk = tr_token[o], par = tr_parent[o];
      if (tk >= 0 && tk != eos && pos >= 0) hyp[row * L + pos--] = tk;
      if (par < 0 || par >= N) break;
      cur = par;
    }
  }
  const unsigned long long live = __ballot(lane < N && fin != 2);
  if (lane == 0) n_hyp[b] = __popcll(live);
}

}  // namespace

bool attdec_supported(int64_t N, int64_t d, int64_t H, int64_t Lk, int64_t L) {
  if (N < 1 || N > kAdMaxN || H < 1 || d < 16 || d > 256 || d % 16 || d % H) return false;
  const int64_t dh = d / H;
  if (!(dh == 16 || dh == 32 || dh == 36 || dh == 64)) return false;
  if (L < 1 || L + 1 > kAdMaxPos) return false;
  return decattn_supported(1, Lk, dh);
}

void launch_decattn_step(const float* qkv, int64_t sq, float* cache, const int* anc,
                         const uint8_t* skip, int64_t R, int64_t H, int64_t dh, int64_t L,
                         int64_t t, float* ctx, hipStream_t s) {
  if (R == 0) return;
  const float scale = 1.0f / sqrtf((float)dh);
  const dim3 grid((unsigned)(R * H)), block(64);
#define OB_AD_STEP(D)                                                                          \
  hipLaunchKernelGGL(decattn_step_kernel<D>, grid, block, 0, s, qkv, sq, cache, anc, skip,     \
                     (int)R, (int)H, (int)L, (int)t, scale, ctx)
  switch (dh) {
    case 16: OB_AD_STEP(16); break;
    case 32: OB_AD_STEP(32); break;
    case 36: OB_AD_STEP(36); break;
    default: OB_AD_STEP(64); break;
  }
#undef OB_AD_STEP
}

namespace {
inline int topk_tile_k(int64_t K) { return (int)std::min<int64_t>(K, kScBN); }
}  // namespace

size_t seq_topk_workspace(int64_t R, int64_t d, int64_t V, int64_t K) {
  (void)d;
  const unsigned __int128 n_ct = (unsigned __int128)ceil_div(V, kScBN);
  const unsigned __int128 per_row = n_ct * 8 + n_ct * (unsigned)topk_tile_k(K) * 5;
  const unsigned __int128 bytes = (unsigned __int128)R * per_row;
  return bytes > (unsigned __int128)(SIZE_MAX / 2) ? 0 : (size_t)((bytes + 7) / 8 * 8);
}

void launch_seq_topk(const float* hidden, int64_t R, int64_t d, const float* weight,
                     const float* bias, int64_t V, const int* banned, int n_banned,
                     const uint8_t* skip, int64_t K, void* ws, double* lse, float* topv,
                     int* topi, hipStream_t s) {
  if (R == 0) return;
  const int n_ct = (int)ceil_div(V, kScBN);
  const int n16 = (int)ceil_div(R, 16);
  const int Kt = topk_tile_k(K);
  const size_t lds = sc_lds_bytes((int)d);
  const int per_cu = (int)std::min<size_t>(kScLdsCU / lds, 2);
  int64_t rgroups = std::max<int64_t>(1, (int64_t)256 * per_cu / n_ct);
  rgroups = std::min<int64_t>(rgroups, ceil_div(n16, kScWaves));
  BanList ban;
  for (int q = 0; q < kSeqTopkMaxBanned; ++q) ban.id[q] = q < n_banned ? banned[q] : -1;
  float2* part = static_cast<float2*>(ws);
  float* cval = reinterpret_cast<float*>(part + R * n_ct);
  uint8_t* ccol = reinterpret_cast<uint8_t*>(cval + R * n_ct * Kt);
  hipLaunchKernelGGL(seq_topk_tile_kernel, dim3((unsigned)(rgroups * n_ct)), dim3(64 * kScWaves),
                     lds, s, hidden, R, (int)d, weight, (int)V, bias, skip, ban, n_ct, n16,
                     (int)rgroups, Kt, part, cval, ccol);
  hipLaunchKernelGGL(seq_topk_merge_kernel, dim3((unsigned)ceil_div(R, 4)), dim3(256), 0, s,
                     (const float2*)part, (const float*)cval, (const uint8_t*)ccol, skip, R, n_ct,
                     Kt, (int)K, lse, topv, topi);
}

void launch_attdec_init(const uint8_t* kmask, int64_t B, int64_t N, int64_t Lk, int64_t L, int bos,
                        const AttdecState& st, int* anc, hipStream_t s) {
  if (B == 0) return;
  hipLaunchKernelGGL(attdec_init_kernel, dim3((unsigned)B), dim3(64), 0, s, kmask, (int)N, (int)Lk,
                     (int)L, bos, st, anc);
}

void launch_attdec_step(int mode, const double* lse, const float* topv, const int* topi,
                        const double* cpsi, double w, const double* lmsc, double lw, int64_t B,
                        int64_t N, int64_t K, int64_t L, int64_t t, int eos, int pad,
                        const double* norm, const int* anc_in, int* anc_out,
                        const AttdecState& st, double* att, double* ctc, double* lm, int* link,
                        int* tr_parent, int* tr_token, double* tr_score, hipStream_t s,
                        const double* bsc, double bw, double* bias) {
  if (B == 0) return;
  const JointArgs jt = mode == kStepBeam ? JointArgs{} : JointArgs{cpsi, w, att, ctc, link};
  const LmArgs la = mode >= kStepFused ? LmArgs{lmsc, lw, lm} : LmArgs{};
  auto launch = [&](auto kernel, auto ba) {
    hipLaunchKernelGGL(kernel, dim3((unsigned)B), dim3(64), 0, s, lse, topv, topi, (int)N, (int)K,
                       (int)L, (int)t, eos, pad, norm, anc_in, anc_out, st, tr_parent, tr_token,
                       tr_score, (int)B, jt, la, ba);
  };
  switch (mode) {
    case kStepBeam: launch(attdec_beam_step_kernel<kStepBeam>, NoBiasArgs{}); break;
    case kStepJoint: launch(attdec_beam_step_kernel<kStepJoint>, NoBiasArgs{}); break;
    case kStepFused: launch(attdec_beam_step_kernel<kStepFused>, NoBiasArgs{}); break;
    case kStepBiased:
      launch(attdec_beam_step_kernel<kStepBiased>, BiasArgs{bsc, bw, bias});
      break;
  }
}

void launch_attdec_finalize(const int* tr_parent, const int* tr_token, const AttdecState& st,
                            int64_t B, int64_t N, int64_t L, int eos, int* hyp, int* hyp_len,
                            int* n_hyp, double* score, uint8_t* finished, hipStream_t s) {
  if (B == 0) return;
  hipLaunchKernelGGL(attdec_finalize_kernel, dim3((unsigned)B), dim3(64), 0, s, tr_parent,
                     tr_token, st, (int)B, (int)N, (int)L, eos, hyp, hyp_len, n_hyp, score,
                     finished);
}

}  // namespace ob
