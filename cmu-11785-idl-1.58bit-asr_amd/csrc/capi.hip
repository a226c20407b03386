// capi.hip — the C ABI declared in include/onebit_hip.h: argument validation, workspace
// carving and launch-error reporting around the launchers in quant.hip / gemm.hip.
#include <float.h>

#include <algorithm>
#include <vector>

#include "../../include/onebit_hip.h"
#include "ob_launch.h"
#include <stdint.h>

using namespace ob;

namespace {

constexpr int kAbiVersion = 4;  // 4 (round 6): ob_decattn_bwd consumes probs (dS' written there)

inline hipStream_t as_stream(void* s) { return reinterpret_cast<hipStream_t>(s); }

inline bool aligned4(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 3) == 0; }
inline bool misaligned8(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 7) != 0; }

inline int check_bits(int bits) { return (bits == 1 || bits == 2) ? OB_OK : OB_ERR_BITWIDTH; }

inline int launched() {
  const hipError_t e = hipGetLastError();
  return e == hipSuccess ? OB_OK : OB_ERR_HIP;
}

inline size_t align_up(size_t x) { return (x + 255) & ~size_t(255); }

struct DwWorkspace {
  size_t part, part_db, apart, total;
};

// G > 1: one layer's share of a grouped launch (plan of the G layers' N_total = G * N)
DwWorkspace dw_layout(int64_t P, int64_t M, int64_t N, int64_t K, int64_t G = 1) {
  const DwPlan p = plan_dw_passes(P, M, G * N, K);
  DwWorkspace w;
  w.part = align_up(sizeof(float) * (size_t)p.chunks * (size_t)N * (size_t)K);
  w.part_db = align_up(sizeof(float) * (size_t)p.chunks * (size_t)N);
  const int64_t napart = std::max<int64_t>(ste_reduce_blocks(N * K + N),
                                           p.tiles_n * p.tiles_k * p.chunks);
  w.apart = align_up(16 + sizeof(float) * (size_t)napart);
  w.total = w.part + w.part_db + w.apart;
  return w;
}

}  // namespace

extern "C" {

int ob_abi_version(void) { return kAbiVersion; }

const char* ob_status_string(int status) {
  switch (status) {
    case OB_OK: return "ok";
    case OB_ERR_NULL: return "null pointer argument";
    case OB_ERR_SHAPE: return "invalid shape";
    case OB_ERR_BITWIDTH: return "bitwidth must be one of {1,2,32}";
    case OB_ERR_WORKSPACE: return "workspace too small";
    case OB_ERR_ALIGN: return "pointer not 4-byte aligned";
    case OB_ERR_HIP: return "HIP launch error";
    default: return "unknown status";
  }
}

int ob_quant_pack(const float* W, const float* alpha, int alpha_raw, int bits, int64_t N,
                  int64_t K, uint32_t* codes, uint32_t* codes_t, void* stream) {
  if (int st = check_bits(bits)) return st;
  if (N < 0 || K < 0) return OB_ERR_SHAPE;
  if (!alpha || (N * K > 0 && !W)) return OB_ERR_NULL;
  if (!aligned4(W) || !aligned4(codes) || !aligned4(codes_t)) return OB_ERR_ALIGN;
  launch_quant_pack(W, alpha, alpha_raw, bits, nullptr, N, K, codes, codes_t, as_stream(stream));
  return launched();
}

int ob_quant_pack_dyn(const float* W, const float* alpha, int alpha_raw, const int32_t* bits_dev,
                      int64_t N, int64_t K, uint32_t* codes, uint32_t* codes_t, void* stream) {
  if (N < 0 || K < 0) return OB_ERR_SHAPE;
  if (!alpha || !bits_dev || (N * K > 0 && !W)) return OB_ERR_NULL;
  if (!aligned4(W) || !aligned4(codes) || !aligned4(codes_t) || !aligned4(bits_dev))
    return OB_ERR_ALIGN;
  launch_quant_pack(W, alpha, alpha_raw, 2, bits_dev, N, K, codes, codes_t, as_stream(stream));
  return launched();
}

int64_t ob_quant_pack_item_blocks(int64_t N, int64_t K) {
  if (N < 0 || K < 0) return OB_ERR_SHAPE;
  return quant_pack_item_blocks(N, K);
}

int64_t ob_weight_bf16_item_blocks(int64_t N, int64_t K) {
  if (N < 0 || K < 0) return OB_ERR_SHAPE;
  return quant_pack_item_blocks16(N, K);
}

int ob_quant_pack_group(const ob_pack_item* items, int n_items, int64_t total_blocks,
                        void* stream) {
  if (n_items < 0 || total_blocks < 0 || total_blocks > 0x7fffffff) return OB_ERR_SHAPE;
  if (n_items > 0 && !items) return OB_ERR_NULL;
  if (((uintptr_t)items & 7u) != 0) return OB_ERR_ALIGN;
  launch_quant_pack_group(items, n_items, total_blocks, as_stream(stream));
  return launched();
}

int ob_quant_dequant(const float* W, const float* alpha, int alpha_raw, int bits, int64_t n,
                     float* W_hat, void* stream) {
  if (int st = check_bits(bits)) return st;
  if (n < 0) return OB_ERR_SHAPE;
  if (!alpha || (n > 0 && (!W || !W_hat))) return OB_ERR_NULL;
  if (!aligned4(W) || !aligned4(W_hat)) return OB_ERR_ALIGN;
  launch_quant_dequant(W, alpha, alpha_raw, bits, n, W_hat, as_stream(stream));
  return launched();
}

size_t ob_quant_ste_bwd_workspace(int64_t n) {
  if (n < 0) return 0;
  return align_up(16 + sizeof(float) * (size_t)(ste_reduce_blocks(n) + 1));
}

int ob_quant_ste_bwd(const float* grad_W_hat, const float* W, const float* alpha, int alpha_raw,
                     int bits, int64_t n, float* grad_W, float* grad_alpha, void* ws,
                     size_t ws_bytes, void* stream) {
  if (int st = check_bits(bits)) return st;
  if (n < 0) return OB_ERR_SHAPE;
  if (!alpha || !grad_alpha || !ws || (n > 0 && (!grad_W_hat || !W || !grad_W)))
    return OB_ERR_NULL;
  if (ws_bytes < ob_quant_ste_bwd_workspace(n)) return OB_ERR_WORKSPACE;
  // ws: [ticket (16 B)][block partials]
  uint32_t* ticket = static_cast<uint32_t*>(ws);
  float* apart = reinterpret_cast<float*>(static_cast<char*>(ws) + 16);
  launch_zero_words(ticket, 1, as_stream(stream));
  launch_ste_reduce(grad_W_hat, 1, n, nullptr, 0, W, alpha, alpha_raw, bits, nullptr, grad_W,
                    nullptr, apart, ticket, grad_alpha, as_stream(stream));
  return launched();
}

int ob_bitlinear_fwd(const float* X, int64_t M, int64_t K, const uint32_t* codes,
                     const float* alpha, int alpha_raw, const float* bias, int64_t N, float* Y,
                     void* stream) {
  if (M < 0 || K < 0 || N < 0) return OB_ERR_SHAPE;
  if (!alpha || (M * N > 0 && !Y) || (M * K > 0 && !X) || (N * K > 0 && !codes))
    return OB_ERR_NULL;
  if (!aligned4(X) || !aligned4(Y) || !aligned4(bias)) return OB_ERR_ALIGN;
  launch_ternary_gemm(X, M, K, codes, N, alpha, alpha_raw, bias, Y, as_stream(stream));
  return launched();
}

int ob_bitlinear_fwd_signacc(const float* X, int64_t M, int64_t K, const uint32_t* codes,
                             const float* alpha, int alpha_raw, const float* bias, int64_t N,
                             float* Y, void* stream) {
  if (M < 0 || K < 0 || N < 0) return OB_ERR_SHAPE;
  if (!alpha || (M * N > 0 && !Y) || (M * K > 0 && !X) || (N * K > 0 && !codes))
    return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || !aligned4(Y) || !aligned4(bias)) return OB_ERR_ALIGN;
  if (!launch_ternary_gemm_signacc(X, M, K, codes, N, alpha, alpha_raw, bias, Y, as_stream(stream)))
    return OB_ERR_SHAPE;
  return launched();
}

int ob_bitlinear_bwd_dx(const float* dY, int64_t M, int64_t N, const uint32_t* codes_t,
                        const float* alpha, int alpha_raw, int64_t K, float* dX, void* stream) {
  if (M < 0 || K < 0 || N < 0) return OB_ERR_SHAPE;
  if (!alpha || (M * K > 0 && !dX) || (M * N > 0 && !dY) || (N * K > 0 && !codes_t))
    return OB_ERR_NULL;
  if (!aligned4(dY) || !aligned4(dX)) return OB_ERR_ALIGN;
  // dX = a * dY . Q: the same ternary GEMM with the roles of N and K exchanged.
  launch_ternary_gemm(dY, M, N, codes_t, K, alpha, alpha_raw, nullptr, dX, as_stream(stream));
  return launched();
}

size_t ob_bitlinear_bwd_dw_workspace(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 0 || K < 0) return 0;
  return dw_layout(1, M, N, K).total;
}

namespace {

// P stacked passes of M rows each (P = 1: the single-call entries). Pass bitwidths come
// from pass_bits (device [P]) when given, else from bits / bits_dev for the one pass.
int bwd_dw_impl(const float* dY, const float* X, int64_t P, int64_t M, int64_t N, int64_t K,
                const float* W, const float* alpha, int alpha_raw, int bits,
                const int32_t* bits_dev, const int32_t* pass_bits, float* dW, float* dalpha,
                float* db, void* ws, size_t ws_bytes, void* stream,
                DwFinish* defer = nullptr, DwFinishEntry* table = nullptr, int slot = 0,
                int64_t start = 0, int64_t* n_blocks = nullptr) {
  if (n_blocks) *n_blocks = 0;
  if (M < 0 || N < 0 || K < 0 || P < 1 || P > kMaxPasses) return OB_ERR_SHAPE;
  if (!alpha || !dalpha || !ws || (N * K > 0 && (!W || !dW)) || (M > 0 && (!dY || (K > 0 && !X))))
    return OB_ERR_NULL;
  if (!aligned4(dY) || !aligned4(X) || !aligned4(dW) || !aligned4(db) || !aligned4(bits_dev) ||
      !aligned4(pass_bits))
    return OB_ERR_ALIGN;
  const DwWorkspace L = dw_layout(P, M, N, K);
  if (ws_bytes < L.total) return OB_ERR_WORKSPACE;
  const DwPlan p = plan_dw_passes(P, M, N, K);
  char* base = static_cast<char*>(ws);
  float* part = reinterpret_cast<float*>(base);
  float* part_db = db ? reinterpret_cast<float*>(base + L.part) : nullptr;
  // apart region: [ticket (16 B)][block partials]
  uint32_t* ticket = reinterpret_cast<uint32_t*>(base + L.part + L.part_db);
  float* apart = reinterpret_cast<float*>(base + L.part + L.part_db + 16);
  hipStream_t s = as_stream(stream);
  int chunks = (int)p.chunks;
  int cpp = (int)p.chunks_per_pass;
  if (M == 0 || N == 0) {
    // No rows: every gradient is zero. Zero the first slab and reduce one chunk.
    launch_zero_words(part, N * K, s);
    if (db) launch_zero_words(part_db, N, s);
    launch_zero_words(ticket, 1, s);
    chunks = 1;
    cpp = 1;
    P = 1;
  } else if (p.variant >= 9) {  // LDS path: alpha partials in the GEMM, no ticket
    const DwAlpha al{W, alpha, alpha_raw, bits, reinterpret_cast<const int*>(bits_dev),
                     reinterpret_cast<const int*>(pass_bits), apart};
    const DwFinish fin{part, chunks, N * K, part_db, db ? N : 0, W, alpha, alpha_raw, apart,
                       (int)(p.tiles_n * p.tiles_k * p.chunks), dW, db, dalpha};
    if (table) {  // finish deferred to ob_dw_finish_table (entry written by the partial launch)
      const DwFinishEntry ent{fin, start};
      launch_dw_partial_group_defer(&dY, 1, X, P * M, N, K, p, &part, &part_db, &al, table, slot,
                                    &ent, s);
      if (n_blocks) *n_blocks = dw_finish_blocks(fin);
      return launched();
    }
    launch_dw_partial(dY, X, P * M, N, K, p, part, part_db, ticket, s, &al);
    if (defer) {  // the caller launches it (grouped with other layers' finishes)
      *defer = fin;
      return launched();
    }
    launch_dw_finish(fin.part, fin.chunks, fin.nk, fin.part_db, fin.n_db, fin.W, fin.alpha,
                     fin.alpha_raw, fin.apart, fin.n_apart, fin.dW, fin.db, fin.dalpha, s);
    return launched();
  } else {
    launch_dw_partial(dY, X, P * M, N, K, p, part, part_db, ticket, s);
  }
  if (pass_bits)
    launch_ste_reduce_passes(part, (int)P, cpp, N * K, part_db, db ? N : 0, W, alpha, alpha_raw,
                             reinterpret_cast<const int*>(pass_bits), dW, db, apart, ticket,
                             dalpha, s);
  else
    launch_ste_reduce(part, chunks, N * K, part_db, db ? N : 0, W, alpha, alpha_raw, bits,
                      reinterpret_cast<const int*>(bits_dev), dW, db, apart, ticket, dalpha, s);
  return launched();
}

}  // namespace

int ob_bitlinear_bwd_dw(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                        const float* W, const float* alpha, int alpha_raw, int bits, float* dW,
                        float* dalpha, float* db, void* ws, size_t ws_bytes, void* stream) {
  if (int st = check_bits(bits)) return st;
  return bwd_dw_impl(dY, X, 1, M, N, K, W, alpha, alpha_raw, bits, nullptr, nullptr, dW, dalpha,
                     db, ws, ws_bytes, stream);
}

int ob_bitlinear_bwd_dw_dyn(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                            const float* W, const float* alpha, int alpha_raw,
                            const int32_t* bits_dev, float* dW, float* dalpha, float* db, void* ws,
                            size_t ws_bytes, void* stream) {
  if (!bits_dev) return OB_ERR_NULL;
  return bwd_dw_impl(dY, X, 1, M, N, K, W, alpha, alpha_raw, 2, bits_dev, nullptr, dW, dalpha,
                     db, ws, ws_bytes, stream);
}

int ob_bitlinear_fwd_passes(const float* X, int64_t P, int64_t M, int64_t K,
                            const uint32_t* codes2, const uint32_t* codes1,
                            const int32_t* pass_bits, const float* alpha, int alpha_raw,
                            const float* bias, int64_t N, float* Y, void* stream) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (!alpha || !pass_bits || (M * N > 0 && !Y) || (M * K > 0 && !X) ||
      (N * K > 0 && (!codes2 || !codes1)))
    return OB_ERR_NULL;
  if (!aligned4(X) || !aligned4(Y) || !aligned4(bias) || !aligned4(pass_bits)) return OB_ERR_ALIGN;
  launch_ternary_gemm_passes(X, (int)P, M, K, codes2, codes1, reinterpret_cast<const int*>(pass_bits),
                             N, alpha, alpha_raw, bias, Y, as_stream(stream));
  return launched();
}

int ob_bitlinear_fwd_passes_group(int64_t G, const float* X, int64_t P, int64_t M, int64_t K,
                                  const uint32_t* const* codes2, const uint32_t* const* codes1,
                                  const int32_t* pass_bits, const float* const* alpha,
                                  int alpha_raw, const float* const* bias, int64_t N,
                                  float* const* Y, void* stream) {
  if (G < 1 || G > 3 || M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (!codes2 || !codes1 || !alpha || !bias || !Y || !pass_bits || (M * K > 0 && !X))
    return OB_ERR_NULL;
  for (int64_t i = 0; i < G; ++i) {
    if (!alpha[i] || (M * N > 0 && !Y[i]) || (N * K > 0 && (!codes2[i] || !codes1[i])))
      return OB_ERR_NULL;
    if (!aligned4(Y[i]) || !aligned4(bias[i])) return OB_ERR_ALIGN;
  }
  if (!aligned4(X) || !aligned4(pass_bits)) return OB_ERR_ALIGN;
  if (!launch_ternary_gemm_passes_group(X, (int)P, M, K, (int)G, codes2, codes1,
                                        reinterpret_cast<const int*>(pass_bits), N, alpha,
                                        alpha_raw, bias, Y, as_stream(stream)))
    return OB_ERR_SHAPE;
  return launched();
}

namespace {

// Shared argument checks of the fused-epilogue GEMM entries.
int fused_gemm_check(const float* A, int64_t P, int64_t M, int64_t K, const uint32_t* codes2,
                     const uint32_t* codes1, const int32_t* pass_bits, const float* alpha,
                     int64_t N, const float* out, float p_drop, const uint64_t* rng) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (!(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  if (P > 1 && !pass_bits) return OB_ERR_NULL;
  if (!alpha || (M * N > 0 && !out) || (M * K > 0 && !A) ||
      (N * K > 0 && (!codes2 || (pass_bits && !codes1))) || (p_drop > 0.0f && !rng))
    return OB_ERR_NULL;
  if (!aligned4(A) || !aligned4(out) || !aligned4(pass_bits)) return OB_ERR_ALIGN;
  return OB_OK;
}

}  // namespace

int ob_bitlinear_fwd_swish_drop(const float* X, int64_t P, int64_t M, int64_t K,
                                const uint32_t* codes2, const uint32_t* codes1,
                                const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                const float* bias, int64_t N, float p_drop, const uint64_t* rng,
                                int64_t rng_offset, float* Y_pre, float* Y_act, void* stream) {
  if (int st = fused_gemm_check(X, P, M, K, codes2, codes1, pass_bits, alpha, N, Y_act, p_drop, rng))
    return st;
  if (M * N > 0 && !Y_pre) return OB_ERR_NULL;
  if (!aligned4(Y_pre) || !aligned4(bias)) return OB_ERR_ALIGN;
  TgemmEpi ep{};
  ep.mode = kEpiSwishDrop;
  ep.C2 = Y_pre;
  ep.p_drop = p_drop;
  ep.rng = rng;
  ep.rng_off = (uint64_t)rng_offset;
  launch_ternary_gemm_passes(X, (int)P, M, K, codes2, pass_bits ? codes1 : codes2,
                             reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw, bias,
                             Y_act, as_stream(stream), &ep);
  return launched();
}

int ob_bitlinear_fwd_residual(const float* X, int64_t P, int64_t M, int64_t K,
                              const uint32_t* codes2, const uint32_t* codes1,
                              const int32_t* pass_bits, const float* alpha, int alpha_raw,
                              const float* bias, int64_t N, const float* R, float rscale,
                              float p_drop, const uint64_t* rng, int64_t rng_offset,
                              const int32_t* lens, int64_t T, float* Y, void* stream) {
  if (int st = fused_gemm_check(X, P, M, K, codes2, codes1, pass_bits, alpha, N, Y, p_drop, rng))
    return st;
  if (M * N > 0 && !R) return OB_ERR_NULL;
  if (lens && (T < 1 || (P * M) % T)) return OB_ERR_SHAPE;
  if (T > 0x7fffffff) return OB_ERR_SHAPE;
  if (!aligned4(R) || !aligned4(bias) || !aligned4(lens)) return OB_ERR_ALIGN;
  TgemmEpi ep{};
  ep.mode = kEpiResidual;
  ep.R = R;
  ep.rscale = rscale;
  ep.lens = reinterpret_cast<const int*>(lens);
  ep.T = (int)T;
  ep.p_drop = p_drop;
  ep.rng = rng;
  ep.rng_off = (uint64_t)rng_offset;
  launch_ternary_gemm_passes(X, (int)P, M, K, codes2, pass_bits ? codes1 : codes2,
                             reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw, bias, Y,
                             as_stream(stream), &ep);
  return launched();
}

int ob_bitlinear_fwd_residual_ln(const float* X, int64_t P, int64_t M, int64_t K,
                                 const uint32_t* codes2, const uint32_t* codes1,
                                 const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                 const float* bias, int64_t N, const float* R, float rscale,
                                 float p_drop, const uint64_t* rng, int64_t rng_offset,
                                 const int32_t* lens, int64_t T, float* Y, int nln,
                                 const float* ln_w0, const float* ln_b0, float eps0, float* ln_y0,
                                 float* ln_mean0, float* ln_rstd0, const float* ln_w1,
                                 const float* ln_b1, float eps1, float* ln_y1, float* ln_mean1,
                                 float* ln_rstd1, void* stream) {
  if (int st = fused_gemm_check(X, P, M, K, codes2, codes1, pass_bits, alpha, N, Y, p_drop, rng))
    return st;
  if (nln < 1 || nln > 2) return OB_ERR_SHAPE;
  if (!ternary_residual_ln_supported(K, N, alpha_raw)) return OB_ERR_SHAPE;  // caller falls back
  if (M * N > 0 && (!R || !ln_y0 || !ln_mean0 || !ln_rstd0 ||
                    (nln > 1 && (!ln_y1 || !ln_mean1 || !ln_rstd1))))
    return OB_ERR_NULL;
  if (lens && (T < 1 || (P * M) % T)) return OB_ERR_SHAPE;
  if (T > 0x7fffffff) return OB_ERR_SHAPE;
  auto a16 = [](const void* q) { return (reinterpret_cast<uintptr_t>(q) & 15) == 0; };
  if (!a16(X) || !a16(R) || !a16(Y) || !a16(ln_y0) || !a16(ln_w0) || !a16(ln_b0) ||
      (nln > 1 && (!a16(ln_y1) || !a16(ln_w1) || !a16(ln_b1))) || !aligned4(bias) ||
      !aligned4(lens) || !aligned4(ln_mean0) || !aligned4(ln_rstd0) || !aligned4(ln_mean1) ||
      !aligned4(ln_rstd1))
    return OB_ERR_ALIGN;
  TgemmEpi ep{};
  ep.mode = kEpiResidual;
  ep.R = R;
  ep.rscale = rscale;
  ep.lens = reinterpret_cast<const int*>(lens);
  ep.T = (int)T;
  ep.p_drop = p_drop;
  ep.rng = rng;
  ep.rng_off = (uint64_t)rng_offset;
  ep.nln = nln;
  ep.lng[0] = ln_w0;
  ep.lnb[0] = ln_b0;
  ep.lneps[0] = eps0;
  ep.lny[0] = ln_y0;
  ep.lnmean[0] = ln_mean0;
  ep.lnrstd[0] = ln_rstd0;
  ep.lng[1] = ln_w1;
  ep.lnb[1] = ln_b1;
  ep.lneps[1] = eps1;
  ep.lny[1] = ln_y1;
  ep.lnmean[1] = ln_mean1;
  ep.lnrstd[1] = ln_rstd1;
  launch_ternary_gemm_passes(X, (int)P, M, K, codes2, pass_bits ? codes1 : codes2,
                             reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw, bias, Y,
                             as_stream(stream), &ep);
  return launched();
}

int ob_bitlinear_bwd_dx_swish_drop(const float* dY, int64_t P, int64_t M, int64_t N,
                                   const uint32_t* codes2_t, const uint32_t* codes1_t,
                                   const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                   int64_t K, const float* pre, float p_drop, const uint64_t* rng,
                                   int64_t rng_offset, float* dPre, void* stream) {
  if (int st = fused_gemm_check(dY, P, M, N, codes2_t, codes1_t, pass_bits, alpha, K, dPre, p_drop,
                                rng))
    return st;
  if (M * K > 0 && !pre) return OB_ERR_NULL;
  if (!aligned4(pre)) return OB_ERR_ALIGN;
  TgemmEpi ep{};
  ep.mode = kEpiSwishDropBwd;
  ep.R = pre;
  ep.p_drop = p_drop;
  ep.rng = rng;
  ep.rng_off = (uint64_t)rng_offset;
  launch_ternary_gemm_passes(dY, (int)P, M, N, codes2_t, pass_bits ? codes1_t : codes2_t,
                             reinterpret_cast<const int*>(pass_bits), K, alpha, alpha_raw, nullptr,
                             dPre, as_stream(stream), &ep);
  return launched();
}

int ob_drop_scale_bwd(const float* dOut, int64_t rows, int64_t N, float rscale, float p_drop,
                      const uint64_t* rng, int64_t rng_offset, const int32_t* lens, int64_t T,
                      float* dY, void* stream) {
  if (rows < 0 || N < 0 || !(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  if (lens && (T < 1 || T > 0x7fffffff || rows % T)) return OB_ERR_SHAPE;
  if ((rows * N > 0 && (!dOut || !dY)) || (p_drop > 0.0f && !rng)) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(dOut) & 15) || (reinterpret_cast<uintptr_t>(dY) & 15) ||
      !aligned4(lens))
    return OB_ERR_ALIGN;
  launch_drop_scale_bwd(dOut, rows, N, rscale, p_drop, rng, (uint64_t)rng_offset,
                        reinterpret_cast<const int*>(lens), (int)T, dY, as_stream(stream));
  return launched();
}

int ob_residual_drop_fwd(const float* R, const float* Y, int64_t rows, int64_t N, float rscale,
                         float p_drop, const uint64_t* rng, int64_t rng_offset,
                         const int32_t* lens, int64_t T, float* out, void* stream) {
  if (rows < 0 || N < 0 || !(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  if (lens && (T < 1 || T > 0x7fffffff || rows % T)) return OB_ERR_SHAPE;
  if ((rows * N > 0 && (!R || !Y || !out)) || (p_drop > 0.0f && !rng)) return OB_ERR_NULL;
  if (!aligned4(R) || !aligned4(Y) || !aligned4(out) || !aligned4(lens)) return OB_ERR_ALIGN;
  launch_residual_drop_fwd(R, Y, rows, N, rscale, p_drop, rng, (uint64_t)rng_offset,
                           reinterpret_cast<const int*>(lens), (int)T, out, as_stream(stream));
  return launched();
}

int ob_bias_relu_fwd(float* y, const float* bias, int64_t B, int64_t C, int64_t hw,
                     void* stream) {
  if (B < 0 || C < 0 || hw < 0) return OB_ERR_SHAPE;
  if (B * C * hw > 0 && (!y || !bias)) return OB_ERR_NULL;
  if (!aligned4(y) || !aligned4(bias)) return OB_ERR_ALIGN;
  if (hw % 4 == 0 && (reinterpret_cast<uintptr_t>(y) & 15)) return OB_ERR_ALIGN;
  launch_bias_relu_fwd(y, bias, B, C, hw, as_stream(stream));
  return launched();
}

size_t ob_relu_bias_bwd_workspace(int64_t B, int64_t C) {
  return (B < 0 || C < 0) ? 0 : relu_bias_bwd_workspace(B, C);
}

int ob_relu_bias_bwd(const float* g, const float* y, int64_t B, int64_t C, int64_t hw,
                     float* gout, float* dbias, void* ws, size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || hw < 0 || B * C > 0x7fffffff) return OB_ERR_SHAPE;
  if (B * C * hw > 0 && (!g || !y || !gout)) return OB_ERR_NULL;
  if (B * C > 0 && !ws) return OB_ERR_NULL;
  if (ws_bytes < relu_bias_bwd_workspace(B, C)) return OB_ERR_WORKSPACE;
  if (!aligned4(g) || !aligned4(y) || !aligned4(gout) || !aligned4(dbias)) return OB_ERR_ALIGN;
  launch_relu_bias_bwd(g, y, B, C, hw, gout, dbias, ws, as_stream(stream));
  return launched();
}

size_t ob_colsum_workspace(int64_t N) { return N < 0 ? 0 : colsum_workspace(N); }

int ob_colsum(const float* x, int64_t rows, int64_t N, float* out, void* ws, size_t ws_bytes,
              void* stream) {
  if (rows < 0 || N < 0 || N > 0x7fffffff) return OB_ERR_SHAPE;
  if (N > 0 && (!out || !ws || (rows > 0 && !x))) return OB_ERR_NULL;
  if (ws_bytes < colsum_workspace(N)) return OB_ERR_WORKSPACE;
  if (!aligned4(x) || !aligned4(out)) return OB_ERR_ALIGN;
  launch_colsum(x, rows, N, out, ws, as_stream(stream));
  return launched();
}

namespace {
inline bool aligned16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
}  // namespace

int ob_dense_supported(int64_t K, int64_t N) { return dense_gemm_supported(K, N) ? 1 : 0; }

int ob_silu_fast_monotone_check(uint32_t lo_bits, uint32_t hi_bits, uint32_t* bad, void* stream) {
  if (!bad) return OB_ERR_NULL;
  if (lo_bits > hi_bits || hi_bits >= 0x7F800000u) return OB_ERR_SHAPE;  // finite, >= +0
  launch_silu_monotone_check(lo_bits, hi_bits, bad, as_stream(stream));
  return launched();
}

int ob_dense_gemm(const float* X, int64_t M, int64_t K, const float* W, int w_trans,
                  const float* bias, int64_t N, float* Y, void* stream) {
  if (M < 0 || M > ((int64_t)1 << 40) || !dense_gemm_supported(K, N)) return OB_ERR_SHAPE;
  if (!W || (M > 0 && (!X || !Y))) return OB_ERR_NULL;
  if (!aligned16(X) || !aligned16(W) || !aligned16(Y) || !aligned4(bias)) return OB_ERR_ALIGN;
  if (!launch_dense_gemm(X, M, K, W, w_trans, bias, N, Y, as_stream(stream))) return OB_ERR_SHAPE;
  return launched();
}

int ob_dense_gemm_residual_drop(const float* X, int64_t M, int64_t K, const float* W,
                                const float* bias, int64_t N, const float* R, float p_drop,
                                const int64_t* rng, int64_t rng_offset, float* Y, void* stream) {
  if (M < 0 || M > ((int64_t)1 << 40) || !dense_gemm_supported(K, N)) return OB_ERR_SHAPE;
  if (!(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  if (!W || (M > 0 && (!X || !Y || !R)) || (p_drop > 0.0f && !rng)) return OB_ERR_NULL;
  if (!aligned16(X) || !aligned16(W) || !aligned16(Y) || !aligned4(bias) || !aligned4(R))
    return OB_ERR_ALIGN;
  const DenseEpi epi{R, p_drop, reinterpret_cast<const uint64_t*>(rng), (uint64_t)rng_offset};
  if (!launch_dense_gemm(X, M, K, W, 0, bias, N, Y, as_stream(stream), &epi)) return OB_ERR_SHAPE;
  return launched();
}

size_t ob_dense_dw_workspace(int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N <= 0 || K <= 0 || N % 4 != 0 || K % 4 != 0) return 0;
  const int v = plan_dw(M, N, K).variant;
  if (v != 4 && v < 9) return 0;  // the bf16x6 tiles (LDS: widths % 48; register: % 4)
  return dw_layout(1, M, N, K).total;
}

int ob_dense_dw(const float* dY, const float* X, int64_t M, int64_t N, int64_t K, float* dW,
                float* db, void* ws, size_t ws_bytes, void* stream) {
  return ob_dense_dw_defer(dY, X, M, N, K, dW, db, ws, ws_bytes, nullptr, 0, 0, nullptr, stream);
}

int ob_dense_dw_defer(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                      float* dW, float* db, void* ws, size_t ws_bytes, void* table, int64_t slot,
                      int64_t start, int64_t* n_blocks, void* stream) {
  if (n_blocks) *n_blocks = 0;
  if (table && (!n_blocks || slot < 0 || start < 0)) return OB_ERR_NULL;
  const size_t need = ob_dense_dw_workspace(M, N, K);
  if (need == 0) return OB_ERR_SHAPE;
  if (!dW || !ws || (M > 0 && (!dY || !X))) return OB_ERR_NULL;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  if (!aligned16(dY) || !aligned16(X) || !aligned4(dW) || !aligned4(db)) return OB_ERR_ALIGN;
  hipStream_t s = as_stream(stream);
  if (M == 0) {
    launch_zero_words(dW, N * K, s);
    if (db) launch_zero_words(db, N, s);
    return launched();
  }
  const DwWorkspace L = dw_layout(1, M, N, K);
  const DwPlan p = plan_dw(M, N, K);
  char* base = static_cast<char*>(ws);
  float* part = reinterpret_cast<float*>(base);
  float* part_db = db ? reinterpret_cast<float*>(base + L.part) : nullptr;
  const DwAlpha al{nullptr, nullptr, 0, 2, nullptr, nullptr, nullptr};  // no alpha: dense
  if (p.variant < 9) {  // register bf16x6 tiles (64-wide): the same chunk partials + finish
    uint32_t* ticket = reinterpret_cast<uint32_t*>(base + L.part + L.part_db);
    launch_dw_partial(dY, X, M, N, K, p, part, part_db, ticket, s);
    const DwFinish fin{part, (int)p.chunks, N * K, part_db, db ? N : 0, nullptr, nullptr, 0,
                       nullptr, 0, dW, db, nullptr};
    if (table) {
      // (no entry written by the register kernel: a 1-block launch writes it)
      const DwFinishEntry ent{fin, start};
      launch_dw_table_entry(static_cast<DwFinishEntry*>(table), (int)slot, ent, s);
      *n_blocks = dw_finish_blocks(fin);
      return launched();
    }
    launch_dw_finish(part, (int)p.chunks, N * K, part_db, db ? N : 0, nullptr, nullptr, 0,
                     nullptr, 0, dW, db, nullptr, s);
    return launched();
  }
  if (table) {  // finish deferred to ob_dw_finish_table
    const DwFinish fin{part, (int)p.chunks, N * K, part_db, db ? N : 0, nullptr, nullptr, 0,
                       nullptr, 0, dW, db, nullptr};
    const DwFinishEntry ent{fin, start};
    launch_dw_partial_group_defer(&dY, 1, X, M, N, K, p, &part, &part_db, &al,
                                  static_cast<DwFinishEntry*>(table), (int)slot, &ent, s);
    *n_blocks = dw_finish_blocks(fin);
    return launched();
  }
  launch_dw_partial(dY, X, M, N, K, p, part, part_db, nullptr, s, &al);
  launch_dw_finish(part, (int)p.chunks, N * K, part_db, db ? N : 0, nullptr, nullptr, 0, nullptr,
                   0, dW, db, nullptr, s);
  return launched();
}

namespace {
int subsample_check(int64_t B, int64_t T, int64_t F, int64_t C) {
  if (B < 1 || B > 65535 || T > (1 << 20) || F > (1 << 16)) return OB_ERR_SHAPE;
  if (B * ((T - 3) / 2 + 1) * ((F - 3) / 2 + 1) * C >= ((int64_t)1 << 30)) return OB_ERR_SHAPE;
  if (!subsample_supported(T, F, C)) return OB_ERR_SHAPE;
  return OB_OK;
}
}  // namespace

size_t ob_subsample_image_bytes(int64_t C) {
  return subsample_supported(7, 7, C) ? subsample_image_bytes(C) : 0;
}

int ob_subsample_pack(const float* W2, int64_t C, void* img, void* stream) {
  if (!subsample_supported(7, 7, C)) return OB_ERR_SHAPE;
  if (!W2 || !img) return OB_ERR_NULL;
  if (!aligned4(W2) || !aligned16(img)) return OB_ERR_ALIGN;
  launch_subsample_pack(W2, C, img, as_stream(stream));
  return launched();
}

int ob_subsample_fwd(const float* X, int64_t B, int64_t T, int64_t F, int64_t C,
                     const float* W0, const float* b0, const void* img, const float* b2,
                     float* Y1, float* Y2, void* stream) {
  if (const int st = subsample_check(B, T, F, C)) return st;
  if (!X || !W0 || !b0 || !img || !b2 || !Y1 || !Y2) return OB_ERR_NULL;
  if (!aligned4(X) || !aligned4(W0) || !aligned4(b0) || !aligned4(b2) || !aligned16(img) ||
      !aligned16(Y1) || !aligned16(Y2))
    return OB_ERR_ALIGN;
  launch_subsample_fwd(X, B, T, F, C, W0, b0, img, b2, Y1, Y2, as_stream(stream));
  return launched();
}

size_t ob_subsample_bwd_workspace(int64_t B, int64_t T, int64_t F, int64_t C) {
  return subsample_check(B, T, F, C) ? 0 : subsample_bwd_workspace(B, T, F, C);
}

int ob_subsample_bwd(const float* X, const float* W0, const float* b0, const float* Y1,
                     const float* Y2, const float* dY2, int64_t B, int64_t T, int64_t F, int64_t C,
                     const void* img, float* dW0,
                     float* db0, float* dW2, float* db2, void* ws, size_t ws_bytes,
                     void* stream) {
  if (const int st = subsample_check(B, T, F, C)) return st;
  if (!X || !W0 || !b0 || !Y1 || !Y2 || !dY2 || !img || !dW0 || !db0 || !dW2 || !db2 || !ws)
    return OB_ERR_NULL;
  if (ws_bytes < subsample_bwd_workspace(B, T, F, C)) return OB_ERR_WORKSPACE;
  if (!aligned4(X) || !aligned4(W0) || !aligned4(b0) || !aligned16(Y1) || !aligned16(Y2) ||
      !aligned16(dY2) || !aligned16(img) ||
      !aligned16(ws) || !aligned4(dW0) || !aligned4(db0) || !aligned4(dW2) || !aligned4(db2))
    return OB_ERR_ALIGN;
  if (B * ((T - 3) / 2 + 1) * ((F - 3) / 2 + 1) * C * 4 >= ((int64_t)1 << 31)) return OB_ERR_SHAPE;
  launch_subsample_bwd(X, W0, b0, Y1, Y2, dY2, B, T, F, C, img, dW0, db0, dW2, db2, ws,
                       as_stream(stream));
  return launched();
}

namespace {
int convmod_check(int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K) {
  if (P < 1 || Bt < 0 || T < 0 || C < 1 || K < 1 || Bt % P || Bt > 65535) return OB_ERR_SHAPE;
  if (!convmod_supported(C, K) || Bt * T * 2 * C > ((int64_t)1 << 40)) return OB_ERR_SHAPE;
  if (!convmod_addressable(T, C, K)) return OB_ERR_SHAPE;
  return OB_OK;
}
}  // namespace

size_t ob_convmod_workspace(int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K) {
  if (convmod_check(P, Bt, T, C, K)) return 0;
  return convmod_workspace(P, Bt, T, C, K);
}

int ob_convmod_fwd(const float* u, const float* w_dw, const float* b_dw, const float* gamma,
                   const float* beta, int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K,
                   float eps, float* z, float* g, float* stats, float* v, void* ws,
                   size_t ws_bytes, void* stream) {
  if (int st = convmod_check(P, Bt, T, C, K)) return st;
  if (Bt * T == 0) return OB_OK;
  if (!u || !w_dw || !gamma || !beta || !z || !g || !stats || !v || !ws) return OB_ERR_NULL;
  if (ws_bytes < convmod_workspace(P, Bt, T, C, K)) return OB_ERR_WORKSPACE;
  if (((uintptr_t)ws & 7u) || !aligned4(u) || !aligned4(z) || !aligned4(v) || !aligned4(stats) ||
      !aligned4(w_dw) || !aligned4(b_dw))
    return OB_ERR_ALIGN;
  if (!aligned4(g)) return OB_ERR_ALIGN;
  launch_convmod_fwd(u, w_dw, b_dw, gamma, beta, P, Bt, T, C, K, eps, z, g, stats, v, ws,
                     as_stream(stream));
  return launched();
}

int ob_convmod_bwd(const float* dv, const float* u, const float* z, const float* g,
                   const float* stats, const float* w_dw, const float* gamma, const float* beta,
                   int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K, float* du,
                   float* dw_dw, float* db_dw, float* dgamma, float* dbeta, void* ws,
                   size_t ws_bytes, void* stream) {
  if (int st = convmod_check(P, Bt, T, C, K)) return st;
  if (!dw_dw || !dgamma || !dbeta || !w_dw || !gamma || !beta) return OB_ERR_NULL;
  if (Bt * T > 0 && (!dv || !u || !z || !g || !stats || !du || !ws)) return OB_ERR_NULL;
  if (ws_bytes < convmod_workspace(P, Bt, T, C, K)) return OB_ERR_WORKSPACE;
  if (((uintptr_t)ws & 7u) || !aligned4(dv) || !aligned4(u) || !aligned4(z) || !aligned4(g) ||
      !aligned4(du))
    return OB_ERR_ALIGN;
  launch_convmod_bwd(dv, u, z, g, stats, w_dw, gamma, beta, P, Bt, T, C, K, du, dw_dw, db_dw,
                     dgamma, dbeta, ws, as_stream(stream));
  return launched();
}

int ob_convmod_bwd_defer(const float* dv, const float* u, const float* z, const float* g,
                         const float* stats, const float* w_dw, const float* gamma,
                         const float* beta, int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K,
                         float* du, float* dw_dw, float* db_dw, float* dgamma, float* dbeta,
                         void* ws, size_t ws_bytes, void* table, int64_t slot, int64_t* deferred,
                         void* stream) {
  if (int st = convmod_check(P, Bt, T, C, K)) return st;
  if (!dw_dw || !dgamma || !dbeta || !w_dw || !gamma || !beta) return OB_ERR_NULL;
  if (Bt * T > 0 && (!dv || !u || !z || !g || !stats || !du || !ws)) return OB_ERR_NULL;
  if (ws_bytes < convmod_workspace(P, Bt, T, C, K)) return OB_ERR_WORKSPACE;
  if (((uintptr_t)ws & 7u) || !aligned4(dv) || !aligned4(u) || !aligned4(z) || !aligned4(g) ||
      !aligned4(du))
    return OB_ERR_ALIGN;
  if (slot < 0) return OB_ERR_SHAPE;
  // (one frame per pass: launch_convmod_bwd writes the exact zeros itself, nothing to defer)
  const bool dfr = table && Bt * T > 0 && Bt / P * T != 1 && convmod_bwd_deferrable(C, K);
  const CmDefer df{dfr ? static_cast<CmWgradEntry*>(table) : nullptr, (int)slot};
  launch_convmod_bwd(dv, u, z, g, stats, w_dw, gamma, beta, P, Bt, T, C, K, du, dw_dw, db_dw,
                     dgamma, dbeta, ws, as_stream(stream), &df);
  if (deferred) *deferred = dfr ? 1 : 0;
  return launched();
}

size_t ob_cm_wgrad_entry_bytes(void) { return sizeof(CmWgradEntry); }

int ob_cm_wgrad_table(const void* table, int64_t n, int64_t nmax, void* stream) {
  if (n < 0 || nmax < 0 || nmax > (1 << 24)) return OB_ERR_SHAPE;
  if (n > 0 && !table) return OB_ERR_NULL;
  launch_cm_wgrad_table(static_cast<const CmWgradEntry*>(table), (int)n, (int)nmax,
                        as_stream(stream));
  return launched();
}

size_t ob_act_absmax_workspace(int64_t P) {
  return (P < 1 || P > 65535) ? 0 : act_absmax_workspace((int)P);
}

int ob_act_absmax(const float* X, int64_t P, int64_t n_per_pass, float* amax, void* ws,
                  size_t ws_bytes, void* stream) {
  if (P < 1 || P > 65535 || n_per_pass < 0) return OB_ERR_SHAPE;
  if (!amax || !ws || (n_per_pass > 0 && !X)) return OB_ERR_NULL;
  if (ws_bytes < act_absmax_workspace((int)P)) return OB_ERR_WORKSPACE;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (n_per_pass % 4) || !aligned4(amax) ||
      !aligned4(ws))
    return OB_ERR_ALIGN;
  launch_act_absmax(X, (int)P, n_per_pass, amax, ws, as_stream(stream));
  return launched();
}

int ob_act_dequant_i8(const float* X, int64_t P, int64_t n_per_pass, const float* amax,
                      float* X_deq, void* stream) {
  if (P < 1 || P > 65535 || n_per_pass < 0) return OB_ERR_SHAPE;
  if (!amax || (n_per_pass > 0 && (!X || !X_deq))) return OB_ERR_NULL;
  if (!aligned4(X) || !aligned4(X_deq) || !aligned4(amax)) return OB_ERR_ALIGN;
  launch_act_dequant(X, (int)P, n_per_pass, amax, X_deq, as_stream(stream));
  return launched();
}

int ob_bitlinear_fwd_i8(const float* X, int64_t P, int64_t M, int64_t K, const uint32_t* codes,
                        const uint32_t* codes1, const int32_t* pass_bits, const float* alpha,
                        int alpha_raw, const float* amax, const float* bias, int64_t N, float* Y,
                        void* stream) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (P > 1 && !pass_bits) return OB_ERR_NULL;
  if (!alpha || !amax || (M * N > 0 && !Y) || (M * K > 0 && !X) || (N * K > 0 && !codes) ||
      (pass_bits && N * K > 0 && !codes1))
    return OB_ERR_NULL;
  if (M * N > 0 && !ternary_gemm_i8_supported(K, N)) return OB_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || !aligned4(Y) || !aligned4(bias) ||
      !aligned4(amax) || !aligned4(pass_bits))
    return OB_ERR_ALIGN;
  if (!launch_ternary_gemm_i8(X, (int)P, M, K, codes, pass_bits ? codes1 : codes,
                              reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw, amax,
                              bias, Y, as_stream(stream)))
    return OB_ERR_SHAPE;
  return launched();
}

int ob_bitlinear_fwd_i8_epi(const float* X, int64_t P, int64_t M, int64_t K,
                            const uint32_t* codes, const uint32_t* codes1,
                            const int32_t* pass_bits, const float* alpha, int alpha_raw,
                            const float* amax, const float* bias, int64_t N, int mode,
                            const float* R, float rscale, const int32_t* lens, int64_t T,
                            float* amax_out, float* Y, void* stream) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535 || (mode != 1 && mode != 2) || N % 4)
    return OB_ERR_SHAPE;
  if (P > 1 && !pass_bits) return OB_ERR_NULL;
  if (!alpha || !amax || (M * N > 0 && !Y) || (M * K > 0 && !X) || (N * K > 0 && !codes) ||
      (pass_bits && N * K > 0 && !codes1) || (mode == 1 && !amax_out) ||
      (mode == 2 && M * N > 0 && !R) || (lens && T < 1))
    return OB_ERR_NULL;
  if (M * N > 0 && !ternary_gemm_i8_supported(K, N)) return OB_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(X) & 15) || (reinterpret_cast<uintptr_t>(Y) & 15) ||
      (reinterpret_cast<uintptr_t>(R) & 15) || !aligned4(bias) || !aligned4(amax) ||
      !aligned4(pass_bits) || !aligned4(amax_out) || !aligned4(lens))
    return OB_ERR_ALIGN;
  if (!launch_ternary_gemm_i8_epi(X, (int)P, M, K, codes, pass_bits ? codes1 : codes,
                                  reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw,
                                  amax, bias, Y, mode, R, rscale,
                                  reinterpret_cast<const int*>(lens), T, amax_out,
                                  as_stream(stream)))
    return OB_ERR_SHAPE;
  return launched();
}

int ob_bitlinear_fwd_i8q(const int8_t* Xq, int64_t P, int64_t M, int64_t K,
                         const uint32_t* codes, const uint32_t* codes1, const int32_t* pass_bits,
                         const float* alpha, int alpha_raw, const float* amax, const float* bias,
                         int64_t N, int mode, const float* R, float rscale, const int32_t* lens,
                         int64_t T, float* amax_out, void* Y, void* stream) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535 || (mode != 0 && mode != 2 && mode != 3) ||
      N % 4 || (mode == 3 && N % 16))
    return OB_ERR_SHAPE;
  if (P > 1 && !pass_bits) return OB_ERR_NULL;
  if (!alpha || !amax || (M * N > 0 && !Y) || (M * K > 0 && !Xq) || (N * K > 0 && !codes) ||
      (pass_bits && N * K > 0 && !codes1) || (mode == 3 && !amax_out) ||
      (mode == 2 && M * N > 0 && !R) || (lens && T < 1))
    return OB_ERR_NULL;
  if (M * N > 0 && !ternary_gemm_i8_supported(K, N)) return OB_ERR_SHAPE;
  if ((reinterpret_cast<uintptr_t>(Xq) & 15) || (reinterpret_cast<uintptr_t>(Y) & 15) ||
      (reinterpret_cast<uintptr_t>(R) & 15) || !aligned4(bias) || !aligned4(amax) ||
      !aligned4(pass_bits) || !aligned4(amax_out) || !aligned4(lens))
    return OB_ERR_ALIGN;
  if (!launch_ternary_gemm_i8q(Xq, (int)P, M, K, codes, pass_bits ? codes1 : codes,
                               reinterpret_cast<const int*>(pass_bits), N, alpha, alpha_raw, amax,
                               bias, Y, mode, R, rscale, reinterpret_cast<const int*>(lens), T,
                               amax_out, as_stream(stream)))
    return OB_ERR_SHAPE;
  return launched();
}

int ob_bitlinear_bwd_dx_passes(const float* dY, int64_t P, int64_t M, int64_t N,
                               const uint32_t* codes2_t, const uint32_t* codes1_t,
                               const int32_t* pass_bits, const float* alpha, int alpha_raw,
                               int64_t K, float* dX, void* stream) {
  if (M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (!alpha || !pass_bits || (M * K > 0 && !dX) || (M * N > 0 && !dY) ||
      (N * K > 0 && (!codes2_t || !codes1_t)))
    return OB_ERR_NULL;
  if (!aligned4(dY) || !aligned4(dX) || !aligned4(pass_bits)) return OB_ERR_ALIGN;
  launch_ternary_gemm_passes(dY, (int)P, M, N, codes2_t, codes1_t,
                             reinterpret_cast<const int*>(pass_bits), K, alpha, alpha_raw, nullptr,
                             dX, as_stream(stream));
  return launched();
}

int ob_bitlinear_bwd_dx_passes_sum(int64_t G, const float* const* dY, int64_t P, int64_t M,
                                   int64_t N, const uint32_t* const* codes2_t,
                                   const uint32_t* const* codes1_t, const int32_t* pass_bits,
                                   const float* const* alpha, int alpha_raw, int64_t K, float* dX,
                                   void* stream) {
  if (G < 1 || G > 3 || M < 0 || K < 0 || N < 0 || P < 1 || P > 65535) return OB_ERR_SHAPE;
  if (!dY || !codes2_t || !codes1_t || !alpha || !pass_bits || !dX) return OB_ERR_NULL;
  for (int64_t i = 0; i < G; ++i)
    if (!dY[i] || !codes2_t[i] || !codes1_t[i] || !alpha[i]) return OB_ERR_NULL;
  if (!aligned4(pass_bits)) return OB_ERR_ALIGN;
  if (!launch_ternary_dx_sum((int)G, dY, (int)P, M, N, codes2_t, codes1_t,
                             reinterpret_cast<const int*>(pass_bits), alpha, alpha_raw, K, dX,
                             as_stream(stream)))
    return OB_ERR_SHAPE;  // not this kernel's shape: one ob_bitlinear_bwd_dx_passes per source
  return launched();
}

size_t ob_bitlinear_bwd_dw_passes_workspace(int64_t P, int64_t M, int64_t N, int64_t K) {
  if (M < 0 || N < 0 || K < 0 || P < 1 || P > kMaxPasses) return 0;
  return dw_layout(P, M, N, K).total;
}

int ob_bitlinear_bwd_dw_passes(const float* dY, const float* X, int64_t P, int64_t M, int64_t N,
                               int64_t K, const float* W, const float* alpha, int alpha_raw,
                               const int32_t* pass_bits, float* dW, float* dalpha, float* db,
                               void* ws, size_t ws_bytes, void* stream) {
  if (!pass_bits) return OB_ERR_NULL;
  return bwd_dw_impl(dY, X, P, M, N, K, W, alpha, alpha_raw, 2, nullptr, pass_bits, dW, dalpha,
                     db, ws, ws_bytes, stream);
}

size_t ob_bitlinear_bwd_dw_passes_group_workspace(int64_t G, int64_t P, int64_t M, int64_t N,
                                                  int64_t K) {
  if (G < 1 || G > kMaxDwGroup) return 0;
  const size_t one = ob_bitlinear_bwd_dw_passes_workspace(P, M, N, K);
  if (!one) return 0;
  return (size_t)G * std::max(align_up(one), dw_layout(P, M, N, K, G).total);
}

namespace {
int dw_group_impl(int64_t G, const float* const* dY, const float* X, int64_t P, int64_t M,
                  int64_t N, int64_t K, const float* const* W, const float* const* alpha,
                  int alpha_raw, const int32_t* pass_bits, float* const* dW,
                  float* const* dalpha, float* const* db, void* ws, size_t ws_bytes,
                  void* stream, DwFinishEntry* table, int slot, int64_t start,
                  int64_t* n_blocks);
}  // namespace

int ob_bitlinear_bwd_dw_passes_group(int64_t G, const float* const* dY, const float* X,
                                     int64_t P, int64_t M, int64_t N, int64_t K,
                                     const float* const* W, const float* const* alpha,
                                     int alpha_raw, const int32_t* pass_bits, float* const* dW,
                                     float* const* dalpha, float* const* db, void* ws,
                                     size_t ws_bytes, void* stream) {
  return dw_group_impl(G, dY, X, P, M, N, K, W, alpha, alpha_raw, pass_bits, dW, dalpha, db, ws,
                       ws_bytes, stream, nullptr, 0, 0, nullptr);
}

int ob_bitlinear_bwd_dw_passes_group_defer(int64_t G, const float* const* dY, const float* X,
                                           int64_t P, int64_t M, int64_t N, int64_t K,
                                           const float* const* W, const float* const* alpha,
                                           int alpha_raw, const int32_t* pass_bits,
                                           float* const* dW, float* const* dalpha,
                                           float* const* db, void* ws, size_t ws_bytes,
                                           void* table, int64_t slot, int64_t start,
                                           int64_t* n_blocks, void* stream) {
  if (!table || !n_blocks || slot < 0 || start < 0) return OB_ERR_NULL;
  return dw_group_impl(G, dY, X, P, M, N, K, W, alpha, alpha_raw, pass_bits, dW, dalpha, db, ws,
                       ws_bytes, stream, static_cast<DwFinishEntry*>(table), (int)slot, start,
                       n_blocks);
}

namespace {
int dw_group_impl(int64_t G, const float* const* dY, const float* X, int64_t P, int64_t M,
                  int64_t N, int64_t K, const float* const* W, const float* const* alpha,
                  int alpha_raw, const int32_t* pass_bits, float* const* dW,
                  float* const* dalpha, float* const* db, void* ws, size_t ws_bytes,
                  void* stream, DwFinishEntry* table, int slot, int64_t start,
                  int64_t* n_blocks) {
  if (n_blocks) *n_blocks = 0;
  if (G < 1 || G > kMaxDwGroup) return OB_ERR_SHAPE;
  if (!dY || !W || !alpha || !dW || !dalpha || !db || !pass_bits || !ws) return OB_ERR_NULL;
  const size_t need = ob_bitlinear_bwd_dw_passes_group_workspace(G, P, M, N, K);
  if (need == 0) return OB_ERR_SHAPE;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  const size_t one = need / (size_t)G;
  const DwPlan pg = plan_dw_passes(P, M, G * N, K);
  if (pg.variant >= 9 && M > 0 && N > 0 && K > 0 && P <= kMaxPasses) {
    // one partial launch for the G layers (they share X), then one grouped finish
    for (int64_t i = 0; i < G; ++i)
      if (!dY[i] || !W[i] || !alpha[i] || !dW[i] || !dalpha[i]) return OB_ERR_NULL;
    if (!X) return OB_ERR_NULL;
    if (!aligned4(X) || !aligned4(pass_bits)) return OB_ERR_ALIGN;
    const DwWorkspace Lg = dw_layout(P, M, N, K, G);
    float* part[kMaxDwGroup];
    float* part_db[kMaxDwGroup];
    DwAlpha al[kMaxDwGroup];
    DwFinish fin[kMaxDwGroup];
    for (int64_t i = 0; i < G; ++i) {
      if (!aligned4(dY[i]) || !aligned4(dW[i]) || !aligned4(db[i])) return OB_ERR_ALIGN;
      char* base = static_cast<char*>(ws) + i * one;
      part[i] = reinterpret_cast<float*>(base);
      part_db[i] = db[i] ? reinterpret_cast<float*>(base + Lg.part) : nullptr;
      float* apart = reinterpret_cast<float*>(base + Lg.part + Lg.part_db + 16);
      al[i] = DwAlpha{W[i], alpha[i], alpha_raw, 2, nullptr,
                      reinterpret_cast<const int*>(pass_bits), apart};
      fin[i] = DwFinish{part[i], (int)pg.chunks, N * K, part_db[i], db[i] ? N : 0, W[i],
                        alpha[i], alpha_raw, apart, (int)(pg.tiles_n / G * pg.tiles_k * pg.chunks),
                        dW[i], db[i], dalpha[i]};
    }
    hipStream_t s = as_stream(stream);
    if (table) {  // finishes deferred to ob_dw_finish_table
      DwFinishEntry ent[kMaxDwGroup];
      int64_t at = start;
      for (int64_t i = 0; i < G; ++i) {
        ent[i] = DwFinishEntry{fin[i], at};
        at += dw_finish_blocks(fin[i]);
      }
      launch_dw_partial_group_defer(dY, (int)G, X, P * M, N, K, pg, part, part_db, al, table,
                                    slot, ent, s);
      *n_blocks = at - start;
      return launched();
    }
    launch_dw_partial_group(dY, (int)G, X, P * M, N, K, pg, part, part_db, al, s);
    launch_dw_finish_group(fin, (int)G, s);
    return launched();
  }
  DwFinish fin[kMaxDwGroup];
  bool deferred[kMaxDwGroup] = {false, false, false};
  for (int64_t i = 0; i < G; ++i) {
    fin[i].part = nullptr;
    const int st = bwd_dw_impl(dY[i], X, P, M, N, K, W[i], alpha[i], alpha_raw, 2, nullptr,
                               pass_bits, dW[i], dalpha[i], db[i],
                               static_cast<char*>(ws) + i * one, one, stream, &fin[i]);
    if (st != OB_OK) return st;
    deferred[i] = fin[i].part != nullptr;
  }
  // the LDS path deferred its finish (every layer, at one shape); others finished already
  int nd = 0;
  DwFinish grp[kMaxDwGroup];
  for (int64_t i = 0; i < G; ++i)
    if (deferred[i]) grp[nd++] = fin[i];
  if (nd) launch_dw_finish_group(grp, nd, as_stream(stream));
  return launched();
}
}  // namespace

int ob_bitlinear_bwd_dw_passes_defer(const float* dY, const float* X, int64_t P, int64_t M,
                                     int64_t N, int64_t K, const float* W, const float* alpha,
                                     int alpha_raw, const int32_t* pass_bits, float* dW,
                                     float* dalpha, float* db, void* ws, size_t ws_bytes,
                                     void* table, int64_t slot, int64_t start, int64_t* n_blocks,
                                     void* stream) {
  if (!pass_bits || !table || !n_blocks || slot < 0 || start < 0) return OB_ERR_NULL;
  return bwd_dw_impl(dY, X, P, M, N, K, W, alpha, alpha_raw, 2, nullptr, pass_bits, dW, dalpha,
                     db, ws, ws_bytes, stream, nullptr, static_cast<DwFinishEntry*>(table),
                     (int)slot, start, n_blocks);
}

size_t ob_dw_finish_entry_bytes(void) { return sizeof(DwFinishEntry); }

int ob_dw_finish_table(const void* table, int64_t n, int64_t total_blocks, void* stream) {
  if (n < 0 || total_blocks < 0 || total_blocks > 0x7fffffff) return OB_ERR_SHAPE;
  if (n > 0 && !table) return OB_ERR_NULL;
  launch_dw_finish_table(static_cast<const DwFinishEntry*>(table), (int)n, total_blocks,
                         as_stream(stream));
  return launched();
}

int ob_dw_grouped_supported(int64_t N, int64_t K) {
  return N > 0 && K > 0 && N % kDwgTile == 0 && K % kDwgTile == 0 && N <= (1 << 20) &&
         K <= (1 << 20);
}

namespace {
struct DwgPlan {
  std::vector<DwgDesc> d;
  int64_t steps = 0;
  int tiles = 0, blocks = 0;
  size_t table = 0, slots = 0, talpha = 0, total = 0;
};

// validates the descriptors and lays out the linear work space (gemm-major, tile, pass, step)
int dwg_plan(const ob_dwg_gemm* g, int64_t G, DwgPlan& pl) {
  if (G < 1 || G > (1 << 16)) return OB_ERR_SHAPE;
  if (!g) return OB_ERR_NULL;
  pl.d.resize((size_t)G);
  int64_t tiles = 0;
  for (int64_t i = 0; i < G; ++i) {
    const ob_dwg_gemm& e = g[i];
    // 32-bit offsets in the kernel: one pass of an operand, the weight, the step count
    if (!ob_dw_grouped_supported(e.N, e.K) || e.M < 1 || e.P < 1 || e.P > kMaxPasses ||
        e.M * e.P >= ((int64_t)1 << 30) || e.M * std::max(e.N, e.K) * 4 >= ((int64_t)1 << 31) ||
        e.N * e.K * 4 >= ((int64_t)1 << 31))
      return OB_ERR_SHAPE;
    if (!e.dY || !e.X || !e.dW) return OB_ERR_NULL;
    if (e.W && (!e.alpha || !e.dalpha)) return OB_ERR_NULL;
    if (e.W && !e.pass_bits && check_bits(e.bits) != OB_OK) return OB_ERR_BITWIDTH;
    if (!aligned4(e.dY) || !aligned4(e.X) || ((reinterpret_cast<uintptr_t>(e.dY) |
                                               reinterpret_cast<uintptr_t>(e.X)) & 15))
      return OB_ERR_ALIGN;
    DwgDesc& d = pl.d[(size_t)i];
    d.dY = e.dY;
    d.X = e.X;
    d.W = e.W;
    d.alpha = e.alpha;
    d.pass_bits = e.pass_bits;
    d.dW = e.dW;
    d.db = e.db;
    d.dalpha = e.dalpha;
    d.N = (int)e.N;
    d.K = (int)e.K;
    d.Mp = (int)e.M;
    d.P = (int)e.P;
    d.alpha_raw = e.alpha_raw;
    d.bits = e.bits;
    d.spp = (int)ceil_div(e.M, 32);
    d.tiles_k = (int)(e.K / kDwgTile);
    d.tiles = (int)((e.N / kDwgTile) * d.tiles_k);
    d.tile0 = (int)tiles;
    d.work0 = pl.steps;
    tiles += d.tiles;
    pl.steps += (int64_t)d.tiles * d.P * d.spp;
  }
  if (tiles > (1 << 24) || pl.steps >= ((int64_t)1 << 31)) return OB_ERR_SHAPE;
  pl.tiles = (int)tiles;
  pl.blocks = dwg_blocks(pl.steps);
  pl.table = align_up(sizeof(DwgDesc) * (size_t)G);
  pl.slots = align_up(dwg_slot_bytes() * 2 * (size_t)pl.blocks);
  pl.talpha = align_up(sizeof(float) * (size_t)tiles);
  pl.total = pl.table + pl.slots + pl.talpha;
  return OB_OK;
}
}  // namespace

size_t ob_dw_grouped_workspace(const ob_dwg_gemm* gemms, int64_t G) {
  DwgPlan pl;
  return dwg_plan(gemms, G, pl) == OB_OK ? pl.total : 0;
}

size_t ob_dw_grouped_tickets(const ob_dwg_gemm* gemms, int64_t G) {
  DwgPlan pl;
  return dwg_plan(gemms, G, pl) == OB_OK ? (size_t)pl.tiles + (size_t)G : 0;
}

int ob_dw_grouped(const ob_dwg_gemm* gemms, int64_t G, void* ws, size_t ws_bytes, void* tickets,
                  size_t ticket_words, void* stream) {
  DwgPlan pl;
  const int st = dwg_plan(gemms, G, pl);
  if (st != OB_OK) return st;
  if (!ws || !tickets) return OB_ERR_NULL;
  if (ws_bytes < pl.total || ticket_words < (size_t)pl.tiles + (size_t)G) return OB_ERR_WORKSPACE;
  unsigned char* base = static_cast<unsigned char*>(ws);
  launch_dw_grouped(pl.d.data(), (int)G, pl.steps, pl.blocks, reinterpret_cast<DwgDesc*>(base),
                    reinterpret_cast<float*>(base + pl.table),
                    reinterpret_cast<float*>(base + pl.table + pl.slots),
                    static_cast<uint32_t*>(tickets), pl.tiles, as_stream(stream));
  return launched();
}

int ob_dwconv1d_fwd(const float* x, const float* w, const float* bias, int64_t B, int64_t C,
                    int64_t T, int64_t KT, float* y, void* stream) {
  if (B < 0 || C < 0 || T < 0 || KT < 1 || KT % 2 == 0 || !dwconv_supported((int)KT))
    return OB_ERR_SHAPE;
  if (B * C * T > 0 && (!x || !y || !w)) return OB_ERR_NULL;
  if (!aligned4(x) || !aligned4(y) || !aligned4(w) || !aligned4(bias)) return OB_ERR_ALIGN;
  launch_dwconv_fwd(x, w, bias, B, C, T, KT, y, as_stream(stream));
  return launched();
}

size_t ob_dwconv1d_bwd_workspace(int64_t B, int64_t C, int64_t KT) {
  if (B < 0 || C < 0 || KT < 1) return 0;
  return align_up(dwconv_bwd_workspace(B, C, KT));
}

int ob_dwconv1d_bwd(const float* x, const float* dy, const float* w, int64_t B, int64_t C,
                    int64_t T, int64_t KT, float* dx, float* dw, float* db, void* ws,
                    size_t ws_bytes, void* stream) {
  if (B < 0 || C < 0 || T < 0 || KT < 1 || KT % 2 == 0 || !dwconv_supported((int)KT))
    return OB_ERR_SHAPE;
  if (!dw || !w || !ws || (B * C * T > 0 && (!x || !dy))) return OB_ERR_NULL;
  if (!aligned4(x) || !aligned4(dy) || !aligned4(dx) || !aligned4(dw) || !aligned4(db))
    return OB_ERR_ALIGN;
  if (ws_bytes < ob_dwconv1d_bwd_workspace(B, C, KT)) return OB_ERR_WORKSPACE;
  launch_dwconv_bwd(x, dy, w, B, C, T, KT, dx, dw, db, static_cast<float*>(ws),
                    as_stream(stream));
  return launched();
}

size_t ob_ctc_loss_workspace(int64_t B, int64_t T, int64_t S) {
  if (B < 0 || T < 0 || S < 0) return 0;
  return align_up(ctc_workspace(B, T, S));
}

int ob_ctc_loss_fwd(const float* log_probs, const int64_t* targets, const int64_t* input_lengths,
                    const int64_t* target_lengths, int64_t B, int64_t T, int64_t V, int64_t S,
                    int blank, float* loss, void* ws, size_t ws_bytes, void* stream) {
  if (B < 1 || T < 0 || V < 1 || S < 0 || blank < 0 || blank >= V || !ctc_supported(S))
    return OB_ERR_SHAPE;
  if (!log_probs || !input_lengths || !target_lengths || !loss || !ws || (S > 0 && !targets))
    return OB_ERR_NULL;
  if (ws_bytes < ob_ctc_loss_workspace(B, T, S)) return OB_ERR_WORKSPACE;
  launch_ctc_fwd(log_probs, targets, input_lengths, target_lengths, B, T, V, S, blank, 1, loss,
                 static_cast<float*>(ws), as_stream(stream));
  return launched();
}

int ob_ctc_loss_fwd_groups(const float* log_probs, const int64_t* targets,
                           const int64_t* input_lengths, const int64_t* target_lengths, int64_t G,
                           int64_t B, int64_t T, int64_t V, int64_t S, int blank, float* loss,
                           void* ws, size_t ws_bytes, void* stream) {
  if (G < 1 || G > 64 || B < 1 || B % G || T < 0 || V < 1 || S < 0 || blank < 0 || blank >= V ||
      !ctc_supported(S))
    return OB_ERR_SHAPE;
  if (!log_probs || !input_lengths || !target_lengths || !loss || !ws || (S > 0 && !targets))
    return OB_ERR_NULL;
  if (ws_bytes < ob_ctc_loss_workspace(B, T, S)) return OB_ERR_WORKSPACE;
  launch_ctc_fwd(log_probs, targets, input_lengths, target_lengths, B, T, V, S, blank, G, loss,
                 static_cast<float*>(ws), as_stream(stream));
  return launched();
}

int ob_ctc_loss_bwd(const float* log_probs, const int64_t* targets, const int64_t* input_lengths,
                    const int64_t* target_lengths, int64_t B, int64_t T, int64_t V, int64_t S,
                    int blank, const float* grad_out, float* grad, void* ws, size_t ws_bytes,
                    void* stream) {
  if (B < 1 || T < 0 || V < 1 || S < 0 || blank < 0 || blank >= V || !ctc_supported(S))
    return OB_ERR_SHAPE;
  if (!log_probs || !input_lengths || !target_lengths || !grad || !ws || (S > 0 && !targets))
    return OB_ERR_NULL;
  if (ws_bytes < ob_ctc_loss_workspace(B, T, S)) return OB_ERR_WORKSPACE;
  launch_ctc_bwd(log_probs, targets, input_lengths, target_lengths, B, T, V, S, blank, 1,
                 grad_out, grad, static_cast<float*>(ws), as_stream(stream));
  return launched();
}

int ob_ctc_loss_bwd_groups(const float* log_probs, const int64_t* targets,
                           const int64_t* input_lengths, const int64_t* target_lengths, int64_t G,
                           int64_t B, int64_t T, int64_t V, int64_t S, int blank,
                           const float* grad_out, float* grad, void* ws, size_t ws_bytes,
                           void* stream) {
  if (G < 1 || G > 64 || B < 1 || B % G || T < 0 || V < 1 || S < 0 || blank < 0 || blank >= V ||
      !ctc_supported(S))
    return OB_ERR_SHAPE;
  if (!log_probs || !input_lengths || !target_lengths || !grad || !ws || (S > 0 && !targets))
    return OB_ERR_NULL;
  if (ws_bytes < ob_ctc_loss_workspace(B, T, S)) return OB_ERR_WORKSPACE;
  launch_ctc_bwd(log_probs, targets, input_lengths, target_lengths, B, T, V, S, blank, G,
                 grad_out, grad, static_cast<float*>(ws), as_stream(stream));
  return launched();
}

size_t ob_ctc_logits_workspace(int64_t B, int64_t T, int64_t S) {
  if (B < 0 || T < 0 || S < 0) return 0;
  return align_up(ctc_logits_workspace_bytes(B, T, S));
}

namespace {
int ctc_logits_check(const float* x, const int64_t* targets, const int64_t* input_lengths,
                     const int64_t* target_lengths, int64_t G, int64_t B, int64_t T, int64_t V,
                     int64_t S, int blank, const void* out, void* ws, size_t ws_bytes) {
  if (G < 1 || G > 64 || B < 1 || B % G || T < 0 || V < 1 || V > INT32_MAX || S < 0 ||
      blank < 0 || blank >= V || !ctc_supported(S) || B * T > INT32_MAX)
    return OB_ERR_SHAPE;
  if (!x || !input_lengths || !target_lengths || !out || !ws || (S > 0 && !targets))
    return OB_ERR_NULL;
  if (ws_bytes < ob_ctc_logits_workspace(B, T, S)) return OB_ERR_WORKSPACE;
  if ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15)) return OB_ERR_ALIGN;
  return OB_OK;
}
}  // namespace

int ob_ctc_loss_logits_fwd_groups(const float* logits, const int64_t* targets,
                                  const int64_t* input_lengths, const int64_t* target_lengths,
                                  int64_t G, int64_t B, int64_t T, int64_t V, int64_t S, int blank,
                                  float* loss, void* ws, size_t ws_bytes, void* stream) {
  if (int st = ctc_logits_check(logits, targets, input_lengths, target_lengths, G, B, T, V, S,
                                blank, loss, ws, ws_bytes))
    return st;
  launch_ctc_logits_fwd(logits, targets, input_lengths, target_lengths, B, T, V, S, blank, G,
                        loss, ws, as_stream(stream));
  return launched();
}

int ob_ctc_loss_logits_bwd_groups(const float* logits, const int64_t* targets,
                                  const int64_t* input_lengths, const int64_t* target_lengths,
                                  int64_t G, int64_t B, int64_t T, int64_t V, int64_t S, int blank,
                                  const float* grad_out, float* grad, void* ws, size_t ws_bytes,
                                  void* stream) {
  if (int st = ctc_logits_check(logits, targets, input_lengths, target_lengths, G, B, T, V, S,
                                blank, grad, ws, ws_bytes))
    return st;
  if ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & 15)) return OB_ERR_ALIGN;
  launch_ctc_logits_bwd(logits, targets, input_lengths, target_lengths, B, T, V, S, blank, G,
                        grad_out, grad, ws, as_stream(stream));
  return launched();
}

size_t ob_att_kl_workspace(int64_t P, int64_t BU) {
  if (P < 1 || BU < 0) return 0;
  return align_up(att_kl_workspace(P, BU));
}

namespace {
int att_kl_check(const float* x, const int64_t* tgt, const uint8_t* pad, int64_t P, int64_t BU,
                 int64_t V, float ls, const void* out, size_t ws_bytes, const void* ws) {
  if (P < 1 || P > 64 || BU < 1 || !att_kl_supported(V) || P * BU > INT32_MAX ||
      !(ls > 0.0f && ls < 1.0f))
    return OB_ERR_SHAPE;
  if (!x || !tgt || !pad || !out || !ws) return OB_ERR_NULL;
  if (ws_bytes < ob_att_kl_workspace(P, BU)) return OB_ERR_WORKSPACE;
  if (reinterpret_cast<uintptr_t>(x) & 15) return OB_ERR_ALIGN;
  return OB_OK;
}
}  // namespace

int ob_att_kl_loss_fwd(const float* logits, const int64_t* tgt_out, const uint8_t* tgt_pad,
                       int64_t P, int64_t BU, int64_t V, int pad_id, float label_smoothing,
                       float* l_att, float* l_kl, void* ws, size_t ws_bytes, void* stream) {
  if (int st = att_kl_check(logits, tgt_out, tgt_pad, P, BU, V, label_smoothing, l_att, ws_bytes,
                            ws))
    return st;
  if (P > 1 && !l_kl) return OB_ERR_NULL;
  launch_att_kl_fwd(logits, tgt_out, tgt_pad, P, BU, V, pad_id, label_smoothing, l_att, l_kl, ws,
                    as_stream(stream));
  return launched();
}

int ob_att_kl_loss_bwd(const float* logits, const int64_t* tgt_out, const uint8_t* tgt_pad,
                       int64_t P, int64_t BU, int64_t V, float label_smoothing,
                       const float* g_att, const float* g_kl, float* grad, const void* ws,
                       size_t ws_bytes, void* stream) {
  if (int st = att_kl_check(logits, tgt_out, tgt_pad, P, BU, V, label_smoothing, grad, ws_bytes,
                            ws))
    return st;
  if (!g_att || (P > 1 && !g_kl)) return OB_ERR_NULL;
  if (reinterpret_cast<uintptr_t>(grad) & 15) return OB_ERR_ALIGN;
  launch_att_kl_bwd(logits, tgt_out, tgt_pad, P, BU, V, label_smoothing, g_att, g_kl, grad, ws,
                    as_stream(stream));
  return launched();
}

int ob_loss_combine_fwd(const float* l_att, const float* l_ctc, const float* l_kl, float gamma,
                        float lambda1, float lambda2, float* loss, float* parts, void* stream) {
  if (!l_att || !l_ctc || !l_kl || !loss || !parts) return OB_ERR_NULL;
  launch_loss_combine_fwd(l_att, l_ctc, l_kl, gamma, lambda1, lambda2, loss, parts,
                          as_stream(stream));
  return launched();
}

int ob_loss_combine_bwd(const float* g_loss, float gamma, float lambda1, float lambda2,
                        float* d_att, float* d_ctc, float* d_kl, void* stream) {
  if (!g_loss || !d_att || !d_ctc || !d_kl) return OB_ERR_NULL;
  launch_loss_combine_bwd(g_loss, gamma, lambda1, lambda2, d_att, d_ctc, d_kl, as_stream(stream));
  return launched();
}

int ob_ctc_greedy_decode(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                         int64_t V, int blank, int32_t* ids, int32_t* out, int32_t* out_len,
                         void* stream) {
  if (B < 0 || T < 0 || V < 1 || V > INT32_MAX || blank < 0 || blank >= V) return OB_ERR_SHAPE;
  if (B > 0 && (!lens || !out_len || (T > 0 && (!logits || !ids || !out)))) return OB_ERR_NULL;
  if (!aligned4(logits) || !aligned4(ids) || !aligned4(out) || !aligned4(out_len))
    return OB_ERR_ALIGN;
  launch_ctc_greedy(logits, lens, B, T, V, blank, reinterpret_cast<int*>(ids),
                    reinterpret_cast<int*>(out), reinterpret_cast<int*>(out_len),
                    as_stream(stream));
  return launched();
}

static bool seq_logprob_shape_ok(int64_t R, int64_t d, int64_t V) {
  return R >= 0 && R <= INT32_MAX - 16 && seq_logprob_supported(d, V);
}

size_t ob_seq_logprob_workspace(int64_t R, int64_t d, int64_t V) {
  if (!seq_logprob_shape_ok(R, d, V)) return 0;
  return seq_logprob_workspace(R, d, V);
}

int ob_seq_logprob(const float* hidden, int64_t R, int64_t d, const float* weight,
                   const float* bias, int64_t V, const int32_t* target, void* ws, size_t ws_bytes,
                   float* lp, void* stream) {
  if (!seq_logprob_shape_ok(R, d, V)) return OB_ERR_SHAPE;
  if (R == 0) return OB_OK;
  if (!hidden || !weight || !target || !ws || !lp) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(hidden) & 15) || (reinterpret_cast<uintptr_t>(weight) & 15) ||
      !aligned4(bias) || !aligned4(target) || !aligned4(lp) ||
      (reinterpret_cast<uintptr_t>(ws) & 7))
    return OB_ERR_ALIGN;
  const size_t need = seq_logprob_workspace(R, d, V);
  if (need == 0) return OB_ERR_SHAPE;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  launch_seq_logprob(hidden, R, d, weight, bias, V, reinterpret_cast<const int*>(target), ws, lp,
                     as_stream(stream));
  return launched();
}

static bool rescore_shape_ok(int64_t B, int64_t N, int64_t T, int64_t Lc) {
  return B >= 0 && B <= INT32_MAX && N >= 1 && N <= 32 && T >= 0 && T < (1 << 24) && Lc >= 0 &&
         Lc < (1 << 16) && (B == 0 || N * std::max<int64_t>(T, Lc + 1) <= INT32_MAX / B);
}

int ob_rescore_prepare(const int32_t* hyp, const int32_t* hyp_len, const int32_t* n_hyp,
                       int64_t B, int64_t N, int64_t T, int64_t Lc, int bos, int eos, int pad,
                       int64_t* tgt_inp, int32_t* target, uint8_t* tgt_pad, uint8_t* ok,
                       void* stream) {
  if (!rescore_shape_ok(B, N, T, Lc)) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if ((T > 0 && !hyp) || !hyp_len || !n_hyp || !tgt_inp || !target || !tgt_pad || !ok)
    return OB_ERR_NULL;
  if (!aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) || !aligned4(target) ||
      (reinterpret_cast<uintptr_t>(tgt_inp) & 7))
    return OB_ERR_ALIGN;
  launch_rescore_prepare(reinterpret_cast<const int*>(hyp), reinterpret_cast<const int*>(hyp_len),
                         reinterpret_cast<const int*>(n_hyp), B, N, T, Lc, bos, eos, pad, tgt_inp,
                         reinterpret_cast<int*>(target), tgt_pad, ok, as_stream(stream));
  return launched();
}

int ob_attdec_supported(int64_t N, int64_t d, int64_t H, int64_t Lk, int64_t L) {
  return attdec_supported(N, d, H, Lk, L) ? 1 : 0;
}

int ob_decattn_step(const float* qkv, int64_t sq, float* cache, const int32_t* anc,
                    const uint8_t* skip, int64_t R, int64_t H, int64_t dh, int64_t L, int64_t t,
                    float* ctx, void* stream) {
  if (R < 0 || H < 1 || !(dh == 16 || dh == 32 || dh == 36 || dh == 64) || L < 1 || L + 1 > 256 ||
      t < 0 || t >= L)
    return OB_ERR_SHAPE;
  if (H > 64 || sq < 3 * H * dh || sq % 4 || R * H > INT32_MAX || R * L > INT32_MAX)
    return OB_ERR_SHAPE;
  if (R == 0) return OB_OK;
  if (!qkv || !cache || !anc || !ctx) return OB_ERR_NULL;
  if (!aligned16(qkv) || !aligned16(cache) || !aligned4(anc) || !aligned4(ctx))
    return OB_ERR_ALIGN;
  launch_decattn_step(qkv, sq, cache, reinterpret_cast<const int*>(anc), skip, R, H, dh, L, t, ctx,
                      as_stream(stream));
  return launched();
}

static bool seq_topk_shape_ok(int64_t R, int64_t d, int64_t V, int64_t K) {
  return seq_logprob_shape_ok(R, d, V) && K >= 1 && K <= 32;
}

size_t ob_seq_topk_workspace(int64_t R, int64_t d, int64_t V, int64_t K) {
  if (!seq_topk_shape_ok(R, d, V, K)) return 0;
  return seq_topk_workspace(R, d, V, K);
}

int ob_seq_topk(const float* hidden, int64_t R, int64_t d, const float* weight, const float* bias,
                int64_t V, const int32_t* banned, int n_banned, const uint8_t* skip, int64_t K,
                void* ws, size_t ws_bytes, double* lse, float* topv, int32_t* topi,
                void* stream) {
  if (!seq_topk_shape_ok(R, d, V, K) || n_banned < 0 || n_banned > kSeqTopkMaxBanned)
    return OB_ERR_SHAPE;
  if (R == 0) return OB_OK;
  if (!hidden || !weight || !ws || !lse || !topv || !topi || (n_banned > 0 && !banned))
    return OB_ERR_NULL;
  if (!aligned16(hidden) || !aligned16(weight) || !aligned4(bias) || !aligned4(banned) ||
      !aligned4(topv) || !aligned4(topi) || (reinterpret_cast<uintptr_t>(ws) & 7) ||
      (reinterpret_cast<uintptr_t>(lse) & 7))
    return OB_ERR_ALIGN;
  const size_t need = seq_topk_workspace(R, d, V, K);
  if (need == 0) return OB_ERR_SHAPE;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  launch_seq_topk(hidden, R, d, weight, bias, V, reinterpret_cast<const int*>(banned), n_banned,
                  skip, K, ws, lse, topv, reinterpret_cast<int*>(topi), as_stream(stream));
  return launched();
}

static bool attdec_state_shape_ok(int64_t B, int64_t N, int64_t L) {
  return B >= 0 && N >= 1 && N <= 32 && L >= 1 && L + 1 <= 256 &&
         (B == 0 || N * L <= INT32_MAX / B);
}

static int attdec_state_check(const double* score, const int32_t* len, const uint8_t* fin,
                              const int64_t* tok, const uint8_t* skip) {
  if (!score || !len || !fin || !tok || !skip) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(score) & 7) || (reinterpret_cast<uintptr_t>(tok) & 7) ||
      !aligned4(len))
    return OB_ERR_ALIGN;
  return OB_OK;
}

int ob_attdec_init(const uint8_t* kmask, int64_t B, int64_t N, int64_t Lk, int64_t L, int bos,
                   double* score, int32_t* len, uint8_t* fin, int64_t* tok, uint8_t* skip,
                   int32_t* anc, void* stream) {
  if (!attdec_state_shape_ok(B, N, L) || Lk < 1 || Lk > INT32_MAX) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!anc) return OB_ERR_NULL;
  if (int st = attdec_state_check(score, len, fin, tok, skip)) return st;
  if (!aligned4(anc)) return OB_ERR_ALIGN;
  const AttdecState st{score, reinterpret_cast<int*>(len), fin, tok, skip};
  launch_attdec_init(kmask, B, N, Lk, L, bos, st, reinterpret_cast<int*>(anc), as_stream(stream));
  return launched();
}

// The three step entries' checks and launch. A mode's entry passes null / 0 for the arguments it
// does not have; a null pointer passes every alignment check.
static int attdec_step(int mode, const double* lse, const float* topv, const int32_t* topi,
                       const double* cpsi, double ctc_weight, const double* lmsc, double lm_weight,
                       int64_t B, int64_t N, int64_t K, int64_t L, int64_t t, int eos, int pad,
                       const double* norm, const int32_t* anc_in, int32_t* anc_out, double* score,
                       double* att, double* ctc, double* lm, int32_t* len, uint8_t* fin,
                       int64_t* tok, uint8_t* skip, int32_t* link, int32_t* trace_parent,
                       int32_t* trace_token, double* trace_score, void* stream,
                       const double* bsc = nullptr, double bias_weight = 0.0,
                       double* bias = nullptr) {
  const bool joint = mode != kStepBeam, biased = mode == kStepBiased;
  const bool fused = mode == kStepFused || biased;
  if (!attdec_state_shape_ok(B, N, L) || K < (joint ? N : 1) || K > 32 || t < 0 || t >= L ||
      (joint && !(ctc_weight >= 0.0 && ctc_weight <= 1.0)) ||
      (fused && !(lm_weight == lm_weight)) ||
      (biased && (!(bias_weight >= 0.0 && bias_weight <= 1.7976931348623157e308) ||
                  (!lmsc && lm_weight != 0.0))))
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!lse || !topv || !topi || !norm || !anc_in || !anc_out || !trace_parent || !trace_token ||
      !trace_score || (joint && (!att || !ctc || !link)) ||
      ((fused ? ctc_weight > 0.0 : joint) && !cpsi) ||
      (fused && (biased ? lmsc && !lm : !lmsc || !lm)) || (biased && (!bsc || !bias)))
    return OB_ERR_NULL;
  if (int st = attdec_state_check(score, len, fin, tok, skip)) return st;
  if (misaligned8(lse) || misaligned8(cpsi) || misaligned8(lmsc) || misaligned8(norm) ||
      misaligned8(bsc) || misaligned8(bias) ||
      misaligned8(att) || misaligned8(ctc) || misaligned8(lm) || misaligned8(trace_score) ||
      !aligned4(topv) || !aligned4(topi) || !aligned4(anc_in) || !aligned4(anc_out) ||
      !aligned4(link) || !aligned4(trace_parent) || !aligned4(trace_token))
    return OB_ERR_ALIGN;
  if (anc_in == anc_out) return OB_ERR_SHAPE;  // the rows are permuted: two buffers
  const AttdecState st{score, reinterpret_cast<int*>(len), fin, tok, skip};
  launch_attdec_step(mode, lse, topv, reinterpret_cast<const int*>(topi), cpsi, ctc_weight, lmsc,
                     lm_weight, B, N, K, L, t, eos, pad, norm,
                     reinterpret_cast<const int*>(anc_in), reinterpret_cast<int*>(anc_out), st, att,
                     ctc, lm, reinterpret_cast<int*>(link), reinterpret_cast<int*>(trace_parent),
                     reinterpret_cast<int*>(trace_token), trace_score, as_stream(stream), bsc,
                     bias_weight, bias);
  return launched();
}

int ob_attdec_beam_step(const double* lse, const float* topv, const int32_t* topi, int64_t B,
                        int64_t N, int64_t K, int64_t L, int64_t t, int eos, int pad,
                        const double* norm, const int32_t* anc_in, int32_t* anc_out, double* score,
                        int32_t* len, uint8_t* fin, int64_t* tok, uint8_t* skip,
                        int32_t* trace_parent, int32_t* trace_token, double* trace_score,
                        void* stream) {
  return attdec_step(kStepBeam, lse, topv, topi, nullptr, 0.0, nullptr, 0.0, B, N, K, L, t, eos,
                     pad, norm, anc_in, anc_out, score, nullptr, nullptr, nullptr, len, fin, tok,
                     skip, nullptr, trace_parent, trace_token, trace_score, stream);
}

int ob_attdec_finalize(const int32_t* trace_parent, const int32_t* trace_token,
                       const double* score, const int32_t* len, const uint8_t* fin, int64_t B,
                       int64_t N, int64_t L, int eos, int32_t* hyp, int32_t* hyp_len,
                       int32_t* n_hyp, double* score_out, uint8_t* finished, void* stream) {
  if (!attdec_state_shape_ok(B, N, L)) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!trace_parent || !trace_token || !score || !len || !fin || !hyp || !hyp_len || !n_hyp ||
      !score_out || !finished)
    return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(score) & 7) || (reinterpret_cast<uintptr_t>(score_out) & 7) ||
      !aligned4(trace_parent) || !aligned4(trace_token) || !aligned4(len) || !aligned4(hyp) ||
      !aligned4(hyp_len) || !aligned4(n_hyp))
    return OB_ERR_ALIGN;
  const AttdecState st{const_cast<double*>(score), reinterpret_cast<int*>(const_cast<int32_t*>(len)),
                       const_cast<uint8_t*>(fin), nullptr, nullptr};
  launch_attdec_finalize(reinterpret_cast<const int*>(trace_parent),
                         reinterpret_cast<const int*>(trace_token), st, B, N, L, eos,
                         reinterpret_cast<int*>(hyp), reinterpret_cast<int*>(hyp_len),
                         reinterpret_cast<int*>(n_hyp), score_out, finished, as_stream(stream));
  return launched();
}

int ob_attdec_joint_step(const double* lse, const float* topv, const int32_t* topi,
                         const double* cpsi, double ctc_weight, int64_t B, int64_t N, int64_t K,
                         int64_t L, int64_t t, int eos, int pad, const double* norm,
                         const int32_t* anc_in, int32_t* anc_out, double* score, double* att,
                         double* ctc, int32_t* len, uint8_t* fin, int64_t* tok, uint8_t* skip,
                         int32_t* link, int32_t* trace_parent, int32_t* trace_token,
                         double* trace_score, void* stream) {
  return attdec_step(kStepJoint, lse, topv, topi, cpsi, ctc_weight, nullptr, 0.0, B, N, K, L, t,
                     eos, pad, norm, anc_in, anc_out, score, att, ctc, nullptr, len, fin, tok, skip,
                     link, trace_parent, trace_token, trace_score, stream);
}

int ob_ctc_prefix_supported(int64_t N, int64_t K, int64_t Tp) {
  return ctc_prefix_supported(N, K, Tp) ? 1 : 0;
}

size_t ob_ctc_prefix_workspace(int64_t B, int64_t N, int64_t K, int64_t Tp) {
  if (B < 0 || (B > 0 && N > 0 && B > INT32_MAX / N)) return 0;
  return ctc_prefix_workspace(B, N, K, Tp);
}

static bool ctc_logits_shape_ok(int64_t B, int64_t Tp, int64_t V) {
  return B >= 0 && Tp >= 1 && Tp <= 256 && V >= 1 && V <= INT32_MAX &&
         (B == 0 || V <= INT64_MAX / 4 / Tp / B);
}

int ob_ctc_frame_lse(const float* logits, const int64_t* lens, int64_t B, int64_t Tp, int64_t V,
                     double* flse, void* stream) {
  if (!ctc_logits_shape_ok(B, Tp, V) || B * Tp > INT32_MAX) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!logits || !lens || !flse) return OB_ERR_NULL;
  if (!aligned4(logits) || misaligned8(lens) || misaligned8(flse)) return OB_ERR_ALIGN;
  launch_ctc_frame_lse(logits, lens, B, Tp, V, flse, as_stream(stream));
  return launched();
}

int ob_ctc_prefix_step(const float* logits, const double* flse, const int64_t* lens,
                       const int32_t* topi, const int64_t* tok, const int32_t* len,
                       const int32_t* link, const uint8_t* skip, int64_t B, int64_t N, int64_t K,
                       int64_t Tp, int64_t V, int blank, int eos, const double* state_in,
                       double* state_out, double* cpsi, void* stream) {
  if (!ctc_prefix_supported(N, K, Tp) || !ctc_logits_shape_ok(B, Tp, V) ||
      (B > 0 && B > INT32_MAX / 2 / N) || blank < 0 || blank >= V || eos < 0 || eos >= V)
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!logits || !flse || !lens || !topi || !tok || !len || !link || !skip || !state_in ||
      !state_out || !cpsi)
    return OB_ERR_NULL;
  if (!aligned4(logits) || !aligned4(topi) || !aligned4(len) || !aligned4(link) ||
      misaligned8(flse) || misaligned8(lens) || misaligned8(tok) || misaligned8(state_in) ||
      misaligned8(state_out) || misaligned8(cpsi))
    return OB_ERR_ALIGN;
  if (state_in == state_out) return OB_ERR_SHAPE;  // a row reads its parent's row: two tables
  launch_ctc_prefix_step(logits, flse, lens, reinterpret_cast<const int*>(topi), tok,
                         reinterpret_cast<const int*>(len), reinterpret_cast<const int*>(link),
                         skip, B, N, K, Tp, V, blank, eos, state_in, state_out, cpsi,
                         as_stream(stream));
  return launched();
}

int ob_ngram_supported(int64_t order, int64_t V, int64_t K) {
  return ngram_supported(order, V, K) ? 1 : 0;
}

int64_t ob_ngram_table_slots(int64_t n_entries) { return ngram_table_slots(n_entries); }

int ob_ngram_table_build(const uint64_t* keys, const float* vals, int64_t n_entries, void* table,
                         size_t table_bytes, int64_t* slots, int32_t* max_probe) {
  if (n_entries < 0 || ngram_table_slots(n_entries) == 0) return OB_ERR_SHAPE;
  if (!slots || !max_probe || (n_entries > 0 && (!keys || !vals))) return OB_ERR_NULL;
  if (misaligned8(keys) || !aligned4(vals) || (reinterpret_cast<uintptr_t>(table) & 15))
    return OB_ERR_ALIGN;
  int mp = 0;
  const int st = ngram_table_build(keys, vals, n_entries, table, table_bytes, slots, &mp);
  *max_probe = mp;
  return st == 0 ? OB_OK : (st == 1 ? OB_ERR_SHAPE : OB_ERR_WORKSPACE);
}

// a table argument: slots a power of two >= 8, the probe bound the builder's
static bool ngram_table_ok(int64_t slots, int max_probe, int order, int64_t V) {
  return slots >= 8 && (slots & (slots - 1)) == 0 && max_probe >= 1 && max_probe <= 64 &&
         ngram_supported(order, V, 1);
}

int ob_ngram_score_host(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                        double unk_logp, const uint64_t* ctx, const int32_t* w, int64_t Q,
                        double* out, int32_t* probes) {
  if (!ngram_table_ok(slots, max_probe, order, V) || Q < 0) return OB_ERR_SHAPE;
  if (Q == 0) return OB_OK;
  if (!table || !ctx || !w || !out) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(table) & 15) || misaligned8(ctx) || misaligned8(out) ||
      !aligned4(w) || !aligned4(probes))
    return OB_ERR_ALIGN;
  ngram_score_host(table, slots, max_probe, order, V, unk_logp, ctx,
                   reinterpret_cast<const int*>(w), Q, out, reinterpret_cast<int*>(probes));
  return OB_OK;
}

int ob_ngram_step(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                  double unk_logp, const int32_t* topi, const int64_t* tok, const int32_t* len,
                  const int32_t* link, const uint8_t* skip, int64_t B, int64_t N, int64_t K,
                  int bos, const uint64_t* ctx_in, uint64_t* ctx_out, double* lmsc,
                  void* stream) {
  if (!ngram_table_ok(slots, max_probe, order, V) || !ngram_supported(order, V, K) || B < 0 ||
      N < 1 || N > 32 || (B > 0 && B > INT32_MAX / 64 / N) || bos < 0 || bos >= V)
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!table || !topi || !tok || !len || !link || !skip || !ctx_in || !ctx_out || !lmsc)
    return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(table) & 15) || !aligned4(topi) || !aligned4(len) ||
      !aligned4(link) || misaligned8(tok) || misaligned8(ctx_in) || misaligned8(ctx_out) ||
      misaligned8(lmsc))
    return OB_ERR_ALIGN;
  if (ctx_in == ctx_out) return OB_ERR_SHAPE;  // a row reads its parent's row: two tables
  launch_ngram_step(table, slots, max_probe, order, V, unk_logp,
                    reinterpret_cast<const int*>(topi), tok, reinterpret_cast<const int*>(len),
                    reinterpret_cast<const int*>(link), skip, B, N, K, bos, ctx_in, ctx_out, lmsc,
                    as_stream(stream));
  return launched();
}

int ob_ngram_seq_logprob(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                         double unk_logp, const int32_t* hyp, const int32_t* hyp_len, int64_t R,
                         int64_t T, int bos, int eos, double* lm, double* tok_lm, void* stream) {
  if (!ngram_table_ok(slots, max_probe, order, V) || R < 0 || R > INT32_MAX || T < 0 ||
      T >= (1 << 24) || bos < 0 || bos >= V || eos < 0 || eos >= V)
    return OB_ERR_SHAPE;
  if (R == 0) return OB_OK;
  if (!table || (T > 0 && !hyp) || !hyp_len || !lm) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(table) & 15) || !aligned4(hyp) || !aligned4(hyp_len) ||
      misaligned8(lm) || misaligned8(tok_lm))
    return OB_ERR_ALIGN;
  launch_ngram_seq_logprob(table, slots, max_probe, order, V, unk_logp,
                           reinterpret_cast<const int*>(hyp),
                           reinterpret_cast<const int*>(hyp_len), R, T, bos, eos, lm, tok_lm,
                           as_stream(stream));
  return launched();
}

// the tables of a phrase list: slots a power of two >= 8, the probe bound the builder's
static bool bias_tables_ok(int64_t n_nodes, int64_t slots, int max_probe, int64_t V) {
  return slots >= 8 && (slots & (slots - 1)) == 0 && slots <= ((int64_t)1 << 40) &&
         max_probe >= 1 && max_probe <= 64 && bias_supported(V, 1, n_nodes);
}

int ob_bias_supported(int64_t V, int64_t K, int64_t n_nodes) {
  return bias_supported(V, K, n_nodes) ? 1 : 0;
}

int ob_bias_sizes(int64_t n_phrases, int64_t total_tokens, int64_t* max_nodes,
                  int64_t* min_slots) {
  if (!max_nodes || !min_slots) return OB_ERR_NULL;
  if (misaligned8(max_nodes) || misaligned8(min_slots)) return OB_ERR_ALIGN;
  return bias_sizes(n_phrases, total_tokens, max_nodes, min_slots) ? OB_OK : OB_ERR_SHAPE;
}

int ob_bias_build(const int32_t* tokens, const int32_t* lengths, const float* boosts,
                  int64_t n_phrases, void* nodes, size_t nodes_bytes, void* edges,
                  size_t edges_bytes, int64_t* n_nodes, int64_t* slots, int32_t* max_probe) {
  if (n_phrases < 0 || n_phrases > ((int64_t)1 << 26)) return OB_ERR_SHAPE;
  if (!n_nodes || !slots || !max_probe || (n_phrases > 0 && (!tokens || !lengths || !boosts)))
    return OB_ERR_NULL;
  if (!aligned4(tokens) || !aligned4(lengths) || !aligned4(boosts) || !aligned4(max_probe) ||
      misaligned8(n_nodes) || misaligned8(slots) || (reinterpret_cast<uintptr_t>(nodes) & 15) ||
      (reinterpret_cast<uintptr_t>(edges) & 15))
    return OB_ERR_ALIGN;
  int mp = 0;
  const int st = bias_build(reinterpret_cast<const int*>(tokens),
                            reinterpret_cast<const int*>(lengths), boosts, n_phrases, nodes,
                            nodes_bytes, edges, edges_bytes, n_nodes, slots, &mp);
  if (st == 1) return OB_ERR_SHAPE;
  *max_probe = mp;
  return st == 0 ? OB_OK : OB_ERR_WORKSPACE;
}

int ob_bias_walk_host(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                      int max_probe, const int32_t* tokens, const int32_t* lens, int64_t Q,
                      int64_t T, int32_t* state, double* kept, double* bias, double* bias_fin) {
  if (!bias_tables_ok(n_nodes, slots, max_probe, 1) || Q < 0 || T < 0 || T >= (1 << 24))
    return OB_ERR_SHAPE;
  if (Q == 0) return OB_OK;
  if (!nodes || !edges || (T > 0 && !tokens) || !lens || !state || !kept || !bias || !bias_fin)
    return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(nodes) & 15) || (reinterpret_cast<uintptr_t>(edges) & 15) ||
      !aligned4(tokens) || !aligned4(lens) || !aligned4(state) || misaligned8(kept) ||
      misaligned8(bias) || misaligned8(bias_fin))
    return OB_ERR_ALIGN;
  bias_walk_host(nodes, n_nodes, edges, slots, max_probe, reinterpret_cast<const int*>(tokens),
                 reinterpret_cast<const int*>(lens), Q, T, reinterpret_cast<int*>(state), kept,
                 bias, bias_fin);
  return OB_OK;
}

int ob_bias_step(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                 int max_probe, const int32_t* topi, const int64_t* tok, const int32_t* len,
                 const int32_t* link, const uint8_t* skip, int64_t B, int64_t N, int64_t K,
                 int eos, const int32_t* st_in, int32_t* st_out, const double* kept_in,
                 double* kept_out, double* bsc, void* stream) {
  if (!bias_tables_ok(n_nodes, slots, max_probe, 1) || !bias_supported(1, K, n_nodes) || B < 0 ||
      N < 1 || N > 32 || (B > 0 && B > INT32_MAX / 64 / N) || eos < 0)
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!nodes || !edges || !topi || !tok || !len || !link || !skip || !st_in || !st_out ||
      !kept_in || !kept_out || !bsc)
    return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(nodes) & 15) || (reinterpret_cast<uintptr_t>(edges) & 15) ||
      !aligned4(topi) || !aligned4(len) || !aligned4(link) || !aligned4(st_in) ||
      !aligned4(st_out) || misaligned8(tok) || misaligned8(kept_in) || misaligned8(kept_out) ||
      misaligned8(bsc))
    return OB_ERR_ALIGN;
  if (st_in == st_out || kept_in == kept_out)
    return OB_ERR_SHAPE;  // a row reads its parent's row: two tables
  launch_bias_step(nodes, n_nodes, edges, slots, max_probe, reinterpret_cast<const int*>(topi),
                   tok, reinterpret_cast<const int*>(len), reinterpret_cast<const int*>(link),
                   skip, B, N, K, eos, reinterpret_cast<const int*>(st_in),
                   reinterpret_cast<int*>(st_out), kept_in, kept_out, bsc, as_stream(stream));
  return launched();
}

int ob_bias_seq_score(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                      int max_probe, const int32_t* hyp, const int32_t* hyp_len, int64_t R,
                      int64_t T, double* bias_fin, void* stream) {
  if (!bias_tables_ok(n_nodes, slots, max_probe, 1) || R < 0 || R > INT32_MAX || T < 0 ||
      T >= (1 << 24))
    return OB_ERR_SHAPE;
  if (R == 0) return OB_OK;
  if (!nodes || !edges || (T > 0 && !hyp) || !hyp_len || !bias_fin) return OB_ERR_NULL;
  if ((reinterpret_cast<uintptr_t>(nodes) & 15) || (reinterpret_cast<uintptr_t>(edges) & 15) ||
      !aligned4(hyp) || !aligned4(hyp_len) || misaligned8(bias_fin))
    return OB_ERR_ALIGN;
  launch_bias_seq_score(nodes, n_nodes, edges, slots, max_probe,
                        reinterpret_cast<const int*>(hyp), reinterpret_cast<const int*>(hyp_len),
                        R, T, bias_fin, as_stream(stream));
  return launched();
}

static bool ctc_beam_shape_ok(int64_t B, int64_t T, int64_t V, int beam, int top_k) {
  // T < 2^24 keeps the prefix table's slot ids below 2^30; B * T rows index one launch grid
  return B >= 0 && B <= INT32_MAX && T >= 0 && T < (1 << 24) && V >= 1 && V <= INT32_MAX &&
         beam >= 1 && beam <= 32 && top_k >= 1 && top_k <= 64 && (B == 0 || T <= INT32_MAX / B);
}

size_t ob_ctc_beam_search_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k) {
  if (!ctc_beam_shape_ok(B, T, V, beam, top_k)) return 0;
  return ctc_beam_workspace(B, T, V, beam, top_k);
}

size_t ob_ctc_beam_search_nbest_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k) {
  return ob_ctc_beam_search_workspace(B, T, V, beam, top_k);
}

size_t ob_ctc_beam_search_lm_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k,
                                       int order) {
  if (!ctc_beam_shape_ok(B, T, V, beam, top_k) || !ngram_supported(order, V, 1)) return 0;
  return ctc_beam_workspace(B, T, V, beam, top_k);
}

// The three search entries' checks and launch. one_best: the 1-best form, the only one with a
// stage (0 both kernels, 1 the frame kernel, 2 the search), no n_hyp and an optional score; the
// others pass stage 0. lm: the fused form, whose ctc / lm / total take the place of score. A
// null pointer passes every alignment check.
static int ctc_beam_search(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                           int64_t V, int blank, int beam, int top_k, int stage, bool one_best,
                           int nbest, const CtcBeamLm* lm, void* ws, size_t ws_bytes, int32_t* hyp,
                           int32_t* hyp_len, int32_t* n_hyp, double* score, void* stream,
                           const CtcBeamBias* bias = nullptr) {
  const double kMax = 1.7976931348623157e308;  // finite: neither NaN nor an infinity
  // the biased form without an LM: a null table, whose other LM arguments are not read
  const bool no_lm = bias && lm && !lm->table;
  if (!ctc_beam_shape_ok(B, T, V, beam, top_k) || blank < 0 || blank >= V || stage < 0 ||
      stage > 2 || nbest < 1 || nbest > beam ||
      (lm && !no_lm &&
       (!ngram_table_ok(lm->slots, lm->max_probe, lm->order, V) || lm->bos < 0 ||
        lm->bos >= V || lm->eos < 0 || lm->eos >= V ||
        !(lm->lm_weight >= 0.0 && lm->lm_weight <= kMax) ||
        !(lm->unk_logp >= -kMax && lm->unk_logp <= kMax))) ||
      (lm && !(lm->ins_bonus >= -kMax && lm->ins_bonus <= kMax)) ||
      (no_lm && lm->lm_weight != 0.0) ||
      (bias && (!lm || !bias_tables_ok(bias->n_nodes, bias->slots, bias->max_probe, V) ||
                !(bias->bias_weight >= 0.0 && bias->bias_weight <= kMax))))
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  const bool frames = stage != 2, search = stage != 1;
  if (!lens || !ws || (frames && T > 0 && !logits) ||
      (search && (!hyp_len || (T > 0 && !hyp))) ||
      (!one_best && (!n_hyp || (lm ? (!bias && !lm->table) || !lm->ctc || !lm->lm || !lm->total
                                   : !score))) ||
      (bias && (!bias->nodes || !bias->edges || !bias->bias)))
    return OB_ERR_NULL;
  if (!aligned4(logits) || !aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) ||
      misaligned8(lens) || misaligned8(ws) || misaligned8(score) ||
      (lm && ((reinterpret_cast<uintptr_t>(lm->table) & 15) || misaligned8(lm->ctc) ||
              misaligned8(lm->lm) || misaligned8(lm->total))) ||
      (bias && ((reinterpret_cast<uintptr_t>(bias->nodes) & 15) ||
                (reinterpret_cast<uintptr_t>(bias->edges) & 15) || misaligned8(bias->bias))))
    return OB_ERR_ALIGN;
  const size_t need = ctc_beam_workspace(B, T, V, beam, top_k);
  if (need == 0) return OB_ERR_SHAPE;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  launch_ctc_beam(logits, lens, B, T, V, blank, beam, top_k, (frames ? 1 : 0) | (search ? 2 : 0),
                  ws, reinterpret_cast<int*>(hyp), reinterpret_cast<int*>(hyp_len),
                  reinterpret_cast<int*>(n_hyp), score, one_best ? 0 : nbest, lm,
                  as_stream(stream), bias);
  return launched();
}

int ob_ctc_beam_search_stage(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                             int64_t V, int blank, int beam, int top_k, int stage, void* ws,
                             size_t ws_bytes, int32_t* out, int32_t* out_len, double* score,
                             void* stream) {
  return ctc_beam_search(logits, lens, B, T, V, blank, beam, top_k, stage, true, 1, nullptr, ws,
                         ws_bytes, out, out_len, nullptr, score, stream);
}

int ob_ctc_beam_search(const float* logits, const int64_t* lens, int64_t B, int64_t T, int64_t V,
                       int blank, int beam, int top_k, void* ws, size_t ws_bytes, int32_t* out,
                       int32_t* out_len, double* score, void* stream) {
  return ob_ctc_beam_search_stage(logits, lens, B, T, V, blank, beam, top_k, 0, ws, ws_bytes, out,
                                  out_len, score, stream);
}

int ob_ctc_beam_search_nbest(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                             int64_t V, int blank, int beam, int top_k, int nbest, void* ws,
                             size_t ws_bytes, int32_t* hyp, int32_t* hyp_len, int32_t* n_hyp,
                             double* score, void* stream) {
  return ctc_beam_search(logits, lens, B, T, V, blank, beam, top_k, 0, false, nbest, nullptr, ws,
                         ws_bytes, hyp, hyp_len, n_hyp, score, stream);
}

int ob_ctc_beam_search_lm(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                          int64_t V, int blank, int beam, int top_k, int nbest, const void* table,
                          int64_t slots, int max_probe, int order, double unk_logp, int bos,
                          int eos, double lm_weight, double ins_bonus, void* ws, size_t ws_bytes,
                          int32_t* hyp, int32_t* hyp_len, int32_t* n_hyp, double* ctc, double* lm,
                          double* total, void* stream) {
  const CtcBeamLm la{table, slots, max_probe, order, unk_logp, bos, eos, lm_weight, ins_bonus,
                     ctc, lm, total};
  return ctc_beam_search(logits, lens, B, T, V, blank, beam, top_k, 0, false, nbest, &la, ws,
                         ws_bytes, hyp, hyp_len, n_hyp, nullptr, stream);
}

size_t ob_ctc_beam_search_bias_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k,
                                         int order, int64_t n_nodes) {
  // order 0: the search without an LM
  if (!ctc_beam_shape_ok(B, T, V, beam, top_k) || !bias_supported(V, 1, n_nodes) ||
      (order != 0 && !ngram_supported(order, V, 1)))
    return 0;
  return ctc_beam_workspace(B, T, V, beam, top_k);
}

int ob_ctc_beam_search_bias(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                            int64_t V, int blank, int beam, int top_k, int nbest,
                            const void* table, int64_t slots, int max_probe, int order,
                            double unk_logp, int bos, int eos, double lm_weight, double ins_bonus,
                            const void* bias_nodes, int64_t n_nodes, const void* bias_edges,
                            int64_t bias_slots, int bias_max_probe, double bias_weight, void* ws,
                            size_t ws_bytes, int32_t* hyp, int32_t* hyp_len, int32_t* n_hyp,
                            double* ctc, double* lm, double* bias, double* total, void* stream) {
  const CtcBeamLm la{table, slots, max_probe, order, unk_logp, bos, eos, lm_weight, ins_bonus,
                     ctc, lm, total};
  const CtcBeamBias ba{bias_nodes, n_nodes, bias_edges, bias_slots, bias_max_probe, bias_weight,
                       bias};
  return ctc_beam_search(logits, lens, B, T, V, blank, beam, top_k, 0, false, nbest, &la, ws,
                         ws_bytes, hyp, hyp_len, n_hyp, nullptr, stream, &ba);
}

int ob_attdec_biased_step(const double* lse, const float* topv, const int32_t* topi,
                          const double* cpsi, double ctc_weight, const double* lmsc,
                          double lm_weight, const double* bsc, double bias_weight, int64_t B,
                          int64_t N, int64_t K, int64_t L, int64_t t, int eos, int pad,
                          const double* norm, const int32_t* anc_in, int32_t* anc_out,
                          double* score, double* att, double* ctc, double* lm, double* bias,
                          int32_t* len, uint8_t* fin, int64_t* tok, uint8_t* skip, int32_t* link,
                          int32_t* trace_parent, int32_t* trace_token, double* trace_score,
                          void* stream) {
  return attdec_step(kStepBiased, lse, topv, topi, cpsi, ctc_weight, lmsc, lm_weight, B, N, K, L,
                     t, eos, pad, norm, anc_in, anc_out, score, att, ctc, lm, len, fin, tok, skip,
                     link, trace_parent, trace_token, trace_score, stream, bsc, bias_weight, bias);
}

int ob_attdec_fused_step(const double* lse, const float* topv, const int32_t* topi,
                         const double* cpsi, double ctc_weight, const double* lmsc,
                         double lm_weight, int64_t B, int64_t N, int64_t K, int64_t L, int64_t t,
                         int eos, int pad, const double* norm, const int32_t* anc_in,
                         int32_t* anc_out, double* score, double* att, double* ctc, double* lm,
                         int32_t* len, uint8_t* fin, int64_t* tok, uint8_t* skip, int32_t* link,
                         int32_t* trace_parent, int32_t* trace_token, double* trace_score,
                         void* stream) {
  return attdec_step(kStepFused, lse, topv, topi, cpsi, ctc_weight, lmsc, lm_weight, B, N, K, L, t,
                     eos, pad, norm, anc_in, anc_out, score, att, ctc, lm, len, fin, tok, skip,
                     link, trace_parent, trace_token, trace_score, stream);
}

// The two pick entries' checks and launch. with_lm: lm is required, and lp may be null together
// with ok / att (no attention pass); without, lm is null and lp, ok and att are required.
static int rescore_select(bool with_lm, const float* lp, const int32_t* hyp,
                          const int32_t* hyp_len, const int32_t* n_hyp, const double* ctc_score,
                          const double* lm, const uint8_t* ok, int64_t B, int64_t N, int64_t T,
                          int64_t Lc, double ctc_weight, double lm_weight, int32_t* out,
                          int32_t* out_len, int32_t* best_k, double* att, double* total,
                          uint8_t* rescored, void* stream) {
  if (!rescore_shape_ok(B, N, T, Lc)) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if ((with_lm ? !lm || (lp && (!ok || !att)) : !lp || !ok || !att) ||
      (T > 0 && (!hyp || !out)) || !hyp_len || !n_hyp || !ctc_score || !out_len || !best_k ||
      !total || !rescored)
    return OB_ERR_NULL;
  if (!aligned4(lp) || !aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) ||
      !aligned4(out) || !aligned4(out_len) || !aligned4(best_k) || misaligned8(ctc_score) ||
      misaligned8(lm) || misaligned8(att) || misaligned8(total))
    return OB_ERR_ALIGN;
  launch_rescore_select(lp, reinterpret_cast<const int*>(hyp),
                        reinterpret_cast<const int*>(hyp_len), reinterpret_cast<const int*>(n_hyp),
                        ctc_score, lm, ok, B, N, T, Lc, ctc_weight, lm_weight,
                        reinterpret_cast<int*>(out), reinterpret_cast<int*>(out_len),
                        reinterpret_cast<int*>(best_k), att, total, rescored, as_stream(stream));
  return launched();
}

int ob_rescore_select(const float* lp, const int32_t* hyp, const int32_t* hyp_len,
                      const int32_t* n_hyp, const double* ctc_score, const uint8_t* ok, int64_t B,
                      int64_t N, int64_t T, int64_t Lc, double ctc_weight, int32_t* out,
                      int32_t* out_len, int32_t* best_k, double* att, double* total,
                      uint8_t* rescored, void* stream) {
  return rescore_select(false, lp, hyp, hyp_len, n_hyp, ctc_score, nullptr, ok, B, N, T, Lc,
                        ctc_weight, 0.0, out, out_len, best_k, att, total, rescored, stream);
}

int ob_rescore_select_lm(const float* lp, const int32_t* hyp, const int32_t* hyp_len,
                         const int32_t* n_hyp, const double* ctc_score, const double* lm,
                         const uint8_t* ok, int64_t B, int64_t N, int64_t T, int64_t Lc,
                         double ctc_weight, double lm_weight, int32_t* out, int32_t* out_len,
                         int32_t* best_k, double* att, double* total, uint8_t* rescored,
                         void* stream) {
  return rescore_select(true, lp, hyp, hyp_len, n_hyp, ctc_score, lm, ok, B, N, T, Lc, ctc_weight,
                        lm_weight, out, out_len, best_k, att, total, rescored, stream);
}

int ob_ctc_align_supported(int64_t Tp, int64_t S) { return ctc_align_supported(Tp, S) ? 1 : 0; }

size_t ob_ctc_align_workspace(int64_t B, int64_t Tp, int64_t S) {
  if (B < 0 || (B > 0 && Tp > 0 && B > INT32_MAX / Tp)) return 0;
  return ctc_align_workspace(B, Tp, S);
}

int ob_ctc_align_stage(const float* logits, const int64_t* lens, const int32_t* targets,
                       const int32_t* tlen, int64_t B, int64_t Tp, int64_t V, int64_t S, int blank,
                       int stage, void* ws, size_t ws_bytes, int32_t* path, int32_t* span,
                       double* tok_score, double* score, void* stream) {
  if (!ctc_align_supported(Tp, S) || B < 0 || V < 1 || V > INT32_MAX ||
      (B > 0 && (B > INT32_MAX / Tp || V > INT64_MAX / 4 / Tp / B)) || blank < 0 || blank >= V ||
      stage < 0 || stage > 3)
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  // stage -> launches: bit 0 the emission launch, bit 1 the recursion, bit 2 the walk + outputs
  const int stages = stage == 0 ? 7 : (stage == 1 ? 1 : (stage == 2 ? 6 : 2));
  const bool outs = (stages & 4) != 0;
  if (!lens || !tlen || !ws || ((stages & 1) && !logits) || ((stages & 2) && !score) ||
      (outs && !path) || (S > 0 && (!targets || (outs && (!span || !tok_score)))))
    return OB_ERR_NULL;
  if (!aligned4(logits) || !aligned4(targets) || !aligned4(tlen) || !aligned4(path) ||
      !aligned4(span) || misaligned8(lens) || misaligned8(ws) || misaligned8(tok_score) ||
      misaligned8(score))
    return OB_ERR_ALIGN;
  const size_t need = ctc_align_workspace(B, Tp, S);
  if (need == 0) return OB_ERR_SHAPE;
  if (ws_bytes < need) return OB_ERR_WORKSPACE;
  launch_ctc_align(logits, lens, reinterpret_cast<const int*>(targets),
                   reinterpret_cast<const int*>(tlen), B, Tp, V, S, blank, stages, ws,
                   reinterpret_cast<int*>(path), reinterpret_cast<int*>(span), tok_score, score,
                   as_stream(stream));
  return launched();
}

int ob_ctc_align(const float* logits, const int64_t* lens, const int32_t* targets,
                 const int32_t* tlen, int64_t B, int64_t Tp, int64_t V, int64_t S, int blank,
                 void* ws, size_t ws_bytes, int32_t* path, int32_t* span, double* tok_score,
                 double* score, void* stream) {
  return ob_ctc_align_stage(logits, lens, targets, tlen, B, Tp, V, S, blank, 0, ws, ws_bytes, path,
                            span, tok_score, score, stream);
}

int ob_edit_supported(int64_t La, int64_t Lb) { return edit_supported(La, Lb) ? 1 : 0; }

size_t ob_edit_distance_workspace(int64_t P, int64_t La, int64_t Lb) {
  return edit_distance_workspace(P, La, Lb);
}

int ob_edit_distance(const int32_t* a, const int32_t* a_len, const int32_t* b,
                     const int32_t* b_len, int64_t P, int64_t La, int64_t Lb, void* ws,
                     size_t ws_bytes, int32_t* dist, int32_t* ops, void* stream) {
  if (!edit_supported(La, Lb) || P < 0 || P > INT32_MAX) return OB_ERR_SHAPE;
  if (P == 0) return OB_OK;
  if (!a_len || !b_len || !dist || !ws || (La > 0 && !a) || (Lb > 0 && !b)) return OB_ERR_NULL;
  if (!aligned4(a) || !aligned4(a_len) || !aligned4(b) || !aligned4(b_len) || !aligned4(dist) ||
      !aligned4(ops) || misaligned8(ws))
    return OB_ERR_ALIGN;
  if (ws_bytes < edit_distance_workspace(P, La, Lb)) return OB_ERR_WORKSPACE;
  launch_edit_distance(reinterpret_cast<const int*>(a), reinterpret_cast<const int*>(a_len),
                       reinterpret_cast<const int*>(b), reinterpret_cast<const int*>(b_len), P, La,
                       Lb, ws, reinterpret_cast<int*>(dist), reinterpret_cast<int*>(ops),
                       as_stream(stream));
  return launched();
}

size_t ob_nbest_edit_distance_workspace(int64_t B, int64_t N, int64_t T, int64_t S) {
  return nbest_edit_distance_workspace(B, N, T, S);
}

int ob_nbest_edit_distance(const int32_t* hyp, const int32_t* hyp_len, const int32_t* n_hyp,
                           const int32_t* ref, const int32_t* ref_len, int64_t B, int64_t N,
                           int64_t T, int64_t S, void* ws, size_t ws_bytes, int32_t* dref,
                           int32_t* ops_ref, int32_t* dpair, void* stream) {
  if (!nbest_edit_supported(B, N, T, S)) return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  const bool with_ref = dref || ops_ref;
  if ((!with_ref && !dpair) || !hyp_len || !n_hyp || !ws || (T > 0 && !hyp) ||
      (with_ref && (!ref_len || (S > 0 && !ref))))
    return OB_ERR_NULL;
  if (!aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) || !aligned4(ref) ||
      !aligned4(ref_len) || !aligned4(dref) || !aligned4(ops_ref) || !aligned4(dpair) ||
      misaligned8(ws))
    return OB_ERR_ALIGN;
  if (ws_bytes < nbest_edit_distance_workspace(B, N, T, S)) return OB_ERR_WORKSPACE;
  launch_nbest_edit_distance(
      reinterpret_cast<const int*>(hyp), reinterpret_cast<const int*>(hyp_len),
      reinterpret_cast<const int*>(n_hyp), reinterpret_cast<const int*>(ref),
      reinterpret_cast<const int*>(ref_len), B, N, T, S, ws, reinterpret_cast<int*>(dref),
      reinterpret_cast<int*>(ops_ref), reinterpret_cast<int*>(dpair), as_stream(stream));
  return launched();
}

int ob_mbr_select(const int32_t* dpair, const int32_t* hyp, const int32_t* hyp_len,
                  const int32_t* n_hyp, const double* score, double scale, int64_t B, int64_t N,
                  int64_t T, int32_t* out, int32_t* out_len, int32_t* best_k, double* risk,
                  double* post, void* stream) {
  if (!nbest_edit_supported(B, N, T, 0) || !(scale >= 0.0) || !(scale <= DBL_MAX))
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!dpair || !hyp_len || !n_hyp || !score || !out_len || !best_k || !risk || !post ||
      (T > 0 && (!hyp || !out)))
    return OB_ERR_NULL;
  if (!aligned4(dpair) || !aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) ||
      !aligned4(out) || !aligned4(out_len) || !aligned4(best_k) || misaligned8(score) ||
      misaligned8(risk) || misaligned8(post))
    return OB_ERR_ALIGN;
  launch_mbr_select(reinterpret_cast<const int*>(dpair), reinterpret_cast<const int*>(hyp),
                    reinterpret_cast<const int*>(hyp_len), reinterpret_cast<const int*>(n_hyp),
                    score, scale, B, N, T, reinterpret_cast<int*>(out),
                    reinterpret_cast<int*>(out_len), reinterpret_cast<int*>(best_k), risk, post,
                    as_stream(stream));
  return launched();
}

int ob_ctc_nbest_supported(int64_t N, int64_t Th) { return ctc_nbest_supported(N, Th) ? 1 : 0; }

namespace {
bool ctc_nbest_shape_ok(int64_t B, int64_t N, int64_t T, int64_t Th) {
  return ctc_nbest_supported(N, Th) && B >= 1 && T >= 1 && B <= INT32_MAX / T &&
         B * T <= INT32_MAX / N;
}

int ctc_nbest_check(const float* x, const int64_t* lens, const int32_t* hyp,
                    const int32_t* hyp_len, const int32_t* n_hyp, int64_t B, int64_t N, int64_t T,
                    int64_t V, int64_t Th, int blank, const void* ws, size_t ws_bytes,
                    const void* out, bool more_null, bool more_misaligned) {
  if (!ctc_nbest_shape_ok(B, N, T, Th) || V < 1 || V > INT32_MAX || blank < 0 || blank >= V)
    return OB_ERR_SHAPE;
  if (!x || !lens || !hyp_len || !n_hyp || !ws || !out || (Th > 0 && !hyp) || more_null)
    return OB_ERR_NULL;
  if (more_misaligned || !aligned4(x) || !aligned4(hyp) || !aligned4(hyp_len) || !aligned4(n_hyp) ||
      misaligned8(lens) || (reinterpret_cast<uintptr_t>(ws) & 255) ||
      ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(x) & 15)))
    return OB_ERR_ALIGN;
  if (ws_bytes < ctc_nbest_workspace(B, N, T, Th)) return OB_ERR_WORKSPACE;
  return OB_OK;
}
}  // namespace

size_t ob_ctc_nbest_workspace(int64_t B, int64_t N, int64_t T, int64_t Th) {
  if (!ctc_nbest_shape_ok(B, N, T, Th)) return 0;
  return ctc_nbest_workspace(B, N, T, Th);
}

int ob_ctc_nbest_logprob(const float* logits, const int64_t* lens, const int32_t* hyp,
                         const int32_t* hyp_len, const int32_t* n_hyp, int64_t B, int64_t N,
                         int64_t T, int64_t V, int64_t Th, int blank, void* ws, size_t ws_bytes,
                         double* ll, void* stream) {
  if (int st = ctc_nbest_check(logits, lens, hyp, hyp_len, n_hyp, B, N, T, V, Th, blank, ws,
                               ws_bytes, ll, false, misaligned8(ll)))
    return st;
  launch_ctc_nbest_logprob(logits, lens, reinterpret_cast<const int*>(hyp),
                           reinterpret_cast<const int*>(hyp_len),
                           reinterpret_cast<const int*>(n_hyp), B, N, T, V, Th, blank, ws, ll,
                           as_stream(stream));
  return launched();
}

int ob_mwer_combine(const double* ll, const double* err, const int32_t* n_hyp, double scale,
                    int64_t B, int64_t N, double* loss, double* post, double* risk, double* coef,
                    void* stream) {
  if (!ctc_nbest_supported(N, 0) || B < 1 || B > INT32_MAX / N || !(scale >= 0.0) ||
      !(scale <= DBL_MAX))
    return OB_ERR_SHAPE;
  if (!ll || !err || !n_hyp || !loss || !post || !risk || !coef) return OB_ERR_NULL;
  if (!aligned4(n_hyp) || misaligned8(ll) || misaligned8(err) || misaligned8(loss) ||
      misaligned8(post) || misaligned8(risk) || misaligned8(coef))
    return OB_ERR_ALIGN;
  launch_mwer_combine(ll, err, reinterpret_cast<const int*>(n_hyp), scale, B, N, loss, post, risk,
                      coef, as_stream(stream));
  return launched();
}

int ob_ctc_nbest_grad(const float* logits, const int64_t* lens, const int32_t* hyp,
                      const int32_t* hyp_len, const int32_t* n_hyp, int64_t B, int64_t N,
                      int64_t T, int64_t V, int64_t Th, int blank, const double* coef,
                      const float* grad_out, int dense, void* ws, size_t ws_bytes, float* grad,
                      void* stream) {
  if (int st = ctc_nbest_check(logits, lens, hyp, hyp_len, n_hyp, B, N, T, V, Th, blank, ws,
                               ws_bytes, grad, !coef,
                               misaligned8(coef) || !aligned4(grad_out) || !aligned4(grad) ||
                                   ((V & 3) == 0 && (reinterpret_cast<uintptr_t>(grad) & 15))))
    return st;
  launch_ctc_nbest_grad(logits, lens, reinterpret_cast<const int*>(hyp), B, N, T, V, Th, blank,
                        coef, grad_out, dense, ws, grad, as_stream(stream));
  return launched();
}

int64_t ob_fbank_num_frames(int64_t n_samples) { return fbank_num_frames(n_samples); }

int64_t ob_frontend_table_floats(int n_mels) {
  return (n_mels < 1 || n_mels > 128) ? 0 : frontend_table_floats(n_mels);
}

int ob_frontend_table_fill(float* host_table, int n_mels) {
  if (n_mels < 1 || n_mels > 128) return OB_ERR_SHAPE;
  if (!host_table) return OB_ERR_NULL;
  if (!aligned4(host_table)) return OB_ERR_ALIGN;
  frontend_table_fill(host_table, n_mels);
  return OB_OK;
}

int ob_frontend_fwd(const float* wave, int64_t wave_stride, const int64_t* wave_lens, int64_t B,
                    int64_t n_max, const float* table, int n_mels, const float* cmvn_mean,
                    const float* cmvn_std, const int32_t* mask_starts, int n_fmask, int fmask_w,
                    int n_tmask, int tmask_w, float* feats, int64_t T, int64_t* feat_lens,
                    void* stream) {
  if (n_mels < 1 || n_mels > 128 || B < 0 || n_max < 0 || wave_stride < n_max || T < 0 ||
      T < fbank_num_frames(n_max) || n_fmask < 0 || fmask_w < 0 || n_tmask < 0 || tmask_w < 0 ||
      T > INT64_MAX / 128 / (B > 0 ? B : 1) || wave_stride > INT64_MAX / 4 / (B > 0 ? B : 1) ||
      frontend_blocks(B, T) > INT32_MAX)
    return OB_ERR_SHAPE;
  if (B == 0) return OB_OK;
  if (!wave_lens || !table || !feat_lens || (n_max > 0 && !wave) || (T > 0 && !feats) ||
      (cmvn_mean == nullptr) != (cmvn_std == nullptr))
    return OB_ERR_NULL;
  if (!aligned4(wave) || !aligned4(table) || !aligned4(cmvn_mean) || !aligned4(cmvn_std) ||
      !aligned4(mask_starts) || !aligned4(feats) || (reinterpret_cast<uintptr_t>(wave_lens) & 7) ||
      (reinterpret_cast<uintptr_t>(feat_lens) & 7))
    return OB_ERR_ALIGN;
  launch_frontend(wave, wave_stride, wave_lens, B, n_max, table, n_mels, cmvn_mean, cmvn_std,
                  reinterpret_cast<const int*>(mask_starts), n_fmask, fmask_w, n_tmask, tmask_w,
                  feats, T, feat_lens, as_stream(stream));
  return launched();
}

int ob_layernorm_fwd(const float* x, const float* gamma, const float* beta, int64_t rows,
                     int64_t d, float eps, float* y, float* mean, float* rstd, void* stream) {
  if (rows < 0 || !layernorm_supported(d) || !(eps >= 0.0f)) return OB_ERR_SHAPE;
  if (rows > 0 && (!x || !y)) return OB_ERR_NULL;
  if (!aligned4(x) || !aligned4(y) || !aligned4(gamma) || !aligned4(beta)) return OB_ERR_ALIGN;
  launch_layernorm_fwd(x, gamma, beta, rows, d, eps, y, mean, rstd, as_stream(stream));
  return launched();
}

int ob_layernorm_fwd_pair(const float* x, const float* g1, const float* b1, const float* g2,
                          const float* b2, int64_t rows, int64_t d, float eps1, float eps2,
                          float* y1, float* mean1, float* rstd1, float* y2, float* mean2,
                          float* rstd2, void* stream) {
  if (rows < 0 || !layernorm_supported(d) || !(eps1 >= 0.0f) || !(eps2 >= 0.0f))
    return OB_ERR_SHAPE;
  if (rows > 0 && (!x || !y1 || !y2)) return OB_ERR_NULL;
  if (!aligned4(x) || !aligned4(y1) || !aligned4(y2) || !aligned4(g1) || !aligned4(b1) ||
      !aligned4(g2) || !aligned4(b2))
    return OB_ERR_ALIGN;
  launch_layernorm_fwd_pair(x, g1, b1, g2, b2, rows, d, eps1, eps2, y1, mean1, rstd1, y2, mean2,
                            rstd2, as_stream(stream));
  return launched();
}

size_t ob_layernorm_fwd_amax_workspace(int64_t P) {
  return (P < 1 || P > 8) ? 0 : layernorm_fwd_amax_workspace(P);
}

int ob_layernorm_fwd_amax(const float* x, const float* gamma, const float* beta, int64_t rows,
                          int64_t d, float eps, float* y, float* mean, float* rstd, int64_t P,
                          float* amax, void* ws, size_t ws_bytes, void* stream) {
  if (rows < 0 || !layernorm_supported(d) || !(eps >= 0.0f) || P < 1 || P > 8 || rows % P)
    return OB_ERR_SHAPE;
  if ((rows > 0 && (!x || !y)) || !amax || !ws) return OB_ERR_NULL;
  if (ws_bytes < layernorm_fwd_amax_workspace(P)) return OB_ERR_WORKSPACE;
  if (!aligned4(x) || !aligned4(y) || !aligned4(gamma) || !aligned4(beta) || !aligned4(amax))
    return OB_ERR_ALIGN;
  launch_layernorm_fwd_amax(x, gamma, beta, rows, d, eps, y, mean, rstd, (int)P, amax, ws,
                            as_stream(stream));
  return launched();
}

int ob_layernorm_fwd_i8(const float* x, const float* gamma, const float* beta, int64_t rows,
                        int64_t d, float eps, int64_t P, float* amax, int8_t* yq, void* ws,
                        size_t ws_bytes, void* stream) {
  if (rows < 0 || !layernorm_supported(d) || !(eps >= 0.0f) || P < 1 || P > 8 || rows % P)
    return OB_ERR_SHAPE;
  if ((rows > 0 && (!x || !yq)) || !amax || !ws) return OB_ERR_NULL;
  if (ws_bytes < layernorm_fwd_amax_workspace(P)) return OB_ERR_WORKSPACE;
  if (!aligned4(x) || !aligned4(yq) || !aligned4(gamma) || !aligned4(beta) || !aligned4(amax))
    return OB_ERR_ALIGN;
  launch_layernorm_fwd_i8(x, gamma, beta, rows, d, eps, (int)P, amax, yq, ws, as_stream(stream));
  return launched();
}

size_t ob_layernorm_bwd_workspace(int64_t rows, int64_t d) {
  if (rows < 0 || !layernorm_supported(d)) return 0;
  return layernorm_bwd_workspace(rows, d);
}

int ob_layernorm_bwd(const float* dy, const float* x, const float* gamma, const float* mean,
                     const float* rstd, int64_t rows, int64_t d, float* dx, float* dgamma,
                     float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (rows < 0 || !layernorm_supported(d)) return OB_ERR_SHAPE;
  if (rows > 0 && (!dy || !x || !mean || !rstd || !dx)) return OB_ERR_NULL;
  if ((dgamma || dbeta) && !ws) return OB_ERR_NULL;
  if ((dgamma || dbeta) && ws_bytes < layernorm_bwd_workspace(rows, d)) return OB_ERR_WORKSPACE;
  if (!aligned4(dy) || !aligned4(x) || !aligned4(dx)) return OB_ERR_ALIGN;
  launch_layernorm_bwd(dy, x, gamma, mean, rstd, rows, d, nullptr, dx, dgamma, dbeta, ws,
                       as_stream(stream));
  return launched();
}

int ob_layernorm_bwd_res(const float* dy, const float* x, const float* gamma, const float* mean,
                         const float* rstd, int64_t rows, int64_t d, const float* dres, float* dx,
                         float* dgamma, float* dbeta, void* ws, size_t ws_bytes, void* stream) {
  if (rows < 0 || !layernorm_supported(d)) return OB_ERR_SHAPE;
  if (rows > 0 && (!dy || !x || !mean || !rstd || !dx || !dres)) return OB_ERR_NULL;
  if ((dgamma || dbeta) && !ws) return OB_ERR_NULL;
  if ((dgamma || dbeta) && ws_bytes < layernorm_bwd_workspace(rows, d)) return OB_ERR_WORKSPACE;
  if (!aligned4(dy) || !aligned4(x) || !aligned4(dx) || !aligned4(dres)) return OB_ERR_ALIGN;
  launch_layernorm_bwd(dy, x, gamma, mean, rstd, rows, d, dres, dx, dgamma, dbeta, ws,
                       as_stream(stream));
  return launched();
}

int ob_layernorm_bwd_ex(const float* dy, const float* x, const float* gamma, const float* mean,
                        const float* rstd, int64_t rows, int64_t d, const float* dres, float* dx,
                        float* dgamma, float* dbeta, void* ws, size_t ws_bytes, float* dy2,
                        float rscale, float p_drop, const uint64_t* rng, int64_t rng_offset,
                        const int32_t* lens, int64_t T, void* stream) {
  return ob_layernorm_bwd_defer(dy, x, gamma, mean, rstd, rows, d, dres, dx, dgamma, dbeta, ws,
                                ws_bytes, dy2, rscale, p_drop, rng, rng_offset, lens, T, nullptr,
                                0, stream);
}

size_t ob_ln_param_entry_bytes(void) { return sizeof(LnParamEntry); }

int ob_ln_param_table(const void* table, int64_t n, int64_t dmax, void* stream) {
  if (n < 0 || dmax < 0 || dmax > 512) return OB_ERR_SHAPE;
  if (n > 0 && !table) return OB_ERR_NULL;
  launch_ln_param_table(static_cast<const LnParamEntry*>(table), (int)n, (int)dmax,
                        as_stream(stream));
  return launched();
}

size_t ob_layernorm_bwd_pair_workspace(int64_t rows, int64_t d) {
  if (rows < 0 || !layernorm_supported(d)) return 0;
  return 2 * layernorm_bwd_workspace(rows, d);
}

int ob_layernorm_bwd_pair(const float* dy, const float* y1, const float* g2, const float* mean2,
                          const float* rstd2, const float* gres, const float* x, const float* g1,
                          const float* mean1, const float* rstd1, int64_t rows, int64_t d,
                          float* dx, float* dg2, float* db2, float* dg1, float* db1, void* ws,
                          size_t ws_bytes, float* dy2, float rscale, float p_drop,
                          const uint64_t* rng, int64_t rng_offset, const int32_t* lens, int64_t T,
                          void* table, int64_t slot2, int64_t slot1, void* stream) {
  if (rows < 0 || !layernorm_supported(d) || !(p_drop >= 0.0f && p_drop < 1.0f))
    return OB_ERR_SHAPE;
  if (rows > 0 && (!dy || !y1 || !mean2 || !rstd2 || !x || !mean1 || !rstd1 || !dx || !ws))
    return OB_ERR_NULL;
  if (dy2 && p_drop > 0.0f && !rng) return OB_ERR_NULL;
  if (ws_bytes < 2 * layernorm_bwd_workspace(rows, d)) return OB_ERR_WORKSPACE;
  if (!aligned4(dy) || !aligned4(y1) || !aligned4(gres) || !aligned4(x) || !aligned4(dx) ||
      !aligned4(dy2) || !aligned4(g1) || !aligned4(g2) || !aligned4(lens) || ((uintptr_t)ws & 15))
    return OB_ERR_ALIGN;
  // (as ob_layernorm_bwd_defer: the kernel indexes lens[row / T], lens being [rows / T])
  if (dy2 && lens && (T < 1 || T > 0x7fffffff || rows % T)) return OB_ERR_SHAPE;
  LnGradScale gsc{dy2, rscale, p_drop, rng, (uint64_t)rng_offset, lens, (int)T};
  LnParamEntry* tab = static_cast<LnParamEntry*>(table);
  const LnDefer f2{tab && slot2 >= 0 ? tab : nullptr, (int)slot2};
  const LnDefer f1{tab && slot1 >= 0 ? tab : nullptr, (int)slot1};
  launch_layernorm_bwd_pair(dy, y1, g2, mean2, rstd2, gres, x, g1, mean1, rstd1, rows, d, dx, dg2,
                            db2, dg1, db1, ws, as_stream(stream), dy2 ? &gsc : nullptr, &f2, &f1);
  return launched();
}

int ob_layernorm_bwd_defer(const float* dy, const float* x, const float* gamma, const float* mean,
                           const float* rstd, int64_t rows, int64_t d, const float* dres,
                           float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                           float* dy2, float rscale, float p_drop, const uint64_t* rng,
                           int64_t rng_offset, const int32_t* lens, int64_t T, void* table,
                           int64_t slot, void* stream) {
  if (table && slot < 0) return OB_ERR_SHAPE;
  if (rows < 0 || !layernorm_supported(d)) return OB_ERR_SHAPE;
  if (rows > 0 && (!dy || !x || !mean || !rstd || !dx)) return OB_ERR_NULL;
  if ((dgamma || dbeta) && !ws) return OB_ERR_NULL;
  if ((dgamma || dbeta) && ws_bytes < layernorm_bwd_workspace(rows, d)) return OB_ERR_WORKSPACE;
  if (!aligned4(dy) || !aligned4(x) || !aligned4(dx) || !aligned4(dres) || !aligned4(dy2) ||
      !aligned4(lens))
    return OB_ERR_ALIGN;
  if (dy2) {
    if (!(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
    if (lens && (T < 1 || T > 0x7fffffff || rows % T)) return OB_ERR_SHAPE;
    if (p_drop > 0.0f && !rng) return OB_ERR_NULL;
  }
  LnGradScale gs{dy2, rscale, p_drop, rng, (uint64_t)rng_offset,
                 reinterpret_cast<const int*>(lens), (int)T};
  const LnDefer df{static_cast<LnParamEntry*>(table), (int)slot};
  launch_layernorm_bwd(dy, x, gamma, mean, rstd, rows, d, dres, dx, dgamma, dbeta, ws,
                       as_stream(stream), &gs, &df);
  return launched();
}

namespace {
int relattn_check(int64_t Bt, int64_t P, int64_t T, int64_t H, int64_t d, float p_drop) {
  if (Bt < 1 || P < 1 || Bt % P != 0 || H < 1 || !relattn_supported(T, d)) return OB_ERR_SHAPE;
  if (Bt > 65535 || H > 65535 || !(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  return OB_OK;
}
}  // namespace

int ob_relattn_fwd(const float* q, const float* k, const float* v, const float* pos,
                   const float* u, const float* vb, const int32_t* lens, int64_t Bt, int64_t P,
                   int64_t T, int64_t H, int64_t d, float p_drop, const int64_t* rng,
                   int64_t rng_offset, float* saved, float* probs, float* ctx, void* stream) {
  if (int st = relattn_check(Bt, P, T, H, d, p_drop)) return st;
  if (!q || !k || !v || !pos || !u || !vb || !lens || !ctx || (p_drop > 0.0f && !rng))
    return OB_ERR_NULL;
  if (((uintptr_t)saved & 15) || ((uintptr_t)probs & 15)) return OB_ERR_ALIGN;
  launch_relattn_fwd(q, k, v, pos, u, vb, lens, Bt, P, T, H, d, p_drop,
                     reinterpret_cast<const uint64_t*>(rng), (uint64_t)rng_offset, saved, probs,
                     ctx, as_stream(stream));
  return launched();
}

int ob_relattn_infer(const float* q, const float* k, const float* v, const float* pos,
                     const float* u, const float* vb, const int32_t* lens, int64_t Bt, int64_t P,
                     int64_t T, int64_t H, int64_t d, float* ctx, void* stream) {
  if (Bt < 1 || P < 1 || Bt % P != 0 || H < 1 || Bt > 65535 || H > 65535 ||
      !relattn_long_supported(T, H, d))
    return OB_ERR_SHAPE;
  if (!q || !k || !v || !pos || !u || !vb || !lens || !ctx) return OB_ERR_NULL;
  launch_relattn_long(q, k, v, pos, u, vb, lens, Bt, P, T, H, d, ctx, as_stream(stream));
  return launched();
}

int64_t ob_relattn_infer_key_chunk(void) { return relattn_long_key_chunk(); }
int64_t ob_relattn_infer_max_t(void) { return relattn_long_max_t(); }

int64_t ob_relattn_saved_elems(int64_t Bt, int64_t T, int64_t H, int64_t d) {
  if (Bt < 1 || H < 1 || !relattn_supported(T, d)) return 0;
  return relattn_saved_elems(Bt, T, H, d);
}

size_t ob_relattn_bwd_workspace(int64_t Bt, int64_t T, int64_t H, int64_t d) {
  if (Bt < 1 || H < 1 || !relattn_supported(T, d)) return 0;
  return align_up(relattn_bwd_workspace(Bt, T, H, d));
}

int ob_relattn_set_bwd_mode(int mode) { return relattn_set_flash(mode); }

int ob_tgemm_set_colloop(int on) { return tgemm_set_colloop(on); }

int ob_relattn_set_kv_ring(int on) { return relattn_set_kv_ring(on); }
int ob_relattn_set_windows(int mask) { return relattn_set_windows(mask); }

int64_t ob_relattn_probs_elems(int64_t Bt, int64_t T, int64_t H) {
  if (Bt < 1 || H < 1 || T < 1) return 0;
  return relattn_probs_elems(Bt, T, H);
}

int ob_relattn_bwd(const float* dctx, const float* ctx, const float* q, const float* k,
                   const float* v, const float* pos, const float* u, const float* vb,
                   const int32_t* lens, int64_t Bt, int64_t P, int64_t T, int64_t H, int64_t d,
                   float p_drop, const int64_t* rng, int64_t rng_offset, const float* saved,
                   int64_t saved_elems, float* dq, float* dk, float* dv, float* dpos, float* du,
                   float* dvb, void* ws, size_t ws_bytes, void* stream) {
  if (int st = relattn_check(Bt, P, T, H, d, p_drop)) return st;
  if (!dctx || !ctx || !q || !k || !v || !pos || !u || !vb || !lens || !saved || !dq || !dk ||
      !dv || !dpos || !du || !dvb || !ws)
    return OB_ERR_NULL;
  // `saved` laid out under the other backward mode (ob_relattn_set_bwd_mode in between)
  if (saved_elems != relattn_saved_elems(Bt, T, H, d)) return OB_ERR_SHAPE;
  (void)rng;  // the forward's keep decisions are in the saved state
  (void)rng_offset;
  if ((uintptr_t)saved & 15) return OB_ERR_ALIGN;
  if (ws_bytes < ob_relattn_bwd_workspace(Bt, T, H, d)) return OB_ERR_WORKSPACE;
  launch_relattn_bwd(dctx, ctx, q, k, v, pos, u, vb, lens, Bt, P, T, H, d, p_drop, saved, dq, dk,
                     dv, dpos, du, dvb, ws, as_stream(stream));
  return launched();
}

int ob_decattn_supported(int64_t Lq, int64_t Lk, int64_t dh) {
  return decattn_supported(Lq, Lk, dh) ? 1 : 0;
}

static int decattn_check(int64_t B, int64_t H, int64_t Lq, int64_t Lk, int64_t dh, int64_t sq,
                         int64_t sk, int64_t sv, float p_drop) {
  if (B < 0 || H < 1 || !decattn_supported(Lq, Lk, dh) || !(p_drop >= 0.0f && p_drop < 1.0f))
    return OB_ERR_SHAPE;
  if (sq < H * dh || sk < H * dh || sv < H * dh) return OB_ERR_SHAPE;
  if (B * H * Lq > INT32_MAX) return OB_ERR_SHAPE;
  return OB_OK;
}

int ob_decattn_fwd(const float* q, int64_t sq, const float* k, int64_t sk, const float* v,
                   int64_t sv, const uint8_t* kmask, int64_t causal, int64_t B, int64_t H,
                   int64_t Lq, int64_t Lk, int64_t dh, float p_drop, const int64_t* rng,
                   int64_t rng_offset, float* probs, float* ctx, void* stream) {
  if (int st = decattn_check(B, H, Lq, Lk, dh, sq, sk, sv, p_drop)) return st;
  if (B > 0 && (!q || !k || !v || !probs || !ctx || (p_drop > 0.0f && !rng))) return OB_ERR_NULL;
  if (!aligned4(q) || !aligned4(k) || !aligned4(v) || !aligned4(probs) ||
      (reinterpret_cast<uintptr_t>(ctx) & 15))
    return OB_ERR_ALIGN;
  launch_decattn_fwd(q, sq, k, sk, v, sv, kmask, causal ? 1 : 0, B, H, Lq, Lk, dh, p_drop,
                     reinterpret_cast<const uint64_t*>(rng), (uint64_t)rng_offset, probs, ctx,
                     as_stream(stream));
  return launched();
}

int ob_decattn_fwd_grouped(const float* q, int64_t sq, const float* k, int64_t sk, const float* v,
                           int64_t sv, const uint8_t* kmask, int64_t causal, int64_t B,
                           int64_t kv_group, int64_t H, int64_t Lq, int64_t Lk, int64_t dh,
                           float* ctx, void* stream) {
  if (kv_group < 1 || B < 0 || (B > 0 && kv_group > INT32_MAX / B)) return OB_ERR_SHAPE;
  if (int st = decattn_check(B * kv_group, H, Lq, Lk, dh, sq, sk, sv, 0.0f)) return st;
  if (B > 0 && (!q || !k || !v || !ctx)) return OB_ERR_NULL;
  if (!aligned4(q) || !aligned4(k) || !aligned4(v) || (reinterpret_cast<uintptr_t>(ctx) & 15))
    return OB_ERR_ALIGN;
  launch_decattn_fwd_grouped(q, sq, k, sk, v, sv, kmask, causal ? 1 : 0, B, kv_group, H, Lq, Lk,
                             dh, ctx, as_stream(stream));
  return launched();
}

int ob_decattn_bwd(const float* dctx, const float* ctx, const float* q, int64_t sq, const float* k,
                   int64_t sk, const float* v, int64_t sv, int64_t B, int64_t H, int64_t Lq, int64_t Lk,
                   int64_t dh, float p_drop, float* probs, float* dq, int64_t gq, float* dk,
                   int64_t gk, float* dv, int64_t gv, void* stream) {
  if (int st = decattn_check(B, H, Lq, Lk, dh, sq, sk, sv, p_drop)) return st;
  if (gq < H * dh || gk < H * dh || gv < H * dh) return OB_ERR_SHAPE;
  if (B > 0 && (!dctx || !ctx || !q || !k || !v || !probs || !dq || !dk || !dv)) return OB_ERR_NULL;
  if (!aligned4(ctx) || !aligned4(dctx) || !aligned4(q) || !aligned4(k) || !aligned4(v) || !aligned4(probs) ||
      !aligned4(dq) || !aligned4(dk) || !aligned4(dv))
    return OB_ERR_ALIGN;
  launch_decattn_bwd(dctx, ctx, q, sq, k, sk, v, sv, B, H, Lq, Lk, dh, p_drop, probs, dq, gq, dk, gk,
                     dv, gv, as_stream(stream));
  return launched();
}

int ob_relattn_dropout_mask(int64_t n, int64_t row_len, float p_drop, const int64_t* rng,
                            int64_t rng_offset, uint8_t* out, void* stream) {
  if (n < 0 || row_len < 1 || !(p_drop >= 0.0f && p_drop < 1.0f)) return OB_ERR_SHAPE;
  if ((n > 0 && !out) || (p_drop > 0.0f && !rng)) return OB_ERR_NULL;
  launch_relattn_dropout_mask(n, row_len, p_drop, reinterpret_cast<const uint64_t*>(rng),
                              (uint64_t)rng_offset, out, as_stream(stream));
  return launched();
}

int ob_embedding_bwd(const int64_t* indices, int64_t N, const float* grad, int64_t C,
                     int64_t V, int64_t padding_idx, float* grad_weight, void* stream) {
  if (N < 0 || V < 0 || !embed_supported(C) || padding_idx >= V) return OB_ERR_SHAPE;
  if ((N > 0 && (!indices || !grad)) || (V > 0 && !grad_weight)) return OB_ERR_NULL;
  if (!aligned4(grad) || !aligned4(grad_weight)) return OB_ERR_ALIGN;
  launch_embed_bwd(indices, N, grad, C, V, padding_idx, grad_weight, as_stream(stream));
  return launched();
}

int64_t ob_adamw_plan(const int64_t* numels, int64_t n_tensors, int64_t* chunk_map) {
  if (!numels || n_tensors < 1) return OB_ERR_SHAPE;
  for (int64_t t = 0; t < n_tensors; ++t)
    if (numels[t] < 1) return OB_ERR_SHAPE;
  return adamw_plan(numels, n_tensors, chunk_map);
}

size_t ob_adamw_workspace(int64_t n_blocks) {
  if (n_blocks < 1) return 0;
  return align_up(adamw_workspace(n_blocks));
}

int ob_adamw_clip_step(const ob_adamw_tensor* table, int64_t n_tensors, const int64_t* chunk_map,
                       int64_t n_blocks, const float* lr, float* step, float grad_scale,
                       double beta1, double beta2, double eps, double weight_decay,
                       double max_norm, float* total_norm,
                       void* ws, size_t ws_bytes, void* stream) {
  static_assert(sizeof(ob_adamw_tensor) == sizeof(AdamwTensor), "table layout");
  if (n_tensors < 1 || n_blocks < 1 || n_blocks > 0x7fffffff) return OB_ERR_SHAPE;
  if (!table || !chunk_map || !lr || !step || !ws) return OB_ERR_NULL;
  if (ws_bytes < ob_adamw_workspace(n_blocks)) return OB_ERR_WORKSPACE;
  launch_adamw(reinterpret_cast<const AdamwTensor*>(table), chunk_map, n_blocks, lr, step,
               grad_scale, beta1, beta2, eps, weight_decay, max_norm, total_norm, ws,
               as_stream(stream));
  return launched();
}

}  // extern "C"
