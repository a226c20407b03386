/*
 * onebit_hip.h — C ABI of the MI355X (gfx950) BitLinear / QuantizedLinear hot path.
 *
 * This is the drop-in boundary for the reference's quantized linear layer
 * (y00njaekim/CMU-11785-IDL-1.58bit-ASR, onebit_asr/quant.py). The reference is
 * pure Python over torch eager ops; each entry point below replaces the torch
 * op sequence cited next to it. The Python host side
 * (cmu-11785-idl-1.58bit-asr_amd/onebit_asr/quant.py) binds these with ctypes.
 *
 * Conventions (all entry points):
 *   - plain C types only: device pointers, int64 sizes, a hipStream_t passed as void*;
 *   - every tensor is dense row-major fp32 (last dim contiguous) unless stated;
 *   - caller owns every buffer, including workspaces; nothing here allocates,
 *     synchronises the device or copies to/from the host, so every call is legal
 *     inside hipStreamBeginCapture/hipGraph capture;
 *   - return value: OB_OK (0) or a negative OB_ERR_* status; no exceptions cross
 *     the ABI; launch failures are reported as OB_ERR_HIP;
 *   - alpha is a DEVICE pointer to one fp32. With alpha_raw = 1 it is the raw
 *     learnable parameter and the kernels use a = |alpha| + 1e-8f exactly as
 *     QuantizedLinear.forward does (quant.py:124); with alpha_raw = 0 it is used
 *     as given (the quantize_weight(W, alpha, bits) entry, quant.py:95-96).
 *   - quant-off ceiling (BASELINE configs[3]: BitLinear -> bf16 nn.Linear): on the GEMM
 *     entries (ob_bitlinear_fwd*, ob_bitlinear_bwd_dx*), alpha_raw = 2 makes each codes
 *     argument a bf16 weight image (uint16 [N][K] = bf16(W) for the forward entries, [K][N]
 *     = bf16(W^T) for the dX entries' codes_t; ob_pack_item bits = 16 packs both) and the
 *     GEMM's B operand that image, with no alpha scale (activations stay exact fp32, as in
 *     every entry). Same kernels, tiles and fused epilogues as the ternary path.
 *   - bits is 1 (binary {-1,+1}, zero -> +1) or 2 (ternary {-1,0,+1}, threshold 0.5)
 *     (quant.py:52-60). bits = 32 is the full-precision passthrough and never
 *     reaches this library (quant.py:121-122); any other value -> OB_ERR_BITWIDTH,
 *     which the host maps to ValueError("bitwidth must be one of {1,2,32}")
 *     (quant.py:65-66).
 *
 * Packed weight codes (2 bits / weight, 16 per uint32, little-end first):
 *   00 -> 0, 01 -> +1, 11 -> -1 (10 unused).
 *   codes   [N][ceil(K/16)] : code of W[n][16*w + j] in bits 2j..2j+1 of codes[n][w]
 *   codes_t [K][ceil(N/16)] : code of W[16*w + j][k] in bits 2j..2j+1 of codes_t[k][w]
 *   Padding positions hold 00.
 */
#ifndef ONEBIT_HIP_H_
#define ONEBIT_HIP_H_

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define OB_API __attribute__((visibility("default")))

enum {
  OB_OK = 0,
  OB_ERR_NULL = -1,      /* a required pointer is NULL */
  OB_ERR_SHAPE = -2,     /* negative / inconsistent size */
  OB_ERR_BITWIDTH = -3,  /* bits not in {1,2} */
  OB_ERR_WORKSPACE = -4, /* workspace smaller than the *_workspace() query */
  OB_ERR_ALIGN = -5,     /* pointer not 4-byte aligned */
  OB_ERR_HIP = -6        /* hipGetLastError() after launch was not hipSuccess */
};

/* ABI version (bumped on any signature change). */
OB_API int ob_abi_version(void);
/* sha256 (hex) of the sources the library was built from (the .hip / .h files of csrc/ and
 * the headers of include/; onebit_asr/_digest.py), generated at build time: the host side refuses a
 * library whose digest differs from the sources beside it. */
OB_API const char* ob_source_digest(void);
/* Static string for a status code. */
OB_API const char* ob_status_string(int status);

/*
 * Quantize + pack (replaces _QuantizeSTE.forward's quantization, quant.py:49-60,
 * without materialising W_hat): codes and codes_t from W[N][K] and alpha.
 * Either output may be NULL to skip it.
 */
OB_API int ob_quant_pack(const float* W, const float* alpha, int alpha_raw, int bits,
                         int64_t N, int64_t K, uint32_t* codes, uint32_t* codes_t,
                         void* stream);

/*
 * Grouped pack: ob_quant_pack over a whole model's (layer, bitwidth) items in ONE launch
 * (the reference quantizes each QuantizedLinear inside its own forward, quant.py:123-126;
 * at Conformer-S a step needs 144 layers x 2 bitwidths). `items` is a DEVICE array of
 * n_items descriptors in block order: items[0].block0 = 0 and
 * items[i+1].block0 = items[i].block0 + ob_quant_pack_item_blocks(N_i, K_i);
 * total_blocks = the sum over all items. The table is built once (it holds the
 * persistent parameter and code buffer addresses) and the call is capture-safe.
 */
typedef struct ob_pack_item {
  const float* W;      /* [N][K] */
  const float* alpha;  /* 1 fp32, device */
  uint32_t* codes;     /* [N][ceil(K/16)] */
  uint32_t* codes_t;   /* [K][ceil(N/16)] */
  int64_t N, K;
  int64_t block0;      /* first block of this item */
  int32_t bits;        /* 1 or 2; 16: bf16 weight images (quant-off), codes <- uint16 [N][K]
                          bf16(W), codes_t <- uint16 [K][N] bf16(W^T), block count from
                          ob_weight_bf16_item_blocks */
  int32_t alpha_raw;
} ob_pack_item;

OB_API int64_t ob_quant_pack_item_blocks(int64_t N, int64_t K);
OB_API int64_t ob_weight_bf16_item_blocks(int64_t N, int64_t K);
OB_API int ob_quant_pack_group(const ob_pack_item* items, int n_items, int64_t total_blocks,
                               void* stream);

/*
 * quantize_weight forward, elementwise (quant.py:49-70): W_hat[i] = a * Q(W[i]/a).
 */
OB_API int ob_quant_dequant(const float* W, const float* alpha, int alpha_raw, int bits,
                            int64_t n, float* W_hat, void* stream);

/*
 * quantize_weight backward (quant.py:72-92): grad_W = g * 1[|W/a| <= 1];
 * grad_alpha[0] = sum(g * term(W/a)) (times sign(alpha) when alpha_raw = 1,
 * i.e. the chain through alpha.abs() at quant.py:124). Deterministic.
 */
OB_API size_t ob_quant_ste_bwd_workspace(int64_t n);
OB_API int ob_quant_ste_bwd(const float* grad_W_hat, const float* W, const float* alpha,
                            int alpha_raw, int bits, int64_t n, float* grad_W,
                            float* grad_alpha, void* ws, size_t ws_bytes, void* stream);

/*
 * BitLinear forward (replaces F.linear(x, alpha*Q, bias), quant.py:124-126):
 *   Y[M][N] = a * (X[M][K] . Q^T) + bias        (bias may be NULL)
 */
OB_API int ob_bitlinear_fwd(const float* X, int64_t M, int64_t K, const uint32_t* codes,
                            const float* alpha, int alpha_raw, const float* bias, int64_t N,
                            float* Y, void* stream);

/*
 * The same forward as a VALU sign-accumulate (north_star's first inner-product option: every
 * x * q with q in {-1, 0, +1} an exact signed add on packed fp32 FMA, one k-ordered chain
 * per output) -- the A/B partner of ob_bitlinear_fwd's bf16x3 MFMA kernel, not used by the
 * module path. K % 4 == 0 and X 16-B aligned, else OB_ERR_SHAPE / OB_ERR_ALIGN.
 * Replaces the same call (quant.py:126).
 */
OB_API int ob_bitlinear_fwd_signacc(const float* X, int64_t M, int64_t K, const uint32_t* codes,
                                    const float* alpha, int alpha_raw, const float* bias,
                                    int64_t N, float* Y, void* stream);

/*
 * BitLinear backward, input gradient (autograd of F.linear at quant.py:126):
 *   dX[M][K] = a * (dY[M][N] . Q)       using codes_t (layout above)
 */
OB_API int ob_bitlinear_bwd_dx(const float* dY, int64_t M, int64_t N, const uint32_t* codes_t,
                               const float* alpha, int alpha_raw, int64_t K, float* dX,
                               void* stream);

/*
 * BitLinear backward, weight / scale / bias gradients (F.linear autograd at
 * quant.py:126 fused with _QuantizeSTE.backward, quant.py:72-92):
 *   G        = dY^T . X                       ([N][K], summed over all M rows)
 *   dW       = G * 1[|W/a| <= 1]
 *   dalpha[0]= sum(G * term(W/a)) (* sign(alpha) when alpha_raw = 1)
 *   db[n]    = sum_m dY[m][n]                 (db may be NULL)
 * Deterministic (fixed-order split-M reduction); ws must hold
 * ob_bitlinear_bwd_dw_workspace(M, N, K) bytes.
 */
OB_API size_t ob_bitlinear_bwd_dw_workspace(int64_t M, int64_t N, int64_t K);
OB_API int ob_bitlinear_bwd_dw(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                               const float* W, const float* alpha, int alpha_raw, int bits,
                               float* dW, float* dalpha, float* db, void* ws, size_t ws_bytes,
                               void* stream);

/*
 * Graph-mode variants: the bitwidth is read on device from *bits_dev (int32, 1 or 2) when
 * the kernel runs, so one captured HIP graph serves the stochastic-precision pass whose
 * per-block bitwidths change every step (reference train.py:102-103, conformer.py:265-269).
 * Same semantics as ob_quant_pack / ob_bitlinear_bwd_dw otherwise.
 */
OB_API int ob_quant_pack_dyn(const float* W, const float* alpha, int alpha_raw,
                             const int32_t* bits_dev, int64_t N, int64_t K, uint32_t* codes,
                             uint32_t* codes_t, void* stream);
OB_API int ob_bitlinear_bwd_dw_dyn(const float* dY, const float* X, int64_t M, int64_t N,
                                   int64_t K, const float* W, const float* alpha, int alpha_raw,
                                   const int32_t* bits_dev, float* dW, float* dalpha, float* db,
                                   void* ws, size_t ws_bytes, void* stream);

/*
 * Conv-module depthwise Conv1d (reference conformer.py:147
 * nn.Conv1d(C, C, KT, padding=KT//2, groups=C), applied at conformer.py:157).
 * x, y: [B][C][T]; w: [C][KT] (the Conv1d weight [C,1,KT]); bias [C] or NULL; KT odd, <= 64.
 *   y[b,c,t] = bias[c] + sum_j w[c,j] * x[b,c,t+j-KT/2]   (zero padding)
 * Backward: dx (may be NULL), dw [C][KT], db [C] (may be NULL); deterministic.
 */
OB_API int ob_dwconv1d_fwd(const float* x, const float* w, const float* bias, int64_t B,
                           int64_t C, int64_t T, int64_t KT, float* y, void* stream);
OB_API size_t ob_dwconv1d_bwd_workspace(int64_t B, int64_t C, int64_t KT);
OB_API int ob_dwconv1d_bwd(const float* x, const float* dy, const float* w, int64_t B, int64_t C,
                           int64_t T, int64_t KT, float* dx, float* dw, float* db, void* ws,
                           size_t ws_bytes, void* stream);

/*
 * CTC loss (reference losses.py:41-47: nn.CTCLoss(blank, zero_infinity=True), 'mean'),
 * with the lengths read on device so a training step can be captured in a HIP graph.
 * log_probs [B][T][V] (log_softmax output), targets [B][S] int64 padded, lengths int64 [B].
 * fwd writes loss[0] and fills ws (alpha, per-sample nll); bwd needs the same ws and writes
 * grad [B][T][V] with torch's CTC gradient formula, scaled by grad_out[0] (NULL -> 1).
 */
OB_API size_t ob_ctc_loss_workspace(int64_t B, int64_t T, int64_t S);
OB_API int ob_ctc_loss_fwd(const float* log_probs, const int64_t* targets,
                           const int64_t* input_lengths, const int64_t* target_lengths, int64_t B,
                           int64_t T, int64_t V, int64_t S, int blank, float* loss, void* ws,
                           size_t ws_bytes, void* stream);
OB_API int ob_ctc_loss_bwd(const float* log_probs, const int64_t* targets,
                           const int64_t* input_lengths, const int64_t* target_lengths, int64_t B,
                           int64_t T, int64_t V, int64_t S, int blank, const float* grad_out,
                           float* grad, void* ws, size_t ws_bytes, void* stream);
/* The same over G groups of B/G consecutive utterances in ONE launch (the three stacked
 * passes of a training step, each the reference's own ctc_loss_from_logits call,
 * losses.py:41-47): loss[g] is group g's 'mean' loss, grad_out[g] its incoming gradient. */
OB_API int ob_ctc_loss_fwd_groups(const float* log_probs, const int64_t* targets,
                                  const int64_t* input_lengths, const int64_t* target_lengths,
                                  int64_t G, int64_t B, int64_t T, int64_t V, int64_t S,
                                  int blank, float* loss, void* ws, size_t ws_bytes,
                                  void* stream);
OB_API int ob_ctc_loss_bwd_groups(const float* log_probs, const int64_t* targets,
                                  const int64_t* input_lengths, const int64_t* target_lengths,
                                  int64_t G, int64_t B, int64_t T, int64_t V, int64_t S,
                                  int blank, const float* grad_out, float* grad, void* ws,
                                  size_t ws_bytes, void* stream);
/* The same grouped CTC loss taken straight from the CTC head's logits [B][T][V]
 * (losses.py:41-47 is log_softmax then the CTC): the log-probabilities are read only at
 * blank and the utterance's labels, and the backward returns d loss / d logits
 * (= scale * (softmax - occupancy), torch's log-prob gradient composed with the log_softmax
 * backward up to its rounding-level sum term), so no [B*T][V] log_softmax or log-prob
 * gradient tensor exists. ws: ob_ctc_logits_workspace(B, T, S) bytes, kept from fwd to bwd.
 * logits / grad 16-byte aligned when V % 4 == 0. */
OB_API size_t ob_ctc_logits_workspace(int64_t B, int64_t T, int64_t S);
OB_API int ob_ctc_loss_logits_fwd_groups(const float* logits, const int64_t* targets,
                                         const int64_t* input_lengths,
                                         const int64_t* target_lengths, int64_t G, int64_t B,
                                         int64_t T, int64_t V, int64_t S, int blank, float* loss,
                                         void* ws, size_t ws_bytes, void* stream);
OB_API int ob_ctc_loss_logits_bwd_groups(const float* logits, const int64_t* targets,
                                         const int64_t* input_lengths,
                                         const int64_t* target_lengths, int64_t G, int64_t B,
                                         int64_t T, int64_t V, int64_t S, int blank,
                                         const float* grad_out, float* grad, void* ws,
                                         size_t ws_bytes, void* stream);

/* Decoder losses of the stacked step (replaces the torch expression of
 * onebit_asr/losses.py:22-35 att_ce_loss with label smoothing and :50-59 kl_logits, as
 * train.py:82-111 calls them per pass). logits [P][BU][V] fp32 (pass-major, P <= 64, pass 0 =
 * the teacher, detached for the KL); tgt_out [BU] int64 (tgt_out != pad_id marks the CE
 * positions); tgt_pad [BU] uint8 (1 = padded decoder input, dropped from the KL).
 * fwd: l_att[P] = mean_q(per-position smoothed CE) * msum / max(msum, 1) (the reference's
 * scalar-mean quirk) and l_kl[P-1] = sum_{q kept} KL(softmax(teacher_q) || softmax(x_pq)) /
 * max(kept, 1). bwd: grad [P][BU][V] from g_att[P], g_kl[P-1] (the teacher rows get only
 * their CE gradient). 0 < label_smoothing < 1; V % 4 == 0, V <= 8192; logits / grad 16-byte
 * aligned. ws: ob_att_kl_workspace(P, BU) bytes, kept from fwd to bwd. */
OB_API size_t ob_att_kl_workspace(int64_t P, int64_t BU);
OB_API int ob_att_kl_loss_fwd(const float* logits, const int64_t* tgt_out,
                              const uint8_t* tgt_pad, int64_t P, int64_t BU, int64_t V,
                              int pad_id, float label_smoothing, float* l_att, float* l_kl,
                              void* ws, size_t ws_bytes, void* stream);
OB_API int ob_att_kl_loss_bwd(const float* logits, const int64_t* tgt_out,
                              const uint8_t* tgt_pad, int64_t P, int64_t BU, int64_t V,
                              float label_smoothing, const float* g_att, const float* g_kl,
                              float* grad, const void* ws, size_t ws_bytes, void* stream);
/* The training step's loss from its per-pass parts (train.py:95-111 with the three passes
 * stacked: teacher 2-bit, student 1-bit, SP): l_int[p] = (1 - gamma) l_att[p] + gamma l_ctc[p],
 * loss = l_int[0] + lambda1 (l_int[1] + l_int[2]) + lambda2 (l_kl[0] + l_kl[1]) -- each
 * multiply and add rounded in that order (the torch expression's sequence) -- and
 * parts[8] = (l_int[0..2], l_kl[0..1], l_ctc[0..2]). DEVICE pointers, one launch each way.
 * bwd: from g_loss [1]: d_att[3], d_ctc[3], d_kl[2] (the expression's autograd). */
OB_API int ob_loss_combine_fwd(const float* l_att, const float* l_ctc, const float* l_kl,
                               float gamma, float lambda1, float lambda2, float* loss,
                               float* parts, void* stream);
OB_API int ob_loss_combine_bwd(const float* g_loss, float gamma, float lambda1, float lambda2,
                               float* d_att, float* d_ctc, float* d_kl, void* stream);

/* ------------------------------------------------------------------------------------
 * Stacked passes. The reference's training step runs every BitLinear three times per
 * batch -- 2-bit teacher, 1-bit student and the stochastic-precision pass
 * (onebit_asr/train.py:82-105) -- each a separate QuantizedLinear.forward
 * (quant.py:120-127) whose autograd gradients torch then sums. These entries take the P
 * passes of one layer stacked along rows: X is [P][M][K] (P*M rows), pass p runs at
 * bitwidth pass_bits[p] (DEVICE int32 [P]; 1 selects the 1-bit codes, anything else the
 * 2-bit codes), so the per-step SP mask can change without re-launch decisions on the
 * host. codes2 / codes1 are the ob_quant_pack outputs of the same (W, alpha) for
 * bits 2 and 1.
 *   fwd : Y[p] = a * X[p] . Q_{bits_p}^T + bias
 *   dX  : dX[p] = a * dY[p] . Q_{bits_p}
 *   dW  : dW = 1[|W/a| <= 1] * sum_p dY[p]^T X[p]; dalpha = sum_p sum(G_p * term_{bits_p})
 *         * d|alpha|; db = sum over all P*M rows of dY -- the sum over passes the
 *         reference's autograd forms (the STE mask does not depend on the bitwidth).
 * P <= 4 for dW (ob_bitlinear_bwd_dw_passes_workspace returns 0 otherwise).
 * ------------------------------------------------------------------------------------ */
OB_API int ob_bitlinear_fwd_passes(const float* X, int64_t P, int64_t M, int64_t K,
                                   const uint32_t* codes2, const uint32_t* codes1,
                                   const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                   const float* bias, int64_t N, float* Y, void* stream);
/* G <= 3 layers of one input (the q / k / v projections of one LayerNorm output,
 * conformer.py:111-113) as ONE launch: Y[i] = ob_bitlinear_fwd_passes(X, codes2[i],
 * codes1[i], alpha[i], bias[i]) for each i (same K, N; the arrays are HOST arrays of device
 * pointers, bias[i] may be NULL). Same arithmetic as G separate calls (bit-identical). */
OB_API int ob_bitlinear_fwd_passes_group(int64_t G, const float* X, int64_t P, int64_t M,
                                         int64_t K, const uint32_t* const* codes2,
                                         const uint32_t* const* codes1, const int32_t* pass_bits,
                                         const float* const* alpha, int alpha_raw,
                                         const float* const* bias, int64_t N, float* const* Y,
                                         void* stream);
/*
 * Opt-in int8 activation mode (north_star "per-tensor absmax int8 activations"; NOT the
 * reference's arithmetic, which keeps activations fp32 at quant.py:126 -- SURVEY.md §0
 * F3). Replaces, for QuantizedLinear.act_quant == "absmax_int8", the F.linear call of
 * quant.py:126 by BitNet-b1.58 activation quantization x int8 matrix cores:
 *   g_p = max(max|X_p|, 1e-5); sx = 127/g_p; xq = clamp(rint(x*sx), -127, 127);
 *   Y = float(sum_k xq*Q) * (a * (g_p/127)) + b   (mul then add, each rounded: no fma).
 * ob_act_absmax: amax[p] = max|X_p| over the n_per_pass elements of pass p (per-block
 *   partials in ws, then a final reduce; order-independent, so deterministic). X 16-byte
 *   aligned, n_per_pass % 4 == 0; ws of ob_act_absmax_workspace(P) bytes.
 * ob_act_dequant_i8: X_deq = xq * (g_p/127) (the activations the int8 forward multiplied;
 *   dW = dY^T X_deq under the straight-through estimator).
 * ob_bitlinear_fwd_i8: P passes stacked on rows like ob_bitlinear_fwd_passes; P == 1 may
 *   pass pass_bits = NULL (then codes is used and codes1 is ignored). Needs K % 16 == 0,
 *   K <= 576 (OB_ERR_SHAPE otherwise) and X 16-byte aligned.
 */
OB_API size_t ob_act_absmax_workspace(int64_t P);
OB_API int ob_act_absmax(const float* X, int64_t P, int64_t n_per_pass, float* amax, void* ws,
                         size_t ws_bytes, void* stream);
OB_API int ob_act_dequant_i8(const float* X, int64_t P, int64_t n_per_pass, const float* amax,
                             float* X_deq, void* stream);
OB_API int ob_bitlinear_fwd_i8(const float* X, int64_t P, int64_t M, int64_t K,
                               const uint32_t* codes, const uint32_t* codes1,
                               const int32_t* pass_bits, const float* alpha, int alpha_raw,
                               const float* amax, const float* bias, int64_t N, float* Y,
                               void* stream);

/* ob_bitlinear_fwd_i8 with the inference call sites' epilogues fused (conformer.py:36-45
 * and :131-138 at dropout 0), N % 4 == 0, X / Y / R 16-byte aligned:
 *   mode 1 (swish)    Y = silu(y) and amax_out[p] = max|Y_p| (amax_out zeroed first): the
 *                     producer-side int8 scale of the next BitLinear (ff.lin2);
 *   mode 2 (residual) Y = R + rscale * (valid ? y : 0*y), row r valid iff lens == NULL or
 *                     (r % T) < lens[r / T] (padded frames zeroed, :137);
 * where y = the ob_bitlinear_fwd_i8 output. */
OB_API int ob_bitlinear_fwd_i8_epi(const float* X, int64_t P, int64_t M, int64_t K,
                                   const uint32_t* codes, const uint32_t* codes1,
                                   const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                   const float* amax, const float* bias, int64_t N, int mode,
                                   const float* R, float rscale, const int32_t* lens, int64_t T,
                                   float* amax_out, float* Y, void* stream);

/* ob_bitlinear_fwd_i8 on an int8 operand Xq [P*M][K] already quantised by its producer at
 * the scale of amax (ob_layernorm_fwd_i8, or mode 3 below): the A tiles are read as int8
 * (K bytes per row instead of 4K). N % 4 == 0; Xq / Y / R 16-byte aligned.
 *   mode 0  Y fp32 = y                              (as ob_bitlinear_fwd_i8)
 *   mode 2  Y fp32 = R + rscale * (valid ? y : 0*y)  (as ob_bitlinear_fwd_i8_epi mode 2)
 *   mode 3  Y int8 = the int8 image of silu(y) at amax_out[p] = max|silu(y)| over pass p
 *           (N % 16 == 0)
 *           (ff.lin1 -> ff.lin2, conformer.py:36-39 at dropout 0): the product is
 *           computed twice (absmax, then quantise + store), so silu(y) never reaches HBM
 *           in fp32; ff.lin2 on Y (mode 2) equals ob_bitlinear_fwd_i8_epi mode 1 -> mode 2
 *           bit for bit. */
OB_API int ob_bitlinear_fwd_i8q(const int8_t* Xq, int64_t P, int64_t M, int64_t K,
                                const uint32_t* codes, const uint32_t* codes1,
                                const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                const float* amax, const float* bias, int64_t N, int mode,
                                const float* R, float rscale, const int32_t* lens, int64_t T,
                                float* amax_out, void* Y, void* stream);

OB_API int ob_bitlinear_bwd_dx_passes(const float* dY, int64_t P, int64_t M, int64_t N,
                                      const uint32_t* codes2_t, const uint32_t* codes1_t,
                                      const int32_t* pass_bits, const float* alpha,
                                      int alpha_raw, int64_t K, float* dX, void* stream);
/* The summed input gradient of G BitLinears that read the same input (the q / k / v
 * projections of one LayerNorm output, conformer.py:111-113; autograd sums their input
 * gradients): dX = sum_g alpha_g dY_g . Q_g (autograd of quant.py:126 per layer, summed) in
 * ONE launch, each dY_g [P*M][N] against its own codes (codes2_t[g] / codes1_t[g] as
 * ob_bitlinear_bwd_dx_passes, per-pass bitwidths from pass_bits), each product formed as
 * (alpha_g dY_g) Q_g (the reference's dY (alpha Q) product rounding). Host arrays of G
 * device pointers. Taken for G = 3, N = 144, K a multiple of 144, 16-byte aligned dY / dX;
 * otherwise OB_ERR_SHAPE with nothing launched (run ob_bitlinear_bwd_dx_passes per source). */
OB_API int ob_bitlinear_bwd_dx_passes_sum(int64_t G, const float* const* dY, int64_t P,
                                          int64_t M, int64_t N, const uint32_t* const* codes2_t,
                                          const uint32_t* const* codes1_t,
                                          const int32_t* pass_bits, const float* const* alpha,
                                          int alpha_raw, int64_t K, float* dX, void* stream);
OB_API size_t ob_bitlinear_bwd_dw_passes_workspace(int64_t P, int64_t M, int64_t N, int64_t K);
OB_API int ob_bitlinear_bwd_dw_passes(const float* dY, const float* X, int64_t P, int64_t M,
                                      int64_t N, int64_t K, const float* W, const float* alpha,
                                      int alpha_raw, const int32_t* pass_bits, float* dW,
                                      float* dalpha, float* db, void* ws, size_t ws_bytes,
                                      void* stream);
/* G (<= 3) layers of the same input X and shape (the q/k/v projections of one LayerNorm
 * output, conformer.py:111-113): ob_bitlinear_bwd_dw_passes of each, their finishes (chunk
 * sum, STE mask, db, dalpha) in ONE launch. Same arithmetic per layer. Arrays of G device
 * pointers (host arrays); db[i] may be NULL. ws: ..._group_workspace(G, P, M, N, K) bytes. */
OB_API size_t ob_bitlinear_bwd_dw_passes_group_workspace(int64_t G, int64_t P, int64_t M,
                                                         int64_t N, int64_t K);
OB_API int ob_bitlinear_bwd_dw_passes_group(int64_t G, const float* const* dY, const float* X,
                                            int64_t P, int64_t M, int64_t N, int64_t K,
                                            const float* const* W, const float* const* alpha,
                                            int alpha_raw, const int32_t* pass_bits,
                                            float* const* dW, float* const* dalpha,
                                            float* const* db, void* ws, size_t ws_bytes,
                                            void* stream);

/* Deferred weight-gradient finishes (reference train.py:104-111: the parameter gradients
 * are read only by clip_grad_norm_ / AdamW after loss.backward() ends). The *_defer entries
 * launch only the split-M partial GEMM; the partial launch itself writes the layer's finish
 * descriptor (chunk sum + STE mask + db + dalpha, as ob_bitlinear_bwd_dw_passes) into slot
 * `slot` of a caller-owned device table of ob_dw_finish_entry_bytes() entries, at finish
 * block offset `start`, and returns the layer's finish block count in *n_blocks (0: the shape
 * took a path that finished immediately -- no entry written). ob_dw_finish_table then runs
 * every entry's finish in ONE launch (total_blocks = the sum of the counts, entries in slot
 * order). Until it has run, dW / dalpha / db are undefined; the workspace must stay
 * allocated. The group form writes G consecutive entries (G <= 3). */
OB_API size_t ob_dw_finish_entry_bytes(void);
OB_API int ob_bitlinear_bwd_dw_passes_defer(const float* dY, const float* X, int64_t P,
                                            int64_t M, int64_t N, int64_t K, const float* W,
                                            const float* alpha, int alpha_raw,
                                            const int32_t* pass_bits, float* dW, float* dalpha,
                                            float* db, void* ws, size_t ws_bytes, void* table,
                                            int64_t slot, int64_t start, int64_t* n_blocks,
                                            void* stream);
OB_API int ob_bitlinear_bwd_dw_passes_group_defer(
    int64_t G, const float* const* dY, const float* X, int64_t P, int64_t M, int64_t N,
    int64_t K, const float* const* W, const float* const* alpha, int alpha_raw,
    const int32_t* pass_bits, float* const* dW, float* const* dalpha, float* const* db,
    void* ws, size_t ws_bytes, void* table, int64_t slot, int64_t start, int64_t* n_blocks,
    void* stream);
OB_API int ob_dw_finish_table(const void* table, int64_t n, int64_t total_blocks, void* stream);

/* Grouped deferred weight gradients. Every weight gradient of a backward whose N and K are
 * multiples of 144 -- a BitLinear's (autograd of quant.py:126 through quant.py:72-92: dW with
 * the STE mask, dalpha at each stacked pass's bitwidth, db) or a dense linear's (W == NULL:
 * dW = dY^T X, db) -- computed in ONE persistent launch after the backward (the reference reads
 * parameter gradients only after loss.backward(), train.py:104-111), instead of one split-M
 * launch per layer plus the finish table. Rows of pass p are rows p*M .. p*M+M-1 of dY and X.
 * `gemms` is a HOST array of G descriptors (device pointers inside). `tickets`: a caller-owned
 * device buffer of ob_dw_grouped_tickets(...) uint32 words, all zero before the first call;
 * every call leaves it zero. Deterministic: fixed partition of the rows, fixed summation order.
 * dY / X / W / alpha / pass_bits must stay valid until the launch has run. */
typedef struct ob_dwg_gemm {
  const float* dY;          /* [P*M][N] */
  const float* X;           /* [P*M][K] */
  const float* W;           /* [N][K] BitLinear weight; NULL = dense (no STE mask, no dalpha) */
  const float* alpha;       /* BitLinear: 0-dim alpha (alpha_raw as ob_bitlinear_bwd_dw) */
  const int32_t* pass_bits; /* DEVICE [P] bitwidths (1 or 2); NULL: `bits` for every pass */
  float* dW;                /* [N][K] */
  float* db;                /* [N] or NULL */
  float* dalpha;            /* 0-dim (BitLinear; unused when W == NULL) */
  int64_t N, K, M, P;       /* M = rows of one pass (>= 1), 1 <= P <= 4 */
  int32_t alpha_raw, bits;
} ob_dwg_gemm;
OB_API int ob_dw_grouped_supported(int64_t N, int64_t K);
OB_API size_t ob_dw_grouped_workspace(const ob_dwg_gemm* gemms, int64_t G);
OB_API size_t ob_dw_grouped_tickets(const ob_dwg_gemm* gemms, int64_t G);
OB_API int ob_dw_grouped(const ob_dwg_gemm* gemms, int64_t G, void* ws, size_t ws_bytes,
                         void* tickets, size_t ticket_words, void* stream);

/* ------------------------------------------------------------------------------------
 * The decoder's attention core (onebit_asr/conformer.py:275-299: the stock
 * nn.TransformerDecoderLayer self- and cross-attention, torch's
 * multi_head_attention_forward between the in- and out-projections):
 *   ctx = dropout(softmax((q k^T) * (1/sqrt(dh)) + mask)) v    per head
 * q [B][Lq][*] with row stride sq floats (head h = columns h*dh .. h*dh+dh-1), k / v
 * [B][Lk][*] (strides sk / sv): the packed projection outputs are read in place. mask: key j
 * of batch row b is -inf when kmask[b*Lk + j] != 0 (kmask may be NULL) and, causal != 0,
 * when j > i. ctx [B][Lq][H*dh]; probs [B][H][Lq][Lk] (the softmax output, a dropped
 * element stored negated) is kept for the backward. Dropout p_drop: the library's counter
 * hash on (rng, rng_offset), like every fused dropout. Supported: dh in {16, 32, 36, 64},
 * Lk <= 256 and the per-(b, h) working set within LDS (ob_decattn_supported).
 * ctx must be 16-byte aligned. bwd (ctx = the forward's output): dq [B][Lq][*] (row stride
 * gq), dk / dv [B][Lk][*] (gk / gv), every element of the heads' columns written -- e.g.
 * straight into the packed projection's gradient. The backward CONSUMES probs: it holds the
 * score gradients dS' afterwards (two launches: dk / dv, then dq from dS'); ABI 4. */
OB_API int ob_decattn_supported(int64_t Lq, int64_t Lk, int64_t dh);
OB_API int ob_decattn_fwd(const float* q, int64_t sq, const float* k, int64_t sk, const float* v,
                          int64_t sv, const uint8_t* kmask, int64_t causal, int64_t B, int64_t H,
                          int64_t Lq, int64_t Lk, int64_t dh, float p_drop, const int64_t* rng,
                          int64_t rng_offset, float* probs, float* ctx, void* stream);
OB_API int ob_decattn_bwd(const float* dctx, const float* ctx, const float* q, int64_t sq,
                          const float* k, int64_t sk, const float* v, int64_t sv, int64_t B, int64_t H, int64_t Lq,
                          int64_t Lk, int64_t dh, float p_drop, float* probs, float* dq,
                          int64_t gq, float* dk, int64_t gk, float* dv, int64_t gv, void* stream);
/* Inference forward with shared keys / values (the n-best hypotheses of one utterance against
 * its encoder memory): q and ctx have B * kv_group batch rows, k / v / kmask have B, and q
 * batch row b reads row b / kv_group. No dropout, no probs output. The same arithmetic in the
 * same order as ob_decattn_fwd at p_drop = 0: bitwise equal to it on explicitly repeated
 * k / v / kmask. Same support limits (ob_decattn_supported); kv_group >= 1. */
OB_API int ob_decattn_fwd_grouped(const float* q, int64_t sq, const float* k, int64_t sk,
                                  const float* v, int64_t sv, const uint8_t* kmask,
                                  int64_t causal, int64_t B, int64_t kv_group, int64_t H,
                                  int64_t Lq, int64_t Lk, int64_t dh, float* ctx, void* stream);

/* ------------------------------------------------------------------------------------
 * Relative-position attention core of MHSA.forward (onebit_asr/conformer.py:115-127),
 * fused: ac = (q+u) k^T, bd = rel_shift((q+v) pos^T) (:97-103), S = (ac + bd) / sqrt(d),
 * frames i or j >= lens[b] masked to -inf (:121-122), A = nan_to_num(softmax(S))
 * (:123-125), A = dropout(A) (:126), ctx = A v (:127).
 *   q, k, v, ctx, dq, dk, dv : [Bt][T][H*d]   (heads side by side, as the projections
 *                              produce them and out_proj consumes them)
 *   pos, dpos : [P][T][H*d]    (pass p = b / (Bt/P) for stacked passes; P = 1 otherwise)
 *   u, vb, du, dvb : [H][d]    (pos_bias_u / pos_bias_v)
 *   lens : DEVICE int32 [Bt]   (valid frames; the encoder's prefix masks)
 *   saved : the forward's state for the backward (ob_relattn_saved_elems fp32 elements,
 *           16-B aligned; NULL when no backward follows): row statistics [Bt*H][Tp][2]
 *           (max of the scaled masked scores, 1/sum; Tp = 16*ceil(T/16)), the dropout keep
 *           bits [Bt*H][Tp][W] (uint32, W = ceil(Tp/32), key j of row i = bit j%32 of word
 *           j/32), then (default backward mode) the probability tiles below -- the
 *           statistics region is reserved but not written -- or, in the flash backward mode
 *           (ob_relattn_set_bwd_mode(1) or OB_ATTN_BWD=flash; only T <= 256 and d <= 36, other
 *           shapes always take the probability tiles), the statistics, the keep bits and the
 *           X rows below each 32-query chunk: that backward recomputes the probabilities of
 *           32-query chunks (bitwise the forward's) and keeps every [T][T] quantity on chip.
 *           It is slower at Conformer-S, hence opt-in.
 *   probs : optional (NULL: not written) MFMA-fragment tiles [Bt*H][nt][nt][64][4],
 *           nt = ceil(T/16), of the softmax before dropout (ob_relattn_probs_elems floats):
 *           tile (a, t), lane r + 16g, element e holds P[16a + r][16t + 4g + e] (rows / keys
 *           >= T: 0); with p_drop > 0 a dropped element is stored as -P.
 *   ctx (bwd) : the forward's output (the softmax backward's row term is dO . ctx)
 *   rng : DEVICE int64 [2] (seed, counter), rng_offset a host offset added to the counter
 *         (the fused BitLinear entries' convention: one device state, a distinct offset per
 *         call site, the counter advanced once per step); dropout keeps element (i, j) of
 *         row bh when the 16-bit field (j & 1) of hash(seed, counter + rng_offset,
 *         ((bh*T + i)*Te + j) / 2) >= p_drop * 2^16, Te = T rounded up to even (the bwd
 *         reads the forward's decisions from the saved keep bits; ob_relattn_dropout_mask
 *         writes the mask out). Unused when p_drop == 0.
 * Supported: 1 <= T <= 512, d in {16, 32, 36, 64} (longer T, forward only: ob_relattn_infer).
 * ------------------------------------------------------------------------------------ */
OB_API int ob_relattn_fwd(const float* q, const float* k, const float* v, const float* pos,
                          const float* u, const float* vb, const int32_t* lens, int64_t Bt,
                          int64_t P, int64_t T, int64_t H, int64_t d, float p_drop,
                          const int64_t* rng, int64_t rng_offset, float* saved, float* probs,
                          float* ctx, void* stream);
OB_API int64_t ob_relattn_saved_elems(int64_t Bt, int64_t T, int64_t H, int64_t d);
OB_API int64_t ob_relattn_probs_elems(int64_t Bt, int64_t T, int64_t H);
OB_API size_t ob_relattn_bwd_workspace(int64_t Bt, int64_t T, int64_t H, int64_t d);
OB_API int ob_relattn_bwd(const float* dctx, const float* ctx, const float* q, const float* k,
                          const float* v, const float* pos, const float* u, const float* vb,
                          const int32_t* lens, int64_t Bt, int64_t P, int64_t T, int64_t H,
                          int64_t d, float p_drop, const int64_t* rng, int64_t rng_offset,
                          const float* saved, int64_t saved_elems,
                          float* dq, float* dk, float* dv, float* dpos, float* du, float* dvb,
                          void* ws, size_t ws_bytes, void* stream);
/* The same attention core for long utterances, forward only (inference): no dropout, nothing
 * saved, ctx the only output. Same layouts as ob_relattn_fwd (q, k, v, ctx [Bt][T][H*d]; pos
 * [P][T][H*d], batch row b uses pass b / (Bt/P); u, vb [H][d]; lens DEVICE int32 [Bt]); T is the
 * padded length of the tensors (rel_shift depends on it), never lens[b]. Keys >= lens[b] are
 * masked and every query row >= lens[b] comes out exactly 0 (a length-0 row is all zeros). The
 * keys are walked in chunks of ob_relattn_infer_key_chunk() with an online softmax in fp32, every
 * product an exact fp32 fma chain; no [T][T] quantity exists anywhere, and two calls on the same
 * inputs give the same bits (not necessarily ob_relattn_fwd's: the sums are ordered differently).
 * Supported: 1 <= T <= ob_relattn_infer_max_t() (4096), d in {16, 32, 36, 64}, T*H*d <= 2^29.
 * OB_ERR_SHAPE for T, d outside that, Bt < 1, P < 1, Bt % P != 0, H < 1, Bt or H > 65535;
 * OB_ERR_NULL for a null tensor pointer; both before any device call. */
OB_API int ob_relattn_infer(const float* q, const float* k, const float* v, const float* pos,
                            const float* u, const float* vb, const int32_t* lens, int64_t Bt,
                            int64_t P, int64_t T, int64_t H, int64_t d, float* ctx, void* stream);
OB_API int64_t ob_relattn_infer_key_chunk(void);
OB_API int64_t ob_relattn_infer_max_t(void);
/* The attention backward mode, process-wide: 0 = probability tiles (default), 1 = flash style
 * (T <= 256, d <= 36); any other value only queries. Returns the previous mode. The initial
 * mode is OB_ATTN_BWD (read once). ob_relattn_saved_elems / ob_relattn_bwd_workspace follow the
 * current mode; ob_relattn_bwd returns OB_ERR_SHAPE when `saved_elems` (the size the forward's
 * buffer was allocated with) is not the current mode's -- the mode changed in between. */
OB_API int ob_relattn_set_bwd_mode(int mode);
/* The K = 144 swish-epilogue ternary GEMMs (ob_bitlinear_fwd_swish_drop with K in 129..160,
 * ob_bitlinear_bwd_dx_swish_drop with N in 129..160; output width a multiple of 64), process-
 * wide: 1 (default) = the column-looped kernel (one block holds all output columns, each
 * activation row is split once), 0 = the 64-column kernel every other shape runs; any other
 * value only queries. Returns the previous setting. Both give the same bits. */
OB_API int ob_tgemm_set_colloop(int on);
/* The key-side kernel of the probability-tile attention backward (ob_relattn_bwd in mode 0),
 * process-wide: 1 (default) = the two-stage LDS ring (one block barrier per 16 queries, the next
 * stage written under the current one's MFMAs), 0 = the kernel that stages 32 queries between
 * two barriers; any other value only queries. Returns the previous setting. Both give the same
 * bits. */
OB_API int ob_relattn_set_kv_ring(int on);
/* The prefetch-window specialisations of the probability-tile attention kernels (ob_relattn_fwd /
 * ob_relattn_bwd in mode 0), process-wide, read at launch: bit 0 = the query-side backward,
 * bit 1 = the forward; default 3. They run where every 16-key tile of the kernel's tile count is
 * live (ceil(T / 16) = 16 for T <= 256, 32 above: the training step's T = 249 is one); every other
 * T, and mask 0, runs the general kernels. A value outside 0 .. 3 only queries. Returns the
 * previous mask. All give the same bits. */
OB_API int ob_relattn_set_windows(int mask);
/* The dropout keep-mask (1 = kept) of n elements laid out in rows of row_len: the attention
 * kernels' mask of [rows][T] probabilities with row_len = T, the BitLinear / LayerNorm /
 * residual-dropout kernels' mask of a flat tensor with row_len = n. */
OB_API int ob_relattn_dropout_mask(int64_t n, int64_t row_len, float p_drop, const int64_t* rng,
                                   int64_t rng_offset, uint8_t* out, void* stream);

/* Token-embedding backward of the decoder (conformer.py:279-299, nn.Embedding with
 * padding_idx): grad_weight[v] = sum over n ascending with indices[n] == v of grad[n]
 * (deterministic, graph-safe); grad_weight[padding_idx] = 0 (padding_idx < 0: none).
 * indices int64 [N] in [0, V); grad [N][C]; grad_weight [V][C]; C <= 1024. */
OB_API int ob_embedding_bwd(const int64_t* indices, int64_t N, const float* grad, int64_t C,
                            int64_t V, int64_t padding_idx, float* grad_weight, void* stream);

/* ------------------------------------------------------------------------------------
 * Optimizer tail of the training step: clip_grad_norm_(params, max_norm) followed by
 * AdamW.step() (reference onebit_asr/train.py:116-118 with the optimizer of train.py:259:
 * betas (0.9, 0.98), eps 1e-8, weight_decay 1e-2). torch issues per-tensor launches for
 * the ~800 parameter tensors; this is three launches over a table of tensors.
 *
 * table     : DEVICE array of n_tensors descriptors (param, grad, exp_avg, exp_avg_sq are
 *             device fp32 buffers of numel elements; exp_avg / exp_avg_sq start at 0)
 * chunk_map : DEVICE int64 [2 * n_blocks] from ob_adamw_plan (host) for the same numels
 * lr        : DEVICE fp32 learning rate (the warmup-cosine schedule writes it)
 * step      : DEVICE fp32 step counter shared by all tensors; incremented by the call
 * grad_scale: every gradient is multiplied by it first (1/world after a SUM all-reduce)
 * max_norm  : <= 0 disables clipping. total_norm (optional DEVICE fp32) receives the
 *             pre-clip global L2 norm, as clip_grad_norm_ returns it.
 * Gradients are clipped in registers (the grad buffers are not modified).
 * ------------------------------------------------------------------------------------ */
typedef struct ob_adamw_tensor {
  float* param;
  const float* grad;
  float* exp_avg;
  float* exp_avg_sq;
  int64_t numel;
} ob_adamw_tensor;

/* Host-only. Number of blocks for these tensor sizes; fills chunk_map (HOST int64
 * [2 * n_blocks]) when non-NULL. Negative status for an empty table or numel < 1. */
OB_API int64_t ob_adamw_plan(const int64_t* numels, int64_t n_tensors, int64_t* chunk_map);
OB_API size_t ob_adamw_workspace(int64_t n_blocks);
OB_API int ob_adamw_clip_step(const ob_adamw_tensor* table, int64_t n_tensors,
                              const int64_t* chunk_map, int64_t n_blocks, const float* lr,
                              float* step, float grad_scale, double beta1, double beta2,
                              double eps, double weight_decay, double max_norm,
                              float* total_norm, void* ws,
                              size_t ws_bytes, void* stream);

/*
 * LayerNorm over the last dim (the Conformer's LayerNorm wrappers, conformer.py:19-24:
 * nn.LayerNorm(d) before every BitLinear call site). x, y [rows][d], d <= 512;
 * gamma/beta [d] or NULL (1 / 0); mean, rstd [rows] (either may be NULL when no backward
 * follows). var is biased (torch), rstd = 1/sqrt(var + eps).
 * Backward: dx [rows][d]; dgamma/dbeta [d] (NULL to skip) summed over rows in a fixed
 * order (deterministic) through the workspace.
 */
OB_API int ob_layernorm_fwd(const float* x, const float* gamma, const float* beta, int64_t rows,
                            int64_t d, float eps, float* y, float* mean, float* rstd,
                            void* stream);
/* Two LayerNorms back to back (a Conformer block's final LN, conformer.py:228, and the next
 * module's input LN, :28 / the encoder's output LN): y1 = LN1(x) (gamma g1, beta b1), y2 =
 * LN2(y1), with both rows' mean / rstd (each may be NULL), in one pass over x -- bit-identical
 * to two ob_layernorm_fwd calls. */
OB_API int ob_layernorm_fwd_pair(const float* x, const float* g1, const float* b1,
                                 const float* g2, const float* b2, int64_t rows, int64_t d,
                                 float eps1, float eps2, float* y1, float* mean1, float* rstd1,
                                 float* y2, float* mean2, float* rstd2, void* stream);
/* ob_layernorm_fwd plus amax[p] = max|y| over pass p (rows split into P equal passes,
 * P <= 8): the producer-side per-tensor scale of the int8 BitLinear that consumes y.
 * ws: ob_layernorm_fwd_amax_workspace(P) bytes (per-block partial maxima). */
OB_API size_t ob_layernorm_fwd_amax_workspace(int64_t P);
OB_API int ob_layernorm_fwd_amax(const float* x, const float* gamma, const float* beta,
                                 int64_t rows, int64_t d, float eps, float* y, float* mean,
                                 float* rstd, int64_t P, float* amax, void* ws,
                                 size_t ws_bytes, void* stream);
/* The int8 image of LN(x) for an int8 BitLinear consumer (north_star "int8 activation tiles"
 * in HBM): amax[p] = max|LN(x)| over pass p, then yq = clamp(rint(LN(x) * 127 /
 * max(amax[p], 1e-5)), -127, 127) int8 [rows][d] -- the quantisation ob_bitlinear_fwd_i8
 * applies in registers to an fp32 operand, so ob_bitlinear_fwd_i8q on yq is bit-identical to
 * ob_bitlinear_fwd_i8 on LN(x). Two row passes (LN is recomputed; no fp32 y in HBM);
 * ws: ob_layernorm_fwd_amax_workspace(P) bytes; yq 4-byte aligned. Replaces the pair
 * LayerNorm (conformer.py:19-24) -> activation quantisation of the consumer. */
OB_API int ob_layernorm_fwd_i8(const float* x, const float* gamma, const float* beta,
                               int64_t rows, int64_t d, float eps, int64_t P, float* amax,
                               int8_t* yq, void* ws, size_t ws_bytes, void* stream);
OB_API size_t ob_layernorm_bwd_workspace(int64_t rows, int64_t d);
OB_API int ob_layernorm_bwd(const float* dy, const float* x, const float* gamma,
                            const float* mean, const float* rstd, int64_t rows, int64_t d,
                            float* dx, float* dgamma, float* dbeta, void* ws, size_t ws_bytes,
                            void* stream);
/* ob_layernorm_bwd plus an additive gradient: dx = LN_backward(dy) + dres. At a residual
 * junction x -> (LN -> module) + x (conformer.py:34-45, :105-138, :149-167) this is the
 * sum autograd would form with a separate add kernel. */
OB_API int ob_layernorm_bwd_res(const float* dy, const float* x, const float* gamma,
                                const float* mean, const float* rstd, int64_t rows, int64_t d,
                                const float* dres, float* dx, float* dgamma, float* dbeta,
                                void* ws, size_t ws_bytes, void* stream);
/* ob_layernorm_bwd / _res (dres may be NULL) with an optional second output for the module
 * whose output this LN normalises: dy2 = rscale * rowvalid * drop(dx), element for element
 * ob_drop_scale_bwd(dx, rows, d, rscale, p_drop, rng, rng_offset, lens, T) -- the backward
 * of that module's residual tail "R + rscale * rowvalid * dropout(y)" (conformer.py:39-45,
 * :131-138, :160-167), formed while dx is in registers instead of in a pass of its own.
 * dy2 == NULL: plain ob_layernorm_bwd_res. */
OB_API int ob_layernorm_bwd_ex(const float* dy, const float* x, const float* gamma,
                               const float* mean, const float* rstd, int64_t rows, int64_t d,
                               const float* dres, float* dx, float* dgamma, float* dbeta,
                               void* ws, size_t ws_bytes, float* dy2, float rscale,
                               float p_drop, const uint64_t* rng, int64_t rng_offset,
                               const int32_t* lens, int64_t T, void* stream);
/* ob_layernorm_bwd_ex with the dgamma / dbeta reduction deferred (table != NULL): the
 * backward launch writes its partials' descriptor into slot `slot` of a caller-owned device
 * table of ob_ln_param_entry_bytes() entries; ob_ln_param_table reduces entries 0 .. n-1 in
 * one launch (dmax = the largest d) with the same fixed-order arithmetic. ws stays allocated
 * until then. dres / dy2 may be NULL. */
OB_API int ob_layernorm_bwd_defer(const float* dy, const float* x, const float* gamma,
                                  const float* mean, const float* rstd, int64_t rows, int64_t d,
                                  const float* dres, float* dx, float* dgamma, float* dbeta,
                                  void* ws, size_t ws_bytes, float* dy2, float rscale,
                                  float p_drop, const uint64_t* rng, int64_t rng_offset,
                                  const int32_t* lens, int64_t T, void* table, int64_t slot,
                                  void* stream);
/* The backward of two LayerNorms back to back (ob_layernorm_fwd_pair: y1 = LN1(x), y2 =
 * LN2(y1); gres = the gradient of y1's other (residual) use, may be NULL): dx =
 * LN1_backward(LN2_backward(dy) + gres), the sum never written to memory; dy2 (may be NULL):
 * the residual-tail gradient of ob_layernorm_bwd_ex for x; dgamma / dbeta of both layers,
 * deferred into `table` at slot2 / slot1 (>= 0) or reduced now (table NULL or slot < 0).
 * ws: ob_layernorm_bwd_pair_workspace(rows, d) bytes, 16-byte aligned. With dy2 and lens
 * ([rows / T], 4-byte aligned), T < 1 or rows % T != 0 is OB_ERR_SHAPE, as in _bwd_defer. */
OB_API size_t ob_layernorm_bwd_pair_workspace(int64_t rows, int64_t d);
OB_API int ob_layernorm_bwd_pair(const float* dy, const float* y1, const float* g2,
                                 const float* mean2, const float* rstd2, const float* gres,
                                 const float* x, const float* g1, const float* mean1,
                                 const float* rstd1, int64_t rows, int64_t d, float* dx,
                                 float* dg2, float* db2, float* dg1, float* db1, void* ws,
                                 size_t ws_bytes, float* dy2, float rscale, float p_drop,
                                 const uint64_t* rng, int64_t rng_offset, const int32_t* lens,
                                 int64_t T, void* table, int64_t slot2, int64_t slot1,
                                 void* stream);
OB_API size_t ob_ln_param_entry_bytes(void);
OB_API int ob_ln_param_table(const void* table, int64_t n, int64_t dmax, void* stream);

/*
 * Batched greedy CTC decode (inference path). Replaces onebit_asr/metrics.py:51-60
 * ctc_greedy_decode(logits[T, V], blank_id) called per utterance: for utterance b over its
 * first lens[b] frames, pred = argmax_v logits[b][t][v] (lowest index on ties, as
 * torch.argmax), emit pred[t] when pred[t] != blank and pred[t] != pred[t-1].
 *   logits [B][T][V] fp32; lens int64 [B] (device); ids int32 [B][T] workspace (the
 *   per-frame argmax, left for the caller); out int32 [B][T] (tokens first, -1 after);
 *   out_len int32 [B].
 */
OB_API int ob_ctc_greedy_decode(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                                int64_t V, int blank, int32_t* ids, int32_t* out,
                                int32_t* out_len, void* stream);

/*
 * Batched CTC prefix beam search without a language model (eval path). Replaces
 * onebit_asr/metrics.py:74-145 ctc_beam_search(logits[T, V], beam_size, blank_id, top_k_per_t)
 * called per utterance by ctc_beam_search_batch (eval.py:118-128: beam_size 10, blank 3, the
 * 20 best tokens per frame). For utterance b over its first clamp(lens[b], 0, T) frames, with
 * lp = log_softmax(logits[b][t]) and a state (p_b, p_nb) per prefix, starting at {(): (0, -inf)}:
 *   blank                new[prefix].p_b      (+)= lse(p_b, p_nb) + lp[blank]
 *   c == last(prefix)    new[prefix].p_nb     (+)= p_b + lp[c]    (the reference's repeat rule:
 *                        p_b only, and the prefix is never extended by its own last token, so
 *                        the frames "a _ a" decode to [a] where greedy gives [a, a])
 *   any other c          new[prefix + c].p_nb (+)= lse(p_b, p_nb) + lp[c]
 * for the K = min(top_k, V) largest logits of the frame (ties to the lowest token index; all V
 * tokens in index order when V <= top_k); blank is skipped as a candidate but keeps its place
 * among the K. (+) is log-sum-exp accumulation per prefix tuple; after each frame the beam
 * prefixes with the largest lse(p_b, p_nb) stay (exact ties: the one the reference's dict holds
 * first). The result is the best prefix after the last frame. The log-softmax denominator and
 * every score are fp64 computed from the fp32 logits (the reference: fp32 log_softmax, then
 * Python doubles). Non-finite logits are outside the contract (the call still terminates and
 * is deterministic).
 *   logits [B][T][V] fp32; lens int64 [B] (device); 1 <= beam <= 32; 1 <= top_k <= 64;
 *   T < 2^24 and B * T < 2^31; ws: ob_ctc_beam_search_workspace(B, T, V, beam, top_k) bytes
 *   (0 for invalid arguments), 8-byte aligned, contents need not be kept between calls;
 *   out int32 [B][T] (tokens first, -1 after); out_len int32 [B]; score fp64 [B], 8-byte
 *   aligned, may be NULL: log-probability of the returned prefix (0 for an empty utterance).
 * B == 0 is OB_OK with no launch.
 */
OB_API size_t ob_ctc_beam_search_workspace(int64_t B, int64_t T, int64_t V, int beam, int top_k);
OB_API int ob_ctc_beam_search(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                              int64_t V, int blank, int beam, int top_k, void* ws,
                              size_t ws_bytes, int32_t* out, int32_t* out_len, double* score,
                              void* stream);
/* DIAGNOSTIC entry (timing each launch, tools/decode_bench.py): not for product code, which
 * calls ob_ctc_beam_search. What a stage 1 call leaves in ws is private to the library: its
 * layout may change with any build, so it is only good for a stage 2 call of the same library.
 * The two launches of ob_ctc_beam_search on their own (stage 0: both, the call above):
 * stage 1 runs the per-frame log-softmax + top-k only and leaves the candidates in ws (out,
 * out_len, score are not touched and may be NULL); stage 2 runs the search only, on the
 * candidates a stage 1 call with the same B, T, V, top_k and lens left in the same ws (logits
 * may be NULL; beam may differ when ws is large enough for it). For timing each phase and for
 * decoding the same frames at several beam sizes. */
OB_API int ob_ctc_beam_search_stage(const float* logits, const int64_t* lens, int64_t B,
                                    int64_t T, int64_t V, int blank, int beam, int top_k,
                                    int stage, void* ws, size_t ws_bytes, int32_t* out,
                                    int32_t* out_len, double* score, void* stream);

/*
 * N-best form of ob_ctc_beam_search: the same search with the same arguments and limits, plus
 * 1 <= nbest <= beam. Returns the first nbest entries of the final beam in the beam's own
 * order: total descending, exact ties in the order the reference's dict holds them. Entry 0 is
 * ob_ctc_beam_search's result bit for bit (tokens, length, score).
 *   hyp int32 [B][nbest][T] (tokens first, -1 after); hyp_len int32 [B][nbest];
 *   n_hyp int32 [B]: live entries, 1 <= n_hyp <= nbest (an utterance with lens[b] == 0 has
 *   one, the empty prefix with score 0); score fp64 [B][nbest], 8-byte aligned, required:
 *   lse(p_b, p_nb) of each entry; absent entries get -inf and hyp_len 0.
 * ws as ob_ctc_beam_search (ob_ctc_beam_search_nbest_workspace returns the same size).
 * B == 0 is OB_OK with no launch.
 */
OB_API size_t ob_ctc_beam_search_nbest_workspace(int64_t B, int64_t T, int64_t V, int beam,
                                                 int top_k);
OB_API int ob_ctc_beam_search_nbest(const float* logits, const int64_t* lens, int64_t B,
                                    int64_t T, int64_t V, int blank, int beam, int top_k,
                                    int nbest, void* ws, size_t ws_bytes, int32_t* hyp,
                                    int32_t* hyp_len, int32_t* n_hyp, double* score,
                                    void* stream);

/*
 * Attention rescoring of the CTC n-best (two-pass decoding; csrc/rescore.hip). N hypotheses
 * per utterance (1 <= N <= 32) are scored by the attention decoder under teacher forcing at a
 * static length Lc (0 <= Lc < 2^16); the best total = att + ctc_weight * ctc_score wins.
 *
 * ob_rescore_prepare: the decoder's inputs from hyp [B][N][T] / hyp_len [B][N] / n_hyp [B]
 * (the layout of ob_ctc_beam_search_nbest). For hypothesis y_1..y_n of a rescored utterance:
 *   tgt_inp int64 [B*N][Lc+1] = bos, y_1..y_n, pad...;  target int32 [B*N][Lc+1] = y_1..y_n,
 *   eos, -1...;  tgt_pad uint8 [B*N][Lc+1] = 1 after position n (position 0, bos, is never
 *   padded, so no attention row is fully masked);  ok uint8 [B] = 0 when a live hypothesis of
 *   the utterance is longer than Lc. The empty hypothesis is valid ([bos] -> [eos]). Absent
 *   entries (k >= n_hyp[b]) and every entry of an utterance with ok == 0 get the input
 *   [bos, pad...] and an all -1 target, so the scorer skips their rows.
 *
 * ob_seq_logprob: lp[r] = (h_r . W[t_r] + b[t_r]) - logsumexp_v(h_r . W[v] + b[v]) for hidden
 * [R][d] fp32, weight [V][d] fp32 (both 16-byte aligned), bias [V] (may be NULL), target int32
 * [R]; rows with target -1 are skipped and get 0 (a target >= V gets NaN). No [R][V] tensor
 * exists: ws (ob_seq_logprob_workspace(R, d, V) bytes, 8-byte aligned; 0 = unsupported) holds
 * a (max, sum of exp) pair per row and 64-column tile plus the target's logit per row.
 * Products are exact fp32 (three-plane bf16 split, six MFMAs per k-step); the tiles merge in
 * index order in fp64, without atomics: results are bitwise reproducible. d % 16 == 0,
 * 16 <= d <= 256, V >= 1, 0 <= R < 2^31 - 16; anything else is OB_ERR_SHAPE. R == 0 is OB_OK
 * with no launch.
 *
 * ob_rescore_select: lp fp32 [B*N][Lc+1] from the scorer on prepare's target. Per utterance:
 *   att[b][k]   = fp64 sum of lp over hypothesis k's len+1 rows, ascending position;
 *   total[b][k] = att + ctc_weight * ctc_score[b][k]; absent entries: att 0, total -inf;
 *   best_k[b]   = the largest total, ties to the smaller k; out int32 [B][T] (its tokens, -1
 *   after) and out_len [B];  rescored uint8 [B] = ok[b]; with ok[b] == 0 the winner is entry 0
 *   (the CTC best) and the utterance's att are 0, its total -inf.
 *   att / total / ctc_score fp64 [B][N], 8-byte aligned.
 * B == 0 is OB_OK with no launch.
 */
OB_API int ob_rescore_prepare(const int32_t* hyp, const int32_t* hyp_len, const int32_t* n_hyp,
                              int64_t B, int64_t N, int64_t T, int64_t Lc, int bos, int eos,
                              int pad, int64_t* tgt_inp, int32_t* target, uint8_t* tgt_pad,
                              uint8_t* ok, void* stream);
OB_API size_t ob_seq_logprob_workspace(int64_t R, int64_t d, int64_t V);
OB_API int ob_seq_logprob(const float* hidden, int64_t R, int64_t d, const float* weight,
                          const float* bias, int64_t V, const int32_t* target, void* ws,
                          size_t ws_bytes, float* lp, void* stream);
OB_API int ob_rescore_select(const float* lp, const int32_t* hyp, const int32_t* hyp_len,
                             const int32_t* n_hyp, const double* ctc_score, const uint8_t* ok,
                             int64_t B, int64_t N, int64_t T, int64_t Lc, double ctc_weight,
                             int32_t* out, int32_t* out_len, int32_t* best_k, double* att,
                             double* total, uint8_t* rescored, void* stream);

/*
 * Autoregressive attention-decoder beam search with a KV cache (csrc/attdec.hip): B utterances,
 * N beam slots each (R = B * N decoder rows, row b * N + k = slot k of utterance b), L static
 * steps. ob_attdec_supported(N, d, H, Lk, L): 1 <= N <= 32; d % 16 == 0, 16 <= d <= 256;
 * dh = d / H in {16, 32, 36, 64}; L >= 1 and L + 1 <= 256; Lk within ob_decattn_supported(1, Lk,
 * dh). No entry allocates, clears memory or synchronises; B == 0 / R == 0 is OB_OK with no launch.
 *
 * ob_decattn_step: the self-attention of step t (0 <= t < L) for one decoder layer. qkv [R][sq]
 * holds q | k | v of the current position (sq >= 3 * H * dh floats, sq % 4 == 0, 16-byte
 * aligned); cache [L][R][2 * H * dh] (k | v, 16-byte aligned) is this layer's; anc int32 [R][L]
 * holds, for row r and position j < t, the row whose cache entry (j, anc[r][j]) is r's ancestor
 * (entries outside 0..R-1 are clamped). The kernel stores row r's k | v at (t, r) and writes
 * ctx [R][H * dh] = softmax(q . k_j / sqrt(dh)) v over j = 0..t. Rows with skip[r] != 0 (skip may
 * be NULL) are left alone: nothing stored, ctx untouched. fp32; the order of every sum depends on
 * the positions only, so the result does not depend on which slots hold the ancestors.
 *
 * ob_seq_topk: for hidden [R][d] and the output layer weight [V][d] / bias [V] (may be NULL), per
 * row with skip[r] == 0 (skip may be NULL): lse fp64 [R] = logsumexp over all V logits, and
 * topv fp32 / topi int32 [R][K] = the K (1 <= K <= 32) largest logits and their ids among the ids
 * not in banned (a HOST array of n_banned <= 8 ids), value descending, exact ties by the smaller
 * id, padded with (-inf, -1) when fewer than K ids remain. Rows with skip[r] != 0 keep whatever
 * lse / topv / topi held. Products, limits (d, V, R) and alignment as ob_seq_logprob; no [R][V]
 * tensor exists: ws (ob_seq_topk_workspace bytes, 8-byte aligned; 0 = unsupported) holds per row
 * and 64-column tile a (max, sum of exp) pair and min(K, 64) (value, column) candidates. Fixed
 * merge order, no atomics: bitwise reproducible.
 *
 * Beam state (device): score fp64 [B][N] (sum of log-probabilities; -inf = dead slot), len int32
 * [B][N] (emitted tokens, eos counted), fin uint8 [B][N] (0 live, 1 finished, 2 dead), tok int64
 * [R] (the next step's decoder input), skip uint8 [R] (fin != 0), and two ancestry tables anc
 * int32 [R][L] used alternately. The key of a hypothesis of n emitted tokens is score / norm[n],
 * norm fp64 [L + 1] (device; the caller computes max(n, 1) ** alpha on the host).
 *   ob_attdec_init: slot 0 of every utterance live with score 0 and input bos, the others dead;
 *     an utterance whose kmask uint8 [B][Lk] (1 = masked; NULL = none) masks every frame has no
 *     live slot. Fills anc with each row's own index.
 *   ob_attdec_beam_step (step t): candidates are (r, topi[r][q]) for live slots r with score
 *     score[r] + ((double)topv[r][q] - lse[r]) and n = len[r] + 1, plus each finished slot itself,
 *     unchanged. The N candidates of largest key are kept in key order (ties: smaller slot, then
 *     smaller token); a selected eos finishes its slot; missing candidates leave dead slots.
 *     Writes the state in place, anc_out rows (anc_in's parent row for positions < t, the parent
 *     at position t; anc_in != anc_out) and the trace [L][B][N] at step t: trace_parent (slot,
 *     -1 for a dead slot), trace_token (-1 = finished slot carried over, -2 = dead slot),
 *     trace_score fp64.
 *   ob_attdec_finalize: hyp int32 [B][N][L] (tokens without eos, -1 after), hyp_len, n_hyp [B]
 *     (slots not dead), score_out fp64 [B][N] (-inf for dead slots), finished uint8 [B][N]: the
 *     layout of ob_ctc_beam_search_nbest, in the key order the last step left.
 * fp64 arrays 8-byte aligned, tok 8-byte, int32 arrays 4-byte.
 */
OB_API int ob_attdec_supported(int64_t N, int64_t d, int64_t H, int64_t Lk, int64_t L);
OB_API int ob_decattn_step(const float* qkv, int64_t sq, float* cache, const int32_t* anc,
                           const uint8_t* skip, int64_t R, int64_t H, int64_t dh, int64_t L,
                           int64_t t, float* ctx, void* stream);
OB_API size_t ob_seq_topk_workspace(int64_t R, int64_t d, int64_t V, int64_t K);
OB_API int ob_seq_topk(const float* hidden, int64_t R, int64_t d, const float* weight,
                       const float* bias, int64_t V, const int32_t* banned, int n_banned,
                       const uint8_t* skip, int64_t K, void* ws, size_t ws_bytes, double* lse,
                       float* topv, int32_t* topi, void* stream);
OB_API int ob_attdec_init(const uint8_t* kmask, int64_t B, int64_t N, int64_t Lk, int64_t L,
                          int bos, double* score, int32_t* len, uint8_t* fin, int64_t* tok,
                          uint8_t* skip, int32_t* anc, void* stream);
OB_API int ob_attdec_beam_step(const double* lse, const float* topv, const int32_t* topi,
                               int64_t B, int64_t N, int64_t K, int64_t L, int64_t t, int eos,
                               int pad, const double* norm, const int32_t* anc_in,
                               int32_t* anc_out, double* score, int32_t* len, uint8_t* fin,
                               int64_t* tok, uint8_t* skip, int32_t* trace_parent,
                               int32_t* trace_token, double* trace_score, void* stream);
OB_API int ob_attdec_finalize(const int32_t* trace_parent, const int32_t* trace_token,
                              const double* score, const int32_t* len, const uint8_t* fin,
                              int64_t B, int64_t N, int64_t L, int eos, int32_t* hyp,
                              int32_t* hyp_len, int32_t* n_hyp, double* score_out,
                              uint8_t* finished, void* stream);

/*
 * Joint CTC/attention beam search (csrc/ctcprefix.hip, csrc/attdec.hip): the attention search
 * above with every candidate scored by S = (1 - w) * A + w * C, A the sum of attention
 * log-probabilities, C the CTC prefix score log P_ctc(transcript starts with the prefix | audio)
 * -- for eos log P_ctc(prefix | audio) -- both products and the sum rounded in float64. Limits:
 * 1 <= N <= K <= 32 candidates per row, 1 <= T' <= 256 encoder frames, any V >= 1.
 * ob_ctc_prefix_supported(N, K, T') says so; ob_ctc_prefix_workspace(B, N, K, T') is the bytes of
 * the two state tables together (0 = unsupported); it does not depend on K. No entry allocates,
 * clears memory or synchronises; B == 0 is OB_OK with no launch.
 *
 * With lens int64 [B] (valid frames, clamped to 0..T'), x[t][v] = (double)logits[b][t][v] -
 * flse[b][t] for t < lens[b]:
 *   ob_ctc_frame_lse: flse fp64 [B][T'] = logsumexp of the fp32 CTC logits [B][T'][V] of frame t
 *     (fp64 sum of exp(z - max)) for t < lens[b]; later frames are neither read nor written.
 *   ob_ctc_prefix_step: for every row r = b * N + k with skip[r] == 0, whose prefix g is empty iff
 *     len[r] == 0, ends in tok[r] otherwise, and extends the prefix of row link[r][0] (whose last
 *     token is link[r][1]; its prefix is empty iff len[r] == 1): derives g's state from the
 *     parent's row of state_in and stores it in row r of state_out -- a state is fp64 [T'][2] =
 *     (gb[t], tot[t]), the log-probabilities that frames 0..t emit exactly g and end in a blank /
 *     end in anything; a table is [R][T'][2], frames >= lens[b] untouched -- then writes cpsi fp64
 *     [R][K]: for candidate c = topi[r][q] the prefix score psi(g . c); for c == eos
 *     tot[lens[b] - 1]; -inf for c == -1 or where no alignment exists (more tokens than frames, a
 *     repeated token without room for the blank). The root state needs no parent. Rows with
 *     skip[r] != 0 are left untouched in state_out and cpsi. state_in != state_out: a step reads
 *     one table and writes the other. Every sum has a fixed order that depends on the prefix
 *     alone: the same bits whichever slot holds a prefix. No NaN for finite logits.
 *   ob_attdec_joint_step: ob_attdec_beam_step on S. Extra state att, ctc fp64 [B][N] next to
 *     score (= S; the caller sets att = ctc = 0 for the live slot before step 0). A candidate has
 *     A' = att[r] + ((double)topv[r][q] - lse[r]), C' = cpsi[r][q], S' = (1 - w) * A' + w * C'; one
 *     with C' == -inf is dropped when w > 0; w == 0 gives S' = A' and drops nothing. Finished
 *     slots compete unchanged. Also writes link int32 [R][2] for the next ob_ctc_prefix_step:
 *     (the new row's parent row, the parent's last token or -1). trace_score holds S.
 *     ob_attdec_init and ob_attdec_finalize serve this search as they are.
 * fp64 arrays, lens and tok 8-byte aligned, int32 / fp32 arrays 4-byte.
 */
OB_API int ob_ctc_prefix_supported(int64_t N, int64_t K, int64_t Tp);
OB_API size_t ob_ctc_prefix_workspace(int64_t B, int64_t N, int64_t K, int64_t Tp);
OB_API int ob_ctc_frame_lse(const float* logits, const int64_t* lens, int64_t B, int64_t Tp,
                            int64_t V, double* flse, void* stream);
OB_API int ob_ctc_prefix_step(const float* logits, const double* flse, const int64_t* lens,
                              const int32_t* topi, const int64_t* tok, const int32_t* len,
                              const int32_t* link, const uint8_t* skip, int64_t B, int64_t N,
                              int64_t K, int64_t Tp, int64_t V, int blank, int eos,
                              const double* state_in, double* state_out, double* cpsi,
                              void* stream);
OB_API int ob_attdec_joint_step(const double* lse, const float* topv, const int32_t* topi,
                                const double* cpsi, double ctc_weight, int64_t B, int64_t N,
                                int64_t K, int64_t L, int64_t t, int eos, int pad,
                                const double* norm, const int32_t* anc_in, int32_t* anc_out,
                                double* score, double* att, double* ctc, int32_t* len,
                                uint8_t* fin, int64_t* tok, uint8_t* skip, int32_t* link,
                                int32_t* trace_parent, int32_t* trace_token, double* trace_score,
                                void* stream);

/*
 * N-gram LM shallow fusion (csrc/ngram.hip, csrc/ob_ngram.h; the fused step in csrc/attdec.hip,
 * the LM pick in csrc/rescore.hip): a back-off n-gram language model over the model's token ids,
 * order 1..4, V <= 65535 (ids 0..65534), as a third score source of the device decoders.
 * ob_ngram_supported(order, V, K): 1 <= order <= 4, 1 <= V <= 65535, 1 <= K <= 32 candidates per
 * row. The device entries take a stream, allocate nothing, need no workspace and no host
 * synchronisation and are capturable; B == 0 / R == 0 is OB_OK with no launch.
 *
 * Table: `slots` (a power of two, >= 2 x the entry count) 16-byte entries {uint64 key, float logp,
 * float backoff}, natural log. A key packs the n-gram (w_1 .. w_n) as four 16-bit fields of
 * (id + 1), w_n in bits 0..15, w_{n-1} in bits 16..31, ...; unused fields are 0, so the number of
 * non-zero fields is the order and key 0 is the empty slot. Home slot = mix(key) & (slots - 1)
 * with the splitmix64 finaliser as the mix, linear probing. Every entry sits within max_probe
 * <= 64 slots of its home; a lookup examines at most max_probe slots, hit or miss.
 *   ob_ngram_table_slots(n): the smallest table for n entries (0 = n out of range).
 *   ob_ngram_table_build (host, pure C): keys uint64 [n] (packed as above, distinct, no gap
 *     between fields: else OB_ERR_SHAPE), vals float [n][2] = (logp, backoff). Entries are
 *     inserted in key order into a zeroed table: the same entries in any order give the same
 *     bytes. The table doubles from ob_ngram_table_slots(n) until the longest probe run is <= 64;
 *     *slots and *max_probe always report the result. With table_bytes < *slots * 16 (or a null
 *     table) nothing is written and the status is OB_ERR_WORKSPACE: call again with that room.
 *
 * Context state: one uint64 per row, the same packing of the last three ids of the row's prefix
 * [bos] + tokens, the newest id in bits 0..15.
 *
 * Scoring rule. h = the last min(order - 1, len(prefix)) ids of the prefix; for candidate w:
 *     acc = 0 (fp64)
 *     for m = len(h) .. 0:
 *         if (h[-m:], w) is an entry:         return acc + logp
 *         if m >= 1 and h[-m:] is an entry:   acc += backoff
 *     return acc + unk_logp                   (w has no unigram)
 * Table values are float32, the sum is float64 in this order, so the result is a function of
 * (h, w) alone: the same bits on the host, on the device and in every slot. eos is scored as </s>
 * (the entry of its id). A candidate id < 0 is an absent candidate and scores -inf, as
 * ob_ctc_prefix_step scores c == -1; an id >= V has no entry and scores the chain + unk_logp.
 *   ob_ngram_score_host (host): out[q] = the rule for (ctx[q], w[q]), Q queries against a table
 *     in host memory, through the same probe routine as the kernels; probes int32 [Q] (may be
 *     NULL) = table slots examined for the query (the context chain included).
 *   ob_ngram_step: ob_ctc_prefix_step's twin. For every row r = b * N + k with skip[r] == 0:
 *     its context is [bos] when len[r] <= 0, [bos, tok[r]] when len[r] == 1, else the context of
 *     row link[r][0] in ctx_in extended by tok[r] (link[r][1] is not used); it is stored in
 *     ctx_out[r], and lmsc fp64 [R][K] receives the rule for each candidate topi[r][q]. Rows with
 *     skip[r] != 0 are left untouched in ctx_out and lmsc. ctx_in != ctx_out. The context's
 *     back-off chain is looked up once per row. One launch.
 *   ob_ngram_seq_logprob: hyp int32 [R][T] padded with -1, hyp_len int32 [R] (clamped to T) ->
 *     lm fp64 [R] = the sum, ascending position, of the rule over the row's tokens and the
 *     closing eos; a row with hyp_len < 0 is absent and gets -inf. tok_lm fp64 [R][T + 1] (may be
 *     NULL) receives the per-position scores, 0 past the eos and in absent rows.
 *   ob_attdec_fused_step: ob_attdec_joint_step with the LM term. Extra state lm fp64 [B][N] (the
 *     caller sets it 0 for the live slot before step 0). A candidate has A', C' as there,
 *     Lm' = lm[r] + lmsc[r][q] and S' = ((1 - w) * A' + w * C') + lm_weight * Lm', every product
 *     and sum rounded on its own in that order (w == 0: S' = A' + lm_weight * Lm', cpsi may be
 *     NULL and ctc stays 0). Dropping, finished slots, link, trace and norm as the joint step.
 *   ob_rescore_select_lm: ob_rescore_select with lm fp64 [B][N]: total = (att + ctc_weight * ctc)
 *     + lm_weight * lm, each operation rounded on its own. lp == NULL means no attention pass:
 *     total = ctc + lm_weight * lm, and ok / att may be NULL (every utterance counts as ok).
 *     Ties and the rescored / ok rules are unchanged.
 * fp64 / uint64 arrays and the table 8-byte (the table 16-byte) aligned, int32 arrays 4-byte.
 */
OB_API int ob_ngram_supported(int64_t order, int64_t V, int64_t K);
OB_API int64_t ob_ngram_table_slots(int64_t n_entries);
OB_API int ob_ngram_table_build(const uint64_t* keys, const float* vals, int64_t n_entries,
                                void* table, size_t table_bytes, int64_t* slots,
                                int32_t* max_probe);
OB_API int ob_ngram_score_host(const void* table, int64_t slots, int max_probe, int order,
                               int64_t V, double unk_logp, const uint64_t* ctx, const int32_t* w,
                               int64_t Q, double* out, int32_t* probes);
OB_API int ob_ngram_step(const void* table, int64_t slots, int max_probe, int order, int64_t V,
                         double unk_logp, const int32_t* topi, const int64_t* tok,
                         const int32_t* len, const int32_t* link, const uint8_t* skip, int64_t B,
                         int64_t N, int64_t K, int bos, const uint64_t* ctx_in, uint64_t* ctx_out,
                         double* lmsc, void* stream);
OB_API int ob_ngram_seq_logprob(const void* table, int64_t slots, int max_probe, int order,
                                int64_t V, double unk_logp, const int32_t* hyp,
                                const int32_t* hyp_len, int64_t R, int64_t T, int bos, int eos,
                                double* lm, double* tok_lm, void* stream);
OB_API int ob_attdec_fused_step(const double* lse, const float* topv, const int32_t* topi,
                                const double* cpsi, double ctc_weight, const double* lmsc,
                                double lm_weight, int64_t B, int64_t N, int64_t K, int64_t L,
                                int64_t t, int eos, int pad, const double* norm,
                                const int32_t* anc_in, int32_t* anc_out, double* score,
                                double* att, double* ctc, double* lm, int32_t* len, uint8_t* fin,
                                int64_t* tok, uint8_t* skip, int32_t* link, int32_t* trace_parent,
                                int32_t* trace_token, double* trace_score, void* stream);
OB_API int ob_rescore_select_lm(const float* lp, const int32_t* hyp, const int32_t* hyp_len,
                                const int32_t* n_hyp, const double* ctc_score, const double* lm,
                                const uint8_t* ok, int64_t B, int64_t N, int64_t T, int64_t Lc,
                                double ctc_weight, double lm_weight, int32_t* out,
                                int32_t* out_len, int32_t* best_k, double* att, double* total,
                                uint8_t* rescored, void* stream);

/*
 * CTC prefix beam search with the n-gram LM inside the search (first-pass fusion; csrc/beam.hip).
 * The search of ob_ctc_beam_search_nbest, unchanged in every respect -- the K candidates per
 * frame, the three transitions with the repeat rule, the merges, the dict-insertion tie order --
 * except for what a frame's pruning compares. Every live prefix y also carries n = len(y) and
 *     lm(y) = sum over j of score([bos] + y[:j], y[j])        (the scoring rule above)
 * an fp64 sum in ascending position that starts at 0 for the empty prefix. lm(y) is a function of
 * the tuple alone: an extension that lands on a live prefix folds only its CTC mass into it, and
 * both copies hold the same LM bits. After each frame the beam prefixes with the largest
 *     key(y) = (lse(p_b, p_nb) + lm_weight * lm(y)) + ins_bonus * n
 * stay, every operation rounded on its own in fp64 (no contraction: the convention of S' in
 * ob_attdec_fused_step); exact ties keep the order of ob_ctc_beam_search. After the last frame
 *     lm_fin(y) = lm(y) + score([bos] + y, eos)
 *     total(y)  = (ctc(y) + lm_weight * lm_fin(y)) + ins_bonus * n,      ctc = lse(p_b, p_nb)
 * and the final beam is ordered by total descending (ties keep the beam's order); its first nbest
 * entries are returned. An utterance with lens[b] == 0 returns the empty hypothesis: ctc 0,
 * lm = score([bos], eos). With lm_weight == 0 and ins_bonus == 0 the hypotheses, their order and
 * ctc are ob_ctc_beam_search_nbest's bit for bit.
 *   Arguments of ob_ctc_beam_search_nbest with the same limits, and the table arguments of
 *   ob_ngram_step (table, slots, max_probe, order, unk_logp; V is the logits' V) with theirs:
 *   1 <= order <= 4 and V <= 65535; bos, eos in [0, V); lm_weight >= 0, ins_bonus and unk_logp
 *   finite (else OB_ERR_SHAPE). ins_bonus is the usual insertion bonus that offsets the LM's
 *   preference for short output.
 *   hyp int32 [B][nbest][T], hyp_len int32 [B][nbest], n_hyp int32 [B] as there; ctc, lm (lm_fin)
 *   and total fp64 [B][nbest], 8-byte aligned, required; absent entries hold -inf and hyp_len 0.
 *   ws: ob_ctc_beam_search_lm_workspace(B, T, V, beam, top_k, order) bytes, 0 for an unsupported
 *   shape (the n-best call's size otherwise).
 * Two launches on the stream, no host synchronisation, capturable. B == 0 is OB_OK with no launch.
 */
OB_API size_t ob_ctc_beam_search_lm_workspace(int64_t B, int64_t T, int64_t V, int beam,
                                              int top_k, int order);
OB_API int ob_ctc_beam_search_lm(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                                 int64_t V, int blank, int beam, int top_k, int nbest,
                                 const void* table, int64_t slots, int max_probe, int order,
                                 double unk_logp, int bos, int eos, double lm_weight,
                                 double ins_bonus, void* ws, size_t ws_bytes, int32_t* hyp,
                                 int32_t* hyp_len, int32_t* n_hyp, double* ctc, double* lm,
                                 double* total, void* stream);

/*
 * Contextual biasing (csrc/bias.hip, csrc/ob_bias.h; the biased step in csrc/attdec.hip, the biased
 * CTC search in csrc/beam.hip): a list of phrases over the model's token ids that the beam searches
 * should prefer, as a fourth score source. ob_bias_supported(V, K, n_nodes): 1 <= V <= 65535,
 * 1 <= K <= 32 candidates per row, 1 <= n_nodes <= 2^30. The device entries take a stream, allocate
 * nothing, need no workspace and no host synchronisation and are capturable; B == 0 / R == 0 is
 * OB_OK with no launch.
 *
 * The phrase list and its automaton. A phrase is 1..16 token ids in 0..65534 with a boost b > 0
 * (float32, per token, finite); the same phrase given twice keeps the larger boost. The phrases
 * form a trie: node 0 is the root, the other nodes are numbered breadth-first by depth and within
 * a depth by (parent number, token) ascending, so the same phrases in any order give the same
 * bytes. With val(n, b) = float32 of the float64 product n * b, each node p (a token path) carries
 *     commit(p) = the maximum of val(len q, b_q) over phrases q that are a prefix of p (q == p
 *                 included), 0 when there is none
 *     phi(p)    = the maximum of commit(p) and val(len p, b_q) over phrases q that p is a prefix
 *                 of; phi(root) = 0
 *     fail(p)   = the longest proper suffix of p that is a node (the root if none)
 *     has_children(p)
 * Nodes: n_nodes 16-byte records {int32 fail, int32 flags (bit 0: has children), float phi, float
 * commit}. Edges: an open-addressed table of `slots` (a power of two, >= 2 x (n_nodes - 1)) 16-byte
 * entries {uint64 key, int32 child, int32 0}, key = ((node + 1) << 16) | (tok + 1), key 0 the empty
 * slot, home slot = mix(key) & (slots - 1) with the splitmix64 finaliser, linear probing, every
 * edge within max_probe <= 64 slots of its home, inserted in key order into a zeroed table: the
 * n-gram table's contract.
 *
 * The step. A hypothesis y carries (state, kept), a node (int32) and an fp64, (root, 0.0) for the
 * empty y. Extending by token w:
 *     u = state
 *     loop:  if child(u, w) exists:  t = child(u, w); break
 *            if commit(u) > 0:       kept += commit(u); t = child(root, w) or root; break
 *            if u == root:           t = root; break
 *            u = fail(u)
 *     if t != root and not has_children(t):   kept += commit(t); t = root
 *     state = t
 * The loop makes at most 17 lookups. Matches are left to right and never overlap: a commit always
 * restarts at the root.
 *     bias(y)     = kept + (double)phi(state)      the running value, partial matches counted
 *     bias_fin(y) = kept + (double)commit(state)   the closed value, an unfinished partial match
 *                                                  taken back
 * Both are functions of the token tuple alone; kept is an fp64 sum of float32 values in a fixed
 * order, so the host, the device and every beam slot hold the same bits, and a CTC merge keeps one
 * value, as with lm(y).
 *   ob_bias_sizes: *max_nodes = total_tokens + 1 and *min_slots, the bounds of what ob_bias_build
 *     reports for n_phrases phrases of total_tokens tokens (OB_ERR_SHAPE when out of range).
 *   ob_bias_build (host, pure C): tokens int32 (the phrases back to back), lengths int32
 *     [n_phrases], boosts float [n_phrases] -> nodes, edges, *n_nodes, *slots, *max_probe. An empty
 *     phrase, a length > 16, an id outside 0..65534, a boost that is not finite or not positive:
 *     OB_ERR_SHAPE. The edge table doubles until the longest probe run is <= 64; *n_nodes, *slots
 *     and *max_probe always report the result. With nodes_bytes < *n_nodes * 16 or edges_bytes <
 *     *slots * 16 (or a null buffer) nothing is written and the status is OB_ERR_WORKSPACE: call
 *     again with that room.
 *   ob_bias_walk_host (host): tokens int32 [Q][T], lens int32 [Q] (clamped to 0..T) -> per row the
 *     state, kept, bias and bias_fin of its tokens, tables in host memory, through the same lookup
 *     routine as the kernels.
 *   ob_bias_step: ob_ngram_step's twin. For every row r = b * N + k with skip[r] == 0: its
 *     (state, kept) is the root's when len[r] <= 0, the root extended by tok[r] when len[r] == 1,
 *     else that of row link[r][0] in st_in / kept_in extended by tok[r]; it is stored in st_out[r]
 *     / kept_out[r], and bsc fp64 [R][K] receives bias(y . c) for each candidate c = topi[r][q]
 *     >= 0, c != eos, bias_fin(y) for c == eos and -inf for c < 0. Rows with skip[r] != 0 are left
 *     untouched. st_in != st_out, kept_in != kept_out. One launch.
 *   ob_bias_seq_score: hyp int32 [R][T] padded with -1, hyp_len int32 [R] (clamped to T) ->
 *     bias_fin fp64 [R]; a row with hyp_len < 0 is absent and gets -inf.
 *   ob_attdec_biased_step: ob_attdec_fused_step with the bias term, through the same kernel. Extra
 *     state bias fp64 [B][N]. A candidate has A', C', Lm' as there and Bi' = bsc[r][q], an absolute
 *     value, not an accumulated one;
 *         S' = (((1 - w) * A' + w * C') + lm_weight * Lm') + bias_weight * Bi'
 *     each operation rounded on its own, no contraction. lmsc == NULL: Lm' = 0, lm is not touched
 *     (may be NULL) and lm_weight must be 0. bias_weight >= 0 and finite (else OB_ERR_SHAPE).
 *     Finished slots keep their terms.
 *   ob_ctc_beam_search_bias: ob_ctc_beam_search_lm with the bias inside the search. Every live
 *     prefix also carries (state, kept); after each frame the beam prefixes with the largest
 *         key(y) = ((lse(p_b, p_nb) + lm_weight * lm(y)) + ins_bonus * n) + bias_weight * bias(y)
 *     stay, and after the last frame
 *         total(y) = ((ctc(y) + lm_weight * lm_fin(y)) + ins_bonus * n) + bias_weight * bias_fin(y)
 *     orders the final beam (ties keep the beam's order); bias fp64 [B][nbest] receives bias_fin,
 *     -inf for absent entries. table == NULL is the search without an LM: lm(y) = lm_fin = 0,
 *     lm_weight must be 0, the other table arguments are not read and the lm output is 0 for
 *     present entries. V <= 65535. With bias_weight == 0 the hypotheses, their order, ctc, lm and
 *     total are ob_ctc_beam_search_lm's bit for bit, and additionally with no LM and ins_bonus == 0
 *     ob_ctc_beam_search_nbest's. lens[b] == 0 returns the empty hypothesis with bias = 0.
 *     ws: ob_ctc_beam_search_bias_workspace(B, T, V, beam, top_k, order, n_nodes) bytes (order 0:
 *     no LM), 0 for an unsupported shape.
 * The tables 16-byte aligned, fp64 / int64 arrays 8-byte, int32 arrays 4-byte.
 */
OB_API int ob_bias_supported(int64_t V, int64_t K, int64_t n_nodes);
OB_API int ob_bias_sizes(int64_t n_phrases, int64_t total_tokens, int64_t* max_nodes,
                         int64_t* min_slots);
OB_API int ob_bias_build(const int32_t* tokens, const int32_t* lengths, const float* boosts,
                         int64_t n_phrases, void* nodes, size_t nodes_bytes, void* edges,
                         size_t edges_bytes, int64_t* n_nodes, int64_t* slots,
                         int32_t* max_probe);
OB_API int ob_bias_walk_host(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                             int max_probe, const int32_t* tokens, const int32_t* lens, int64_t Q,
                             int64_t T, int32_t* state, double* kept, double* bias,
                             double* bias_fin);
OB_API int ob_bias_step(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                        int max_probe, const int32_t* topi, const int64_t* tok,
                        const int32_t* len, const int32_t* link, const uint8_t* skip, int64_t B,
                        int64_t N, int64_t K, int eos, const int32_t* st_in, int32_t* st_out,
                        const double* kept_in, double* kept_out, double* bsc, void* stream);
OB_API int ob_bias_seq_score(const void* nodes, int64_t n_nodes, const void* edges, int64_t slots,
                             int max_probe, const int32_t* hyp, const int32_t* hyp_len, int64_t R,
                             int64_t T, double* bias_fin, void* stream);
OB_API int ob_attdec_biased_step(const double* lse, const float* topv, const int32_t* topi,
                                 const double* cpsi, double ctc_weight, const double* lmsc,
                                 double lm_weight, const double* bsc, double bias_weight,
                                 int64_t B, int64_t N, int64_t K, int64_t L, int64_t t, int eos,
                                 int pad, const double* norm, const int32_t* anc_in,
                                 int32_t* anc_out, double* score, double* att, double* ctc,
                                 double* lm, double* bias, int32_t* len, uint8_t* fin,
                                 int64_t* tok, uint8_t* skip, int32_t* link,
                                 int32_t* trace_parent, int32_t* trace_token, double* trace_score,
                                 void* stream);
OB_API size_t ob_ctc_beam_search_bias_workspace(int64_t B, int64_t T, int64_t V, int beam,
                                                int top_k, int order, int64_t n_nodes);
OB_API int ob_ctc_beam_search_bias(const float* logits, const int64_t* lens, int64_t B, int64_t T,
                                   int64_t V, int blank, int beam, int top_k, int nbest,
                                   const void* table, int64_t slots, int max_probe, int order,
                                   double unk_logp, int bos, int eos, double lm_weight,
                                   double ins_bonus, const void* bias_nodes, int64_t n_nodes,
                                   const void* bias_edges, int64_t bias_slots, int bias_max_probe,
                                   double bias_weight, void* ws, size_t ws_bytes, int32_t* hyp,
                                   int32_t* hyp_len, int32_t* n_hyp, double* ctc, double* lm,
                                   double* bias, double* total, void* stream);

/*
 * CTC forced alignment (csrc/align.hip): the Viterbi path of a given token sequence through the
 * CTC trellis of the logits, with the frame span and the score of every token, on the device.
 * Inputs: logits fp32 [B][T'][V]; lens int64 [B] (valid frames, clamped to 0..T'); targets int32
 * [B][S] (padded, any value past tlen[b]); tlen int32 [B] (clamped to 0..S); blank in [0, V).
 * With x[t][v] = (double)logits[b][t][v] - flse[b][t], flse the fp64 log-sum-exp of the frame
 * (ob_ctc_frame_lse's arithmetic), trellis values in fp64, v_t(s) = max(allowed predecessors) +
 * x[t][label(s)] over the extended labels and the skip rule of the CTC loss.
 * Outputs, every element written by the call:
 *   path int32 [B][T']: the token id emitted at frame t, blank for a blank frame; -1 for
 *     t >= lens[b] and for an infeasible utterance.
 *   span int32 [B][S][2]: (first frame, last frame + 1) of token u's own trellis state (the frames
 *     are contiguous); (-1, -1) for u >= tlen[b] and for an infeasible utterance.
 *   tok_score fp64 [B][S]: the sum of x[t][targets[b][u]] over the token's span, in frame order; 0
 *     where span is -1.
 *   score fp64 [B]: the Viterbi log-probability, the sum of x[t][path[t]] over t < lens[b]; -inf
 *     when no alignment exists: more tokens than frames, a repeated token without room for its
 *     blank, lens == 0 with tlen > 0, or a target token outside [0, V) or equal to blank (such a
 *     token is never used as an index). lens == 0 with tlen == 0 is feasible with score 0;
 *     tlen == 0 with lens > 0 is the all-blank path.
 * Ties: among equal predecessors stay (s) wins over s - 1, which wins over s - 2; at the last
 * frame the final token state 2 tlen - 1 wins against the trailing blank state 2 tlen. The path is
 * therefore a pure function of the utterance's own logits and target. No atomics, every word one
 * writer: an utterance gets the same bits in every batch slot, for every padded T' and S at least
 * as large as its own, and in every run.
 * Limits: 1 <= T' <= 4096, 0 <= S <= 511, V >= 1, B * T' < 2^31; ob_ctc_align_supported(T', S)
 * says so; ob_ctc_align_workspace(B, T', S) is the bytes of ws (0 = unsupported): the emission
 * rows fp64 [B][T'][S + 1] and one back-pointer byte per (b, t, state). S == 0 is legal; targets,
 * span and tok_score may then be NULL. No entry allocates, clears memory or synchronises; B == 0
 * is OB_OK with no launch. fp64 arrays, lens and ws 8-byte aligned, int32 / fp32 arrays 4-byte.
 */
OB_API int ob_ctc_align_supported(int64_t Tp, int64_t S);
OB_API size_t ob_ctc_align_workspace(int64_t B, int64_t Tp, int64_t S);
OB_API int ob_ctc_align(const float* logits, const int64_t* lens, const int32_t* targets,
                        const int32_t* tlen, int64_t B, int64_t Tp, int64_t V, int64_t S,
                        int blank, void* ws, size_t ws_bytes, int32_t* path, int32_t* span,
                        double* tok_score, double* score, void* stream);
/* The phases of ob_ctc_align on their own (stage 0: all, the call above), for timing: stage 1 runs
 * the emission launch only and leaves the emission rows in ws (the outputs are not touched and may
 * be NULL); stage 2 runs the trellis launch only (recursion, walk, outputs) on the rows a stage 1
 * call with the same shapes, lens, targets and tlen left in the same ws (logits may be NULL);
 * stage 3 is stage 2 without the walk: it writes score only (path, span, tok_score may be NULL). */
OB_API int ob_ctc_align_stage(const float* logits, const int64_t* lens, const int32_t* targets,
                              const int32_t* tlen, int64_t B, int64_t Tp, int64_t V, int64_t S,
                              int blank, int stage, void* ws, size_t ws_bytes, int32_t* path,
                              int32_t* span, double* tok_score, double* score, void* stream);

/*
 * Edit distance, error counts and minimum-Bayes-risk selection (csrc/edit.hip, the DP in
 * csrc/ob_edit.h): batched Levenshtein distance over padded int32 sequences, on the device.
 * Definition, a the reference and b the hypothesis, a cell a tuple (d, sub, ins, del):
 *   D[0][j] = (j, 0, j, 0);  D[i][0] = (i, 0, 0, i);
 *   a[i-1] == b[j-1]:  D[i][j] = D[i-1][j-1], unchanged;
 *   otherwise the candidate with the smallest d among the diagonal D[i-1][j-1] (a substitution),
 *   up D[i-1][j] (a deletion of a reference token) and left D[i][j-1] (an insertion of a
 *   hypothesis token), ties in that order; d and the chosen neighbour's count grow by 1.
 * The result is D[len a][len b]: d == sub + ins + del, len b - len a == ins - del, and d is the
 * Levenshtein distance. The counts travel with the cell; there is no backtrace. Any int32 is a
 * token. Results are integers and a function of the inputs alone: no atomics, every word one
 * writer. No entry allocates, clears memory or synchronises; all are capturable in a HIP graph.
 * int32 arrays 4-byte aligned, fp64 arrays and ws 8-byte aligned.
 *
 * ob_edit_distance: a int32 [P][La] with a_len int32 [P], b int32 [P][Lb] with b_len int32 [P];
 *   padding may hold anything; a length above the width is clamped to it; a pair with a negative
 *   length is absent. dist int32 [P]; ops int32 [P][3] = (sub, ins, del), may be NULL (distance
 *   only, a cheaper kernel); an absent pair gets dist = -1 and ops = -1. a (b) may be NULL when
 *   La (Lb) is 0. Limits: 0 <= La, Lb <= 4096 (ob_edit_supported), 0 <= P < 2^31; anything else is
 *   OB_ERR_SHAPE. ob_edit_distance_workspace(P, La, Lb) is the bytes of ws (0 = unsupported): one
 *   row of Lb cells per wave in flight, for the band boundary of references longer than 64.
 *   P == 0 is OB_OK with no launch.
 *
 * ob_nbest_edit_distance: hyp int32 [B][N][T], hyp_len [B][N], n_hyp [B] in the layout of
 *   ob_ctc_beam_search_nbest (n_hyp clamped to 0..N, hyp_len to 0..T); optionally ref int32 [B][S]
 *   with ref_len [B] (clamped to S; negative = no reference for the utterance). One launch:
 *   dref int32 [B][N]: the distance of every live entry to its utterance's reference, with
 *   ops_ref int32 [B][N][3] as above; both -1 for absent entries k >= n_hyp[b] and for an
 *   utterance without a reference.
 *   dpair int32 [B][N][N]: the distances among the live entries, computed for j < k and mirrored;
 *   0 on the diagonal of live entries; -1 in the rows and columns of absent entries.
 *   dref, ops_ref and dpair may each be NULL, not all three; ref and ref_len are read only when
 *   dref or ops_ref is given. Limits: 1 <= N <= 32, 0 <= T, S <= 4096, B * N * (N + 3) / 2 < 2^31.
 *   ob_nbest_edit_distance_workspace(B, N, T, S): bytes of ws for any choice of outputs.
 *   B == 0 is OB_OK with no launch.
 *
 * ob_mbr_select: the minimum-Bayes-risk entry of every n-best. dpair as above, score fp64 [B][N],
 *   scale finite and >= 0 (else OB_ERR_SHAPE). Per utterance over the live entries, in fp64 and in
 *   ascending index order, every product and sum rounded on its own (no fused multiply-add):
 *     m = max score;  w_j = exp(scale * (score_j - m)), 0 for score_j = -inf;  Z = sum_j w_j;
 *     post_j = w_j / Z;  risk_k = sum_j post_j * dpair[k][j];
 *   best_k int32 [B]: the smallest risk, ties to the smaller k; out int32 [B][T] (its tokens, -1
 *   after) and out_len int32 [B]; risk fp64 [B][N], +inf for absent entries; post fp64 [B][N], 0
 *   for absent entries. n_hyp[b] == 0: out_len 0, out all -1, best_k 0. When the largest live
 *   score is -inf (an utterance that rescoring skipped), entry 0 wins, every risk is +inf and every
 *   post 0. hyp and out may be NULL when T == 0. Limits as above. B == 0 is OB_OK with no launch.
 */
OB_API int ob_edit_supported(int64_t La, int64_t Lb);
OB_API size_t ob_edit_distance_workspace(int64_t P, int64_t La, int64_t Lb);
OB_API int ob_edit_distance(const int32_t* a, const int32_t* a_len, const int32_t* b,
                            const int32_t* b_len, int64_t P, int64_t La, int64_t Lb, void* ws,
                            size_t ws_bytes, int32_t* dist, int32_t* ops, void* stream);
OB_API size_t ob_nbest_edit_distance_workspace(int64_t B, int64_t N, int64_t T, int64_t S);
OB_API int ob_nbest_edit_distance(const int32_t* hyp, const int32_t* hyp_len,
                                  const int32_t* n_hyp, const int32_t* ref,
                                  const int32_t* ref_len, int64_t B, int64_t N, int64_t T,
                                  int64_t S, void* ws, size_t ws_bytes, int32_t* dref,
                                  int32_t* ops_ref, int32_t* dpair, void* stream);
OB_API int ob_mbr_select(const int32_t* dpair, const int32_t* hyp, const int32_t* hyp_len,
                         const int32_t* n_hyp, const double* score, double scale, int64_t B,
                         int64_t N, int64_t T, int32_t* out, int32_t* out_len, int32_t* best_k,
                         double* risk, double* post, void* stream);

/*
 * Minimum-WER training over the CTC n-best (csrc/ctcnbest.hip, the recursions of csrc/ctc.hip):
 * the CTC log-likelihood of every entry of an n-best straight from the CTC head's logits, the
 * expected-error loss over the entries' posterior, and the gradient w.r.t. the logits.
 * logits fp32 [B][T][V] (16-byte aligned when V % 4 == 0), lens int64 [B] (clamped to 0..T), hyp
 * int32 [B][N][Th] with hyp_len int32 [B][N] and n_hyp int32 [B] in the layout of
 * ob_ctc_beam_search_nbest (n_hyp clamped to 0..N, hyp_len to 0..Th; padding may hold anything;
 * a token outside [0, V) reads and writes the nearest valid column). No entry allocates, clears
 * memory or synchronises; all are capturable in a HIP graph; no float atomics, every sum in a
 * fixed order: the same bits run to run, and for an utterance in any batch slot. int32 arrays
 * 4-byte aligned, fp64 arrays 8-byte aligned, ws 256-byte aligned.
 * Limits: 1 <= N <= 32, 0 <= Th <= 511 (ob_ctc_nbest_supported), B >= 1, T >= 1, 1 <= V < 2^31,
 * 0 <= blank < V, B * T and B * N * T < 2^31; anything else is OB_ERR_SHAPE with no launch.
 *
 * ob_ctc_nbest_workspace(B, N, T, Th): the bytes of ws (0 = unsupported). ws holds, for the
 *   B * N compact problems: alpha and beta fp32 [B*N][T][2 Th + 1], nll fp32 [B*N], the compact
 *   log-probs lpc fp32 [(b N + k) T + t][Th + 1] (index 0 blank, 1 + u token u of entry k), the
 *   row max and log-sum-exp fp32 [B*T][2], the compact labels int64 [B*N][Th] (equal tokens
 *   share the label of their first occurrence; a token equal to blank is label 0), the expanded
 *   lengths int64 [B*N] twice and the same-label chains int32 [B*N][2][2 Th + 1].
 *
 * ob_ctc_nbest_logprob: one gather launch (one block per frame: the row's max and log-sum-exp
 *   computed once, with the operations of the training CTC's gather, then the compact log-probs
 *   of every live entry) and one launch of the training CTC's alpha and beta recursions over the
 *   2 B N compact problems, fp32. ll fp64 [B][N] = log p_ctc(entry k | logits b): -inf for an
 *   entry CTC cannot align (more tokens than frames, a repeat without a frame for the blank
 *   between, an utterance with lens 0) and for absent entries k >= n_hyp[b]; the all-blank path
 *   for an empty entry. ws keeps the state ob_ctc_nbest_grad needs.
 *
 * ob_mwer_combine: ll, err fp64 [B][N], scale finite and >= 0 (else OB_ERR_SHAPE). Entry k of
 *   utterance b is live when k < n_hyp[b] and ll is finite. Per utterance with at least two live
 *   entries, in fp64 and in ascending k:
 *     m = max ll;  w_k = exp(scale * (ll_k - m));  post_k = w_k / sum_j w_j;
 *     risk_b = sum_k post_k * err_k;  base_b = (sum_k err_k) / live;  loss_b = risk_b - base_b;
 *     coef[b][k] = scale * post_k * (err_k - risk_b) / B     ( = d loss / d ll[b][k] )
 *   post and coef are 0 for entries that are not live; an utterance with fewer than two live
 *   entries has loss_b = 0 and coef = 0 (post 1 on its one live entry, risk its err).
 *   loss fp64 [1] = (sum_b loss_b) / B in ascending b; post, coef fp64 [B][N]; risk fp64 [B].
 *
 * ob_ctc_nbest_grad: after ob_ctc_nbest_logprob with the same arguments and ws. coef fp64
 *   [B][N] = d L / d ll, grad_out fp32 [1] the upstream gradient g of L (NULL: 1). One block
 *   per frame writes the whole row of grad fp32 [B][T][V] (grad is not read before): zeros;
 *   with dense != 0, -g * (sum_k coef_k) * softmax(logits row) first; then, for k ascending,
 *   every entry with coef != 0 and ll finite adds g * coef_k * exp(acc + nll_k - lp) at blank and
 *   at each of its distinct tokens (acc the log-sum of alpha + beta over the label's states),
 *   the entries separated by a block barrier. Frames t >= lens[b] are zero rows. With dense == 0
 *   (sum_k coef_k == 0, as ob_mwer_combine's) the columns outside blank and the n-best's tokens
 *   are exactly 0.
 */
OB_API int ob_ctc_nbest_supported(int64_t N, int64_t Th);
OB_API size_t ob_ctc_nbest_workspace(int64_t B, int64_t N, int64_t T, int64_t Th);
OB_API int ob_ctc_nbest_logprob(const float* logits, const int64_t* lens, const int32_t* hyp,
                                const int32_t* hyp_len, const int32_t* n_hyp, int64_t B,
                                int64_t N, int64_t T, int64_t V, int64_t Th, int blank, void* ws,
                                size_t ws_bytes, double* ll, void* stream);
OB_API int ob_mwer_combine(const double* ll, const double* err, const int32_t* n_hyp, double scale,
                           int64_t B, int64_t N, double* loss, double* post, double* risk,
                           double* coef, void* stream);
OB_API int ob_ctc_nbest_grad(const float* logits, const int64_t* lens, const int32_t* hyp,
                             const int32_t* hyp_len, const int32_t* n_hyp, int64_t B, int64_t N,
                             int64_t T, int64_t V, int64_t Th, int blank, const double* coef,
                             const float* grad_out, int dense, void* ws, size_t ws_bytes,
                             float* grad, void* stream);

/*
 * Feature front end: Kaldi fbank + CMVN + SpecAugment + zero-padded collate for a padded batch
 * of 16 kHz waveforms, one launch. Replaces src/data/dataset.py:117-135 (torchaudio.compliance.
 * kaldi.fbank(waveform, num_mel_bins=80, sample_frequency=16000) with its defaults, then
 * (fbank - mean) / std, then SpecAugment), :150-209 (SpecAugment) and the feature half of the
 * collate, :245-273. Fixed options: dither 0, 25 ms frames (400 samples) every 10 ms (160),
 * pre-emphasis 0.97, DC removal, povey window, 512-point FFT, 20 Hz .. 8 kHz, snip_edges, power
 * spectrum, log, no energy, no mean subtraction, samples at the amplitude given.
 * For utterance b with n = clamp(wave_lens[b], 0, n_max) samples:
 *   m = n < 400 ? 0 : 1 + (n - 400) / 160 frames; frame i is samples [160 i, 160 i + 400);
 *   x -= mean(x) over the frame; y[j] = x[j] - 0.97 x[max(j - 1, 0)]; y[j] *= window[j];
 *   P[k] = |rfft_512(y)[k]|^2; E[f] = sum_k bank[f][k] P[k] (k ascending, fp32);
 *   v = logf(max(E[f], 1.1920929e-07f)); with CMVN v = (v - cmvn_mean[f]) / cmvn_std[f] (a
 *   true division);
 *   with mask_starts (int32 [B][n_fmask + n_tmask], frequency masks first): v = 0.0 where
 *   s <= f < s + min(fmask_w, n_mels) for a frequency start s, or s <= i < s + min(tmask_w, m)
 *   for a time start s (fixed widths, as the reference's SpecAugment has them; an utterance
 *   with m <= tmask_w is zeroed whole by a time mask that starts at 0);
 *   feats[b][i][f] = v for i < m and 0.0 for m <= i < T; feat_lens[b] = m.
 * The output is a pure function of the inputs: fixed summation order, no atomics.
 *
 * ob_fbank_num_frames: m for n samples (host arithmetic; 0 for n < 400).
 * ob_frontend_table_floats / ob_frontend_table_fill: the constant table the kernel reads, built
 * on the HOST in fp64 and rounded to fp32; the caller uploads it once (the library allocates
 * nothing). 0 / OB_ERR_SHAPE for n_mels outside 1..128. Layout, in floats:
 *   [0, 400)        window[j] = (0.5 - 0.5 cos(2 pi j / 399))^0.85
 *   [400, 1424)     (cos, -sin)(2 pi t / 512), t = 0..511
 *   [1424, +3 n_mels)  per filter f: first bin, number of bins, offset into the weights (whole
 *                   numbers stored as floats); a filter's non-zero bins are contiguous
 *   [.., +512)      the weights, filter after filter; unused tail 0
 * Filter f of n_mels is the triangle with corners mel(20) + (f, f + 1, f + 2) d in
 * mel(x) = 1127 ln(1 + x / 700), d = (mel(8000) - mel(20)) / (n_mels + 1), evaluated at the
 * bins' mel(31.25 k), k = 0..255; bin 256 has weight 0.
 *
 * ob_frontend_fwd: wave fp32 [B][wave_stride] (wave_stride >= n_max; only the first n samples
 * of a row are read); wave_lens int64 [B] (device), values above n_max are clamped; table as
 * above (device); cmvn_mean / cmvn_std fp32 [n_mels], both or neither; mask_starts may be NULL
 * (no SpecAugment); feats fp32 [B][T][n_mels] with T >= ob_fbank_num_frames(n_max); feat_lens
 * int64 [B]. B == 0 is OB_OK with no launch. B * ceil(T / 16) < 2^31.
 */
OB_API int64_t ob_fbank_num_frames(int64_t n_samples);
OB_API int64_t ob_frontend_table_floats(int n_mels);
OB_API int ob_frontend_table_fill(float* host_table, int n_mels);
OB_API int ob_frontend_fwd(const float* wave, int64_t wave_stride, const int64_t* wave_lens,
                           int64_t B, int64_t n_max, const float* table, int n_mels,
                           const float* cmvn_mean, const float* cmvn_std,
                           const int32_t* mask_starts, int n_fmask, int fmask_w, int n_tmask,
                           int tmask_w, float* feats, int64_t T, int64_t* feat_lens,
                           void* stream);

/* ------------------------------------------------------------------------------------
 * Fused epilogues: the elementwise ops that follow a BitLinear GEMM at its call sites in
 * the reference, applied in the GEMM's store instead of separate torch kernels.
 * X / Y rows are P stacked passes as in ob_bitlinear_fwd_passes; pass_bits may be NULL
 * when P == 1 (codes2 is used). Element (row, col) of a [P*M][N] output has dropout index
 * row * N + col; keep = hash(seed, counter, index) >= p * 2^32, kept values scale by
 * 1 / (1 - p); rng is a DEVICE {seed, counter} int64[2] (required when p_drop > 0) and the
 * mask is drawn for counter + rng_offset (a per-call-site offset: no per-call device copy).
 * Outputs must not alias inputs.
 *
 * swish_drop   Y_pre = a X.Q^T + b;  Y_act = dropout(silu(Y_pre))
 *              (FeedForwardModule lin1 -> swish -> dropout, conformer.py:36-38)
 * residual     Y = R + rscale * rowvalid * dropout(a X.Q^T + b),
 *              rowvalid = (lens == NULL) || (row % T < lens[row / T])
 *              (lin2 -> dropout -> x + 0.5 h, conformer.py:39-45, rscale 0.5, lens NULL;
 *               out_proj -> dropout -> pad zero -> x + out, conformer.py:131-138, rscale 1)
 * bwd_dx_swish_drop
 *              dPre = (a dY.Q) * keep * scale * silu'(pre): the dX GEMM of lin2 chained
 *              through the dropout and swish backward of swish_drop (same rng, same p)
 * drop_scale_bwd
 *              dY = rscale * rowvalid * dropout(dOut) with the residual entry's mask:
 *              the gradient of `residual`'s output w.r.t. its GEMM output.
 * ------------------------------------------------------------------------------------ */
OB_API int ob_bitlinear_fwd_swish_drop(const float* X, int64_t P, int64_t M, int64_t K,
                                       const uint32_t* codes2, const uint32_t* codes1,
                                       const int32_t* pass_bits, const float* alpha,
                                       int alpha_raw, const float* bias, int64_t N, float p_drop,
                                       const uint64_t* rng, int64_t rng_offset, float* Y_pre,
                                       float* Y_act, void* stream);
OB_API int ob_bitlinear_fwd_residual(const float* X, int64_t P, int64_t M, int64_t K,
                                     const uint32_t* codes2, const uint32_t* codes1,
                                     const int32_t* pass_bits, const float* alpha, int alpha_raw,
                                     const float* bias, int64_t N, const float* R, float rscale,
                                     float p_drop, const uint64_t* rng, int64_t rng_offset,
                                     const int32_t* lens, int64_t T, float* Y, void* stream);
/* ob_bitlinear_fwd_residual whose epilogue also forms the LayerNorm(s) that read Y next
 * (conformer.py:19-24, nn.LayerNorm(d)): nln = 1: ln_y0 = LN0(Y) with its per-row mean / rstd
 * (the statistics ob_layernorm_bwd takes); nln = 2: also ln_y1 = LN1(ln_y0) (a block's final LN
 * and the next block's first, as ob_layernorm_fwd_pair). Same row arithmetic as the LN kernels
 * (bit-identical results). Taken for the K = 576 byte-image launch with N = 144 (the Conformer
 * FFN's second linear); otherwise OB_ERR_SHAPE with nothing launched (run
 * ob_bitlinear_fwd_residual and ob_layernorm_fwd[_pair]). X, R, Y, ln_y*, ln_w*, ln_b* 16-byte
 * aligned; rows of all outputs [P*M][N]. */
OB_API int ob_bitlinear_fwd_residual_ln(
    const float* X, int64_t P, int64_t M, int64_t K, const uint32_t* codes2,
    const uint32_t* codes1, const int32_t* pass_bits, const float* alpha, int alpha_raw,
    const float* bias, int64_t N, const float* R, float rscale, float p_drop, const uint64_t* rng,
    int64_t rng_offset, const int32_t* lens, int64_t T, float* Y, int nln, const float* ln_w0,
    const float* ln_b0, float eps0, float* ln_y0, float* ln_mean0, float* ln_rstd0,
    const float* ln_w1, const float* ln_b1, float eps1, float* ln_y1, float* ln_mean1,
    float* ln_rstd1, void* stream);
OB_API int ob_bitlinear_bwd_dx_swish_drop(const float* dY, int64_t P, int64_t M, int64_t N,
                                          const uint32_t* codes2_t, const uint32_t* codes1_t,
                                          const int32_t* pass_bits, const float* alpha,
                                          int alpha_raw, int64_t K, const float* pre,
                                          float p_drop, const uint64_t* rng, int64_t rng_offset,
                                          float* dPre, void* stream);
OB_API int ob_drop_scale_bwd(const float* dOut, int64_t rows, int64_t N, float rscale,
                             float p_drop, const uint64_t* rng, int64_t rng_offset,
                             const int32_t* lens, int64_t T, float* dY, void* stream);

/* out = R + rscale * rowvalid * dropout(Y) over [rows][N]: the residual/dropout tail of a
 * call site whose producer is not a BitLinear GEMM (the conv module's pw2, conformer.py:
 * 160-167), with the mask convention of the fused entries above. */
OB_API int ob_residual_drop_fwd(const float* R, const float* Y, int64_t rows, int64_t N,
                                float rscale, float p_drop, const uint64_t* rng,
                                int64_t rng_offset, const int32_t* lens, int64_t T, float* out,
                                void* stream);

/* Conv2dSubsampling's conv -> +bias -> ReLU tails (conformer.py:183-186), NCHW planes of
 * hw = H*W elements: fwd y = max(y + b[c], 0) in place; bwd g' = g * (y > 0) (torch's
 * threshold_backward on the ReLU output) and db[c] = sum over (b, h, w) of g'. */
OB_API int ob_bias_relu_fwd(float* y, const float* bias, int64_t B, int64_t C, int64_t hw,
                            void* stream);
OB_API size_t ob_relu_bias_bwd_workspace(int64_t B, int64_t C);
OB_API int ob_relu_bias_bwd(const float* g, const float* y, int64_t B, int64_t C, int64_t hw,
                            float* gout, float* dbias, void* ws, size_t ws_bytes, void* stream);
/* out[n] = sum over rows of x[rows][N], fixed order: the bias gradient of a GEMM on rows
 * (the conv module's pointwise convolutions, conformer.py:143,147). */
OB_API size_t ob_colsum_workspace(int64_t N);
OB_API int ob_colsum(const float* x, int64_t rows, int64_t N, float* out, void* ws,
                     size_t ws_bytes, void* stream);

/* ------------------------------------------------------------------------------------
 * Dense fp32 GEMMs of the conv module's pointwise Conv1d(kernel 1) layers
 * (conformer.py:143,147; replaces the fp32 matmuls / addmm of a 1x1 conv on channels-last
 * rows). Exact-fp32 products on the bf16 matrix cores (6 MFMAs per k-step, csrc/dgemm.hip).
 *   ob_dense_gemm: w_trans = 0: Y[M][N] = X[M][K] . W^T + bias, W [N][K] (the forward);
 *                  w_trans = 1: Y[M][N] = X[M][K] . W,          W [K][N] (dX = dY . W).
 *                  bias may be NULL. X, W, Y 16-byte aligned; K, N multiples of 4.
 *                  A K too long for the whole-K weight image (N <= 144) runs the K-chunked
 *                  form (round 6): the CTC head's input gradient, K = V = 5004, replacing the
 *                  library fp32 `g @ W` of the head's backward (losses.py:41-47 through
 *                  conformer.py:275).
 *   ob_dense_dw:   dW[N][K] = dY[M][N]^T . X[M][K], db[N] = column sums of dY (db may be
 *                  NULL); N, K multiples of 48. Deterministic (fixed-order chunk sums).
 * ob_dense_supported(K, N) / ob_dense_dw_workspace(M, N, K) == 0: the shape is not taken.
 * ------------------------------------------------------------------------------------ */
/* The property the int8 inference path's absmax launch relies on (round 6: max|silu| over a
 * lane's elements taken as silu(max y), csrc/tgemm_i8.hip): adds to *bad (a device uint32 the
 * caller zeroes) the count of fp32 bit patterns b in [lo_bits, hi_bits) with
 * fast_silu(float(b + 1)) < fast_silu(float(b)). Non-negative finite patterns only. */
OB_API int ob_silu_fast_monotone_check(uint32_t lo_bits, uint32_t hi_bits, uint32_t* bad,
                                       void* stream);
OB_API int ob_dense_supported(int64_t K, int64_t N);
OB_API int ob_dense_gemm(const float* X, int64_t M, int64_t K, const float* W, int w_trans,
                         const float* bias, int64_t N, float* Y, void* stream);
/* ob_dense_gemm (w_trans 0) with the residual tail of the conv module (conformer.py:160-167,
 * x + dropout(pw2(.))) in the epilogue: Y = R + dropout(X W^T + bias), R [M][N]; the dropout
 * is ob_residual_drop_fwd's (hash on the flat index row * N + col with rng / rng_offset, rscale
 * 1, no row mask), so Y equals ob_dense_gemm followed by ob_residual_drop_fwd bit for bit. */
OB_API int ob_dense_gemm_residual_drop(const float* X, int64_t M, int64_t K, const float* W,
                                       const float* bias, int64_t N, const float* R,
                                       float p_drop, const int64_t* rng, int64_t rng_offset,
                                       float* Y, void* stream);
OB_API size_t ob_dense_dw_workspace(int64_t M, int64_t N, int64_t K);
OB_API int ob_dense_dw(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                       float* dW, float* db, void* ws, size_t ws_bytes, void* stream);
/* ob_dense_dw with the finish deferred to ob_dw_finish_table (same table and contract as
 * ob_bitlinear_bwd_dw_passes_defer; dense weights carry no STE mask / alpha). */
OB_API int ob_dense_dw_defer(const float* dY, const float* X, int64_t M, int64_t N, int64_t K,
                             float* dW, float* db, void* ws, size_t ws_bytes, void* table,
                             int64_t slot, int64_t start, int64_t* n_blocks, void* stream);

/* ------------------------------------------------------------------------------------
 * Conv module core (ConvModule, conformer.py:139-167; full precision), channels-last.
 * Rows = Bt*T frames (utterance b = rows [b*T, (b+1)*T)), channel fastest; P stacked
 * passes (Bt = P*B) keep per-pass BatchNorm statistics. pw1 / pw2 are plain GEMMs left to
 * the caller; between them:
 *   fwd: u [rows][2C] -> g = u[:, :C] * sigmoid(u[:, C:])      (GLU over channels, :156)
 *        z = depthwise_K(g) + b_dw   (zero padding K/2 at utterance edges, :157)
 *        stats[p][c] = {mean, rstd} of z over pass p's B*T frames (batch statistics,
 *        padded frames included, biased variance, eps; :158)
 *        v = swish(gamma * (z - mean) * rstd + beta)               (:159)
 *        g [rows][C] (the GLU output) is kept for the backward.
 *   bwd: from dv = dL/dv: du [rows][2C], dw_dw [C][K], db_dw [C], dgamma [C], dbeta [C]
 *        (weight gradients summed over passes). u, z, g, stats are the forward's.
 * K odd; ob_convmod_workspace() == 0 means the shape is not supported (C too wide for the
 * LDS tile, or, where the channel-split tiles run (K = 31, C % 16 == 0), an utterance whose
 * [T + 7][2C] floats pass 2^31 bytes: the tiles use 32-bit byte offsets; such shapes return
 * OB_ERR_SHAPE). Deterministic (fixed-order reductions, fp64 statistics).
 * No frames (Bt * T == 0): the forward writes nothing; the backward (and _defer, with
 * *deferred = 0) writes exact zeros to dw_dw, db_dw, dgamma, dbeta and touches nothing else;
 * both return OB_OK. One frame per pass (Bt / P * T == 1): BatchNorm's output is beta and
 * no gradient passes through it; the backward writes exact zeros to du, dw_dw, db_dw
 * (dgamma is an exact 0 by its arithmetic), dbeta as usual, and never defers.
 * ------------------------------------------------------------------------------------ */
OB_API size_t ob_convmod_workspace(int64_t P, int64_t Bt, int64_t T, int64_t C, int64_t K);
OB_API int ob_convmod_fwd(const float* u, const float* w_dw, const float* b_dw,
                          const float* gamma, const float* beta, int64_t P, int64_t Bt,
                          int64_t T, int64_t C, int64_t K, float eps, float* z, float* g,
                          float* stats, float* v, void* ws, size_t ws_bytes, void* stream);
OB_API int ob_convmod_bwd(const float* dv, const float* u, const float* z, const float* g,
                          const float* stats, const float* w_dw, const float* gamma,
                          const float* beta, int64_t P, int64_t Bt, int64_t T, int64_t C,
                          int64_t K, float* du, float* dw_dw, float* db_dw, float* dgamma,
                          float* dbeta, void* ws, size_t ws_bytes, void* stream);
/* ob_convmod_bwd with the depthwise weight-gradient finish (dw_dw, db_dw: the fixed-order
 * sum of the per-tile partials) deferred when table != NULL and the shape runs on the
 * channel-split tiles: the backward launch writes the partials' descriptor into slot `slot`
 * of a caller-owned device table of ob_cm_wgrad_entry_bytes() entries, *deferred = 1, and
 * ob_cm_wgrad_table finishes entries 0 .. n-1 in one launch (nmax = the largest C * (K + 1))
 * with the same arithmetic. ws stays allocated until then. *deferred = 0: finished now. */
OB_API int ob_convmod_bwd_defer(const float* dv, const float* u, const float* z, const float* g,
                                const float* stats, const float* w_dw, const float* gamma,
                                const float* beta, int64_t P, int64_t Bt, int64_t T, int64_t C,
                                int64_t K, float* du, float* dw_dw, float* db_dw, float* dgamma,
                                float* dbeta, void* ws, size_t ws_bytes, void* table, int64_t slot,
                                int64_t* deferred, void* stream);
OB_API size_t ob_cm_wgrad_entry_bytes(void);
OB_API int ob_cm_wgrad_table(const void* table, int64_t n, int64_t nmax, void* stream);

/* ------------------------------------------------------------------------------------
 * Conv2dSubsampling's two convolutions (conformer.py:170-208: Conv2d(1, C, 3, 2) -> ReLU ->
 * Conv2d(C, C, 3, 2) -> ReLU; replaces the torch.nn.Conv2d / cuDNN calls the module makes),
 * channels-last so the flatten + Linear that follows needs no transpose:
 *   X  [B][T][F] feats;  W0 [C][1][3][3], b0 [C];  W2 [C][C][3][3], b2 [C] (torch layouts)
 *   Y1 [B][T1][F1][C] = relu(conv(X, W0) + b0),  T1 = (T-3)/2+1, F1 = (F-3)/2+1
 *   Y2 [B][T2][F2][C] = relu(conv(Y1, W2) + b2), T2 = (T1-3)/2+1, F2 = (F1-3)/2+1
 * ob_subsample_pack re-splits W2 into the bf16 hi/mid/lo images the fp32-exact MFMA
 * GEMMs read (call it whenever W2 changes; ob_subsample_image_bytes(C) bytes, 16-aligned).
 * bwd: from dY2 = dL/dY2 (before the ReLU mask) and the forward's X, W0, b0, Y1, Y2: dW0,
 * db0, dW2, db2 (overwritten; dX is not produced: the feats need no gradient). Deterministic; C in {48, 64, 96, 144},
 * T, F >= 7; ob_subsample_bwd_workspace() == 0 means unsupported.
 * ------------------------------------------------------------------------------------ */
OB_API size_t ob_subsample_image_bytes(int64_t C);
OB_API int ob_subsample_pack(const float* W2, int64_t C, void* img, void* stream);
OB_API int ob_subsample_fwd(const float* X, int64_t B, int64_t T, int64_t F, int64_t C,
                            const float* W0, const float* b0, const void* img,
                            const float* b2, float* Y1, float* Y2, void* stream);
OB_API size_t ob_subsample_bwd_workspace(int64_t B, int64_t T, int64_t F, int64_t C);
OB_API int ob_subsample_bwd(const float* X, const float* W0, const float* b0, const float* Y1,
                            const float* Y2, const float* dY2, int64_t B, int64_t T, int64_t F,
                            int64_t C, const void* img,
                            float* dW0, float* db0, float* dW2, float* db2, void* ws,
                            size_t ws_bytes, void* stream);

#ifdef __cplusplus
}
#endif

#endif /* ONEBIT_HIP_H_ */
