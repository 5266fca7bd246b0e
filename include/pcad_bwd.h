/* pcad_bwd.h - C ABI of libpcad_bwd.so: the backward operators of a Caduceus block beyond the selective scan, and of the masked-LM
 * loss head (training support).
 *
 * A third library beside libpcad.so (include/pcad.h: the inference ABI) and libpcad_train.so (include/pcad_train.h: the selective
 * scan's backward), whose exported symbol sets stay as they are.  This one is OPEN: a later backward operator is added here - its
 * declaration below, its entry in plantcaduceus_amd.engine.BWD_SIGNATURES, its kernel in the library - rather than in yet another
 * library; what is held is that this header, that table and the library's exports name the same pcad_* symbols.
 * libpcad_bwd.so links libpcad.so (same directory) and shares its conventions: status codes (pcad_status), dtypes (pcad_dtype),
 * pcad_stream, and the calling thread's pcad_last_error() text.  Built by the same Makefile from csrc/bwd_api.hip, csrc/conv_bwd.hip,
 * csrc/norm_bwd.hip and csrc/loss_bwd.hip.
 *
 * Common to every entry: no allocation, no synchronisation, all work goes on `stream`; the scratch is the caller's, *_scratch_bytes
 * large and 256-byte aligned (too small / misaligned: PCAD_ERR_WORKSPACE); PCAD_ERR_INVALID names the offending argument through
 * pcad_last_error(); every output is overwritten, never accumulated; no floating-point atomics - every sum has a fixed order, so two
 * calls give the same bits; all in-tensor offsets are 64-bit; rows outside a strand are never read or written. */
#ifndef PCAD_BWD_H
#define PCAD_BWD_H
#include "pcad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of pcad_causal_conv1d_silu_dir on plain rows: conv1d (width 4) + bias + SiLU, one direction.  Replaces: the backward of
 * `causal_conv1d_fn(x, weight, bias, activation="silu")` (causal-conv1d 1.4.0).  Per strand and channel, rows outside [0, L)
 * contributing zero, g = dL/dout:
 *   causal (reverse 0):      a_t = b + sum_k w[k] x[t-3+k]     dx_t = sum_k w[k] da_{t+3-k}     dw[k] = sum_{s,t} da_t x[t-3+k]
 *   anti-causal (reverse 1): a_t = b + sum_k w[k] x[t+3-k]     dx_t = sum_k w[k] da_{t-3+k}     dw[k] = sum_{s,t} da_t x[t+3-k]
 *   da_t = g_t sig(a_t) (1 + a_t (1 - sig(a_t)))               db = sum_{s,t} da_t
 * a_t is recomputed from x in fp32 in the forward's accumulation order (the forward saves nothing).  All products and sums are fp32;
 * the only rounding is the store of dx in the model dtype.
 *   x          [S, L, ldx >= E] dtype (ldx = 2 E: the first half of a token-major xz);  dout, dx [S, L, E] dtype
 *   w, dw      fp32 [E, 4];  b, db fp32 [E]
 *   x, dout, dx, w 16-byte aligned;  E and ldx multiples of 16 bytes of the dtype (8 bf16 / 4 fp32 elements)
 *   scratch    pcad_causal_conv1d_silu_bwd_scratch_bytes(S, L, E) bytes: the dw | db partials of every (strand, segment of 64 steps),
 *              which a second kernel adds in a fixed order
 * S == 0 or L == 0: OK, nothing is done. */
size_t pcad_causal_conv1d_silu_bwd_scratch_bytes(int S, int L, int E);
int pcad_causal_conv1d_silu_bwd(const void* x, int64_t ldx, const float* w, const float* b, const void* dout,
                                void* dx, float* dw, float* db, void* scratch, size_t scratch_bytes,
                                int S, int L, int E, int reverse, int dtype, pcad_stream stream);

/* Backward of pcad_add_rmsnorm.  Replaces: the backward of `rms_norm_fn` (mamba_ssm.ops.triton.layer_norm) for the forms Caduceus
 * uses: no bias, with or without a residual, with or without prenorm.  Per row, everything in fp32:
 *   r = x + residual_in  (unrounded, as the forward forms it; residual_in NULL: x)     rstd = rsqrt(mean(r^2) + eps)     rh = r rstd
 *   dr_i = dresidual_out_i + rstd (w_i dy_i - rh_i (1/D) sum_j w_j dy_j rh_j)           (dresidual_out NULL: 0)
 *   dx = round(dr) in dtype     dresidual_in = round(dr) in res_dtype     dweight_i = sum_rows dy_i rh_i
 * The only roundings are the two stores.
 *   x, dy, dx  [rows, D] dtype;  weight, dweight fp32 [D];  D % 8 == 0, D <= 2048 (as the forward)
 *   residual_in    [rows, D] res_dtype or NULL (the forward's);  dresidual_in [rows, D] res_dtype, required exactly when residual_in is given
 *   dresidual_out  [rows, D] res_dtype or NULL (the caller did not use the prenorm output)
 *   dtype / res_dtype: BF16 / F32, BF16 / BF16 or F32 / F32, as the forward
 *   scratch    pcad_add_rmsnorm_bwd_scratch_bytes(rows, D) bytes: one dweight partial row per slab of 16 rows, which a second kernel
 *              adds in a fixed order
 * rows == 0: OK, nothing is done. */
size_t pcad_add_rmsnorm_bwd_scratch_bytes(int64_t rows, int D);
int pcad_add_rmsnorm_bwd(const void* x, const void* residual_in, const float* weight, const void* dy, const void* dresidual_out,
                         void* dx, void* dresidual_in, float* dweight, void* scratch, size_t scratch_bytes,
                         int64_t rows, int D, float eps, int dtype, int res_dtype, pcad_stream stream);

/* Backward of pcad_loss_head on plain rows (no fragment layout of res): norm_f -> RC re-assembly -> tied RCPS LM head -> weighted
 * cross entropy.  Replaces: the backward of rms_norm_fn + the flips / cats + RCPSLMHead + F.cross_entropy, and never forms norm_f's
 * output or its gradient for the rows that carry no label.  A position (b, t) is labelled exactly as pcad_loss_head decides it:
 * labels equal to ignore_index or negative are ignored, any other label outside [0, 8) contributes nothing (there is no status
 * word here).  Per labelled position, with the rows rf = (b, t) and rr = (B + b, L-1-t), everything in fp32:
 *   v = h + res     rstd = rsqrt(mean(v^2) + eps)     vh = v rstd     o = round(vh w) in dtype              (per row, as the forward)
 *   lg[k] = the forward's logits of (b, t), recomputed bit for bit     p = softmax(lg) over all 8
 *   dlg[k] = (dsum[b] wt + dnll[b, t]) (p[k] - [k == label])           wt = loss_weights[b, t] or 1;  dnll NULL: 0
 *   do_i = sum_k dlg[k] Emb[k][i] (row rf)     do_i = sum_k dlg[k] Emb[complement[k]][i] (row rr)
 *   dv_i = rstd (w_i do_i - vh_i (1/D) sum_j w_j do_j vh_j)            dh = round(dv) in dtype     dres = round(dv) in res_dtype
 *   demb[k] += dlg[k] o (row rf)     demb[complement[k]] += dlg[k] o (row rr)     dnorm_weight_i += do_i vh_i
 * The forward's roundings (o, the strands' partial logits, their sum) are the identity in the derivative; the only new roundings are
 * the stores of dh and dres.  Rows of dh / dres at unlabelled positions are written as zeros.
 *   h, dh      [2B * L, D] dtype;  res, dres [2B * L, D] res_dtype (BF16 / F32, BF16 / BF16 or F32 / F32);  D % 8 == 0, D <= 2048
 *   norm_weight, dnorm_weight fp32 [D];  emb_f32, demb fp32 [8, D];  complement int32 [8];  labels int32 [B, L]
 *   loss_weights fp32 [B, L] or NULL;  dsum fp32 [B]: the gradient of sums_out[b, 0];  dnll fp32 [B, L] or NULL: the gradient of nll_out
 *   dh, dres, dnorm_weight, demb may each be NULL (not computed), not all of them;  h, res, norm_weight, emb_f32, dh, dres 16-byte aligned
 *   scratch    pcad_loss_head_bwd_scratch_bytes(B, L, D) bytes: one row of 9 D partials (demb | dnorm_weight) per (window, segment
 *              of 64 positions), which a second kernel adds in a fixed order, and one spare row
 * B == 0 or L == 0: OK, nothing is done. */
size_t pcad_loss_head_bwd_scratch_bytes(int B, int L, int D);
int pcad_loss_head_bwd(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                       const int32_t* labels, const float* loss_weights, int ignore_index, const float* dsum, const float* dnll,
                       void* dh, void* dres, float* dnorm_weight, float* demb, void* scratch, size_t scratch_bytes,
                       int B, int L, int D, float eps, int dtype, int res_dtype, pcad_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PCAD_BWD_H */
