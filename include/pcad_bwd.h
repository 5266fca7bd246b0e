/* pcad_bwd.h - C ABI of libpcad_bwd.so: the backward operators of a Caduceus block beyond the selective scan, and of the masked-LM
 * loss head and of the pooled sequence-classification head, and the dropout-masked LoRA down-projection (training support).
 *
 * A third library beside libpcad.so (include/pcad.h: the inference ABI) and libpcad_train.so (include/pcad_train.h: the selective
 * scan's backward), whose exported symbol sets stay as they are.  This one is OPEN: a later backward operator is added here - its
 * declaration below, its entry in plantcaduceus_amd.engine.BWD_SIGNATURES, its kernel in the library - rather than in yet another
 * library; what is held is that this header, that table and the library's exports name the same pcad_* symbols.
 * libpcad_bwd.so links libpcad.so (same directory) and shares its conventions: status codes (pcad_status), dtypes (pcad_dtype),
 * pcad_stream, and the calling thread's pcad_last_error() text.  Built by the same Makefile from csrc/bwd_api.hip, csrc/conv_bwd.hip,
 * csrc/norm_bwd.hip, csrc/loss_bwd.hip, csrc/pool_bwd.hip, csrc/optim.hip (the optimizer step that uses the gradients and their gathering
 * into one buffer for a data-parallel run), csrc/wgrad.hip (the weight gradient of a linear layer into an fp32 main gradient) and
 * csrc/lora.hip (the dropout-masked down-projection of a LoRA branch, forward and backward) and csrc/scan_bwd_seg.hip (the selective
 * scan's backward in segments) and csrc/scan_fwd_seg.hip (the scan's training forward in segments: the last two sections below) and
 * csrc/pool_feat.hip (the score head on cached pooled vectors).
 *
 * Common to every entry: no allocation, no synchronisation, all work goes on `stream`; the scratch is the caller's, *_scratch_bytes
 * large and 256-byte aligned (too small / misaligned: PCAD_ERR_WORKSPACE); PCAD_ERR_INVALID names the offending argument through
 * pcad_last_error(); every output is overwritten, never accumulated (the two stated exceptions: pcad_linear_wgrad with accumulate != 0, and pcad_lora_down_bwd, which updates dx in place); no floating-point atomics - every sum has a fixed order, so two
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

/* Backward of pcad_pooled_head on plain rows (no fragment layout of res): norm_f -> per-strand pooling -> score -> (fwd + rc) / 2, the
 * head of CaduceusForSequenceClassification.  Replaces: the backward of rms_norm_fn + the stack / flip of the two strands + the pooling
 * + the score Linear + the strand average, and never forms norm_f's output or its gradient as a tensor.  The forward it differentiates
 * (DESIGN.md section 4f), per row:  v = h + res   rstd = rsqrt(mean(v^2) + eps)   vh = v rstd   o = round(vh w) in dtype;
 * pooled[b, s] = the mean over the strand's own rows (fp32 sum / L, rounded once), or row 0, or row L-1 - the forward strand's rows are
 * b L + p, the rc strand's (B + b) L + p, no flip;  logits[b, n] = round(round(round(pooled[b, 0] . W[n]) + round(pooled[b, 1] . W[n])) / 2).
 * Every rounding of the forward is the identity in the derivative.  Everything in fp32:
 *   dpooled[b, s, :] = 1/2 sum_n dlogits[b, n] W[n, :]                                    (n in index order; the same for both strands)
 *   dscore_w[n, :]   = 1/2 sum_b dlogits[b, n] (pooled[b, 0, :] + pooled[b, 1, :])        (b in index order)
 *   do(row)          = dpooled[b, s] / L   mean: every row of the strand;   first: row 0 only;   last: row L-1 only;   other rows: 0
 *   dv_i = rstd (w_i do_i - vh_i (1/D) sum_j w_j do_j vh_j)            dh = round(dv) in dtype     dres = round(dv) in res_dtype
 *   dnorm_weight_i = sum_rows do_i vh_i
 * The only new roundings are the stores of dh and dres.  With first / last the rows that carry no gradient are written as zeros.
 * PCAD_POOL_MAX is refused (PCAD_ERR_INVALID naming `pooling`): the gradient of a maximum needs a tie rule among rows that are equal
 * after rounding to the model dtype, and nothing in the reference pins one.  Inference keeps max pooling.
 *   h, dh      [2B * L, D] dtype;  res, dres [2B * L, D] res_dtype (BF16 / F32, BF16 / BF16 or F32 / F32);  D % 8 == 0, D <= 2048
 *   norm_weight, dnorm_weight fp32 [D];  score_w, dscore_w fp32 [num_labels, D] (score_w: the dtype-rounded weight, as the forward takes it);
 *   1 <= num_labels <= PCAD_MAX_LABELS;  pooled fp32 [B, 2, D]: the forward's pooled_out;  dlogits fp32 [B, num_labels]
 *   dh, dres, dnorm_weight, dscore_w may each be NULL (not computed), not all of them;  h, res, norm_weight, dh, dres 16-byte aligned
 *   scratch    pcad_pooled_head_bwd_scratch_bytes(B, L, D, pooling) bytes: the windows' do rows [B, D] (formed once per window by a first
 *              launch, not per row), then one row of D partials of dnorm_weight per (window, strand, segment of 64 rows) - first / last:
 *              per (window, strand) - which a second kernel adds in a fixed order; each part rounded up to 256 bytes.  0 for a pooling
 *              this entry refuses.
 * B == 0: OK, nothing is done.  L == 0 with B > 0: PCAD_ERR_INVALID. */
size_t pcad_pooled_head_bwd_scratch_bytes(int B, int L, int D, int pooling);
int pcad_pooled_head_bwd(const void* h, const void* res, const float* norm_weight, const float* score_w, const float* pooled,
                         const float* dlogits, void* dh, void* dres, float* dnorm_weight, float* dscore_w, void* scratch, size_t scratch_bytes,
                         int B, int L, int D, int num_labels, float eps, int pooling, int dtype, int res_dtype, pcad_stream stream);

/* ---- The score head on cached pooled vectors: frozen-trunk fine-tuning --------------------------------------------
 * With a frozen trunk a window's pooled vectors - pcad_pooled_head's / pcad_forward_pooled's pooled_out [2, D] - never change, so they
 * are computed once and kept; these two entries are what is left of the head.  csrc/pool_feat.hip.  No scratch.
 *
 * pcad_pooled_logits: logits[b, n] = round(round(round(pooled[b, 0] . W[n]) + round(pooled[b, 1] . W[n])) / 2), the roundings to `dtype`
 * (the model dtype), fp32 accumulation.  It restates the logits half of pcad_pooled_head's second stage - one block of 256 lanes per
 * window, wave w of 4 takes labels w, w + 4, ..., lane l adds the products of columns l, l + 64, ... in index order, the 64 lanes' sums
 * are added by the xor butterfly (32, 16, ... 1) - so that the logits of cached vectors are the bits pcad_forward_pooled writes.
 *   pooled fp32 [B, 2, D];  score_w fp32 [num_labels, D] (the dtype-rounded weight);  logits fp32 [B, num_labels]
 *   D % 8 == 0, D <= 2048;  1 <= num_labels <= PCAD_MAX_LABELS;  dtype PCAD_BF16 / PCAD_F32;  pooled, score_w 16-byte aligned
 * B == 0: OK, nothing is done (pooled and logits may then be NULL). */
int pcad_pooled_logits(const float* pooled, const float* score_w, float* logits, int B, int D, int num_labels, int dtype,
                       pcad_stream stream);

/* The backward of pcad_pooled_logits.  Every rounding of the forward is the identity in the derivative, so there is no dtype; all fp32:
 *   dscore_w[n, :]   = 1/2 sum_b dlogits[b, n] (pooled[b, 0, :] + pooled[b, 1, :])        (b in index order)
 *   dpooled[b, s, :] = 1/2 sum_n dlogits[b, n] W[n, :]                                    (n in index order; the same for both strands)
 * dscore_w is formed operation for operation as pcad_pooled_head_bwd forms it: the same bits.  dpooled has no 1 / L: the pooling is
 * upstream of `pooled`.
 *   pooled, score_w as above;  dlogits fp32 [B, num_labels];  dscore_w fp32 [num_labels, D] or NULL;  dpooled fp32 [B, 2, D] or NULL
 *   dscore_w and dpooled may each be NULL (not computed), not both; neither changes the other's bits
 *   pooled, score_w, dscore_w, dpooled 16-byte aligned;  D and num_labels as above
 * B == 0: OK, nothing is done - dscore_w is NOT written (pooled and dlogits may then be NULL). */
int pcad_pooled_logits_bwd(const float* pooled, const float* score_w, const float* dlogits, float* dscore_w, float* dpooled,
                           int B, int D, int num_labels, pcad_stream stream);

/* ---- The optimizer step: AdamW with global-norm gradient clipping over a whole parameter set ----------------
 * Replaces: torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step + zero_grad, in three (one) launches however many tensors there are.
 *
 * The caller describes the set once: a table of pcad_optim_tensor records, and beside it a chunk map.  The work is cut into chunks of
 * PCAD_OPTIM_CHUNK elements that never straddle two tensors: tensor i has ceil(n_i / PCAD_OPTIM_CHUNK) chunks, in table order.  The
 * chunking is a function of the table alone - not of the grid, not of the device - and one block works on one chunk, which is what
 * makes the step bit-reproducible.  pcad_optim_plan checks a table in HOST memory and fills the map; the caller uploads both, and the
 * step entries read only the device copies (which they cannot check: a device table that pcad_optim_plan has not accepted, or a map
 * that is not its own, is undefined behaviour). */
#define PCAD_OPTIM_CHUNK 4096          /* elements per chunk */
#define PCAD_OPTIM_DECAY 1             /* flags bit 0: weight decay applies to this tensor */
#define PCAD_OPTIM_MAX_CHUNKS 16777215  /* 2^24 - 1: one 256-lane block per chunk, the grid below 2^32 lanes (6.8e10 elements) */

typedef struct pcad_optim_tensor {     /* 64 bytes; every pointer is device memory, 16-byte aligned */
    void* param;                       /* [n] param_dtype (PCAD_BF16 / PCAD_F32) */
    void* grad;                        /* [n] grad_dtype (PCAD_BF16 / PCAD_F32) */
    float* master;                     /* [n] fp32, or NULL: an fp32 param is its own master (a bf16 param needs one) */
    float* exp_avg;                    /* [n] fp32 */
    float* exp_avg_sq;                 /* [n] fp32 */
    int64_t n;                         /* >= 0; 0: the record has no chunk and its pointers are not read */
    int32_t param_dtype, grad_dtype;
    int32_t flags;                     /* PCAD_OPTIM_DECAY or 0 */
    int32_t reserved;                  /* 0 */
} pcad_optim_tensor;

typedef struct pcad_optim_state {      /* 16 bytes of device memory, 16-byte aligned, the caller's; zeroed once, then only the step writes it */
    float norm;                        /* the last step's total norm of grad_scale * grad */
    float coef;                        /* the factor the last step applied to every gradient */
    int32_t finite;                    /* 1: norm was finite and the step was applied; 0: it was skipped */
    int32_t skipped;                   /* steps skipped so far */
} pcad_optim_state;

/* Checks `table` (HOST memory, count records) and counts its chunks into *chunks_out.  chunk_map (HOST, may be NULL: count only) gets
 * two int32 per chunk, (record index, chunk index within the record), chunk_capacity chunks of room (less than needed: PCAD_ERR_INVALID).
 * PCAD_ERR_INVALID, naming the record and the field: n < 0; a dtype other than PCAD_BF16 / PCAD_F32; unknown flag bits; for n > 0 a
 * NULL param, grad, exp_avg or exp_avg_sq, a bf16 param without master, any of the five pointers not 16-byte aligned; more than
 * PCAD_OPTIM_MAX_CHUNKS chunks in all.  Pointers are compared, never dereferenced. */
int pcad_optim_plan(const pcad_optim_tensor* table, int64_t count, int32_t* chunk_map, int64_t chunk_capacity, int64_t* chunks_out);

/* One step.  table / chunk_map: the DEVICE copies of what pcad_optim_plan accepted / filled; chunks: its count.  Three launches:
 *   1. part[c] = sum over chunk c of (grad_scale g)^2     a lane adds its elements in index order, the 64 lanes of a wave by the xor
 *                                                          butterfly, the 4 waves of the block in index order
 *   2. one block adds part[] (lane t of 1024: t, t + 1024, ... in index order, then the same tree) and writes `state`:
 *        norm = sqrt(sum)     finite = norm is neither inf nor NaN     skipped += !finite
 *        coef = grad_scale * min(1, max_norm / (norm + 1e-6))          (torch.nn.utils.clip_grad_norm_; max_norm <= 0: coef = grad_scale)
 *   3. per element, everything in fp32, only when finite (else nothing at all is stored):
 *        g = coef grad     p = master (param without one)     p = p (1 - lr wd) when PCAD_OPTIM_DECAY
 *        m = b1 m + (1 - b1) g     v = b2 v + (1 - b2) g^2     p -= (lr / bc1) m / (sqrt(v) / sqrt(bc2) + eps)
 *        store master (param without one), m, v; a bf16 param = round-to-nearest-even(master), an fp32 param beside a master = master
 * The host passes lr, bc1 = 1 - b1^t and bc2 = 1 - b2^t (t = the 1-based step) in double; 1 - lr wd, lr / bc1, sqrt(bc2), 1 - b1 and
 * 1 - b2 are formed in double and rounded to fp32 once.  The host never sees the norm unless it reads `state`.
 * A tensor's last n % 4 (both fp32) / n % 8 (a bf16 side) elements are walked one by one: nothing past n is read or written.
 *   scratch    pcad_adamw_step_scratch_bytes(chunks) bytes: part[]
 * PCAD_ERR_INVALID: count or chunks < 0, chunks > PCAD_OPTIM_MAX_CHUNKS, NULL or misaligned table / chunk_map (chunks > 0) / state, bc1 or bc2 not
 * in (0, 1], a non-finite scalar.  chunks == 0: phase 2 alone runs (norm 0). */
size_t pcad_adamw_step_scratch_bytes(int64_t chunks);
int pcad_adamw_step(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, void* state, void* scratch, size_t scratch_bytes,
                    double lr, double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2, double max_norm,
                    double grad_scale, pcad_stream stream);

/* Sets every gradient of the table to zero (all n elements, nothing beyond them) in one launch. */
int pcad_zero_grads(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, pcad_stream stream);

/* ---- Every gradient in one fp32 buffer, for one collective over the ranks of a data-parallel run -------------
 * pcad_grads_flat_plan lays the table's gradients out back to back, each slice padded to a multiple of 4 elements so that it starts
 * 16-byte aligned (what the table asks of a `grad` pointer: the step then runs on a second table whose grads are the slices):
 *   offsets_out[i] = sum_{j < i} round_up_4(n_j)  (elements)      *total_out = sum_j round_up_4(n_j)
 * table: HOST memory, count records; offsets_out: HOST, count int64.  It makes pcad_optim_plan's checks (and refuses what it refuses,
 * the 2^24 - 1 chunks included), dereferences no pointer of a record and needs no device. */
int pcad_grads_flat_plan(const pcad_optim_tensor* table, int64_t count, int64_t* offsets_out, int64_t* total_out);

/* One launch over the step's own chunk map (one 256-lane block per chunk): flat[offsets[t] + i] = (float)grad_t[i] for every i < n_t.
 * bf16 -> fp32 is exact, so the buffer holds the gradients' values; a sum over ranks is then formed in fp32.  16-byte accesses, a full
 * chunk's loads issued before its stores; a tensor's last n % 4 (fp32 gradients) / n % 8 (bf16) elements are walked one by one by the
 * lane that owns them: nothing past n is read, the up to 3 padding elements of a slice are never written (the caller zeroes the buffer
 * once) and the gradients are not modified.
 *   table, chunk_map, count, chunks: as pcad_adamw_step;  offsets: the DEVICE copy of pcad_grads_flat_plan's, 8-byte aligned
 *   flat: fp32 [flat_elems >= total], 16-byte aligned.  A chunk whose slice would not lie within [0, flat_elems) or is not 4-aligned
 *   - offsets that are not this table's - is not written.
 * PCAD_ERR_INVALID: the table arguments as pcad_adamw_step, flat_elems < 0, NULL or misaligned offsets / flat (chunks > 0).
 * chunks == 0: OK, nothing is done. */
int pcad_grads_gather(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, const int64_t* offsets, float* flat,
                      int64_t flat_elems, pcad_stream stream);

/* ---- fp32 main gradients: the weight gradient of a linear layer, accumulated in place ----------------------------
 * Replaces: the `dy.t() @ x` of F.linear's backward, which can only return the gradient in the parameter's dtype.
 *   dw[n, k] = (accumulate ? dw[n, k] : 0) + s[n, k]        s[n, k] = sum_m dy[m, n] x[m, k]
 * This entry is the one stated exception to "every output is overwritten, never accumulated": with accumulate != 0 it ADDS to dw.
 * Each bf16 x bf16 product is exact in fp32; the sum is fp32 in a fixed order; s is formed completely and then added to the old value
 * once - every element of dw sees one read (accumulate only) and one write.  The header's other rules hold: no allocation, no
 * synchronisation, the caller's stream and scratch, no floating-point atomics, 64-bit offsets (M N may pass 2^31).
 *   dy     bf16 [M, N], row stride lddy elements;  x bf16 [M, K], row stride ldx;  dw fp32 [N, K], row stride lddw
 *   N % 8 == 0, K % 8 == 0, 8 <= N, K <= 8192;  lddy % 8 == 0, ldx % 8 == 0, lddw % 4 == 0;  lddy >= N, ldx >= K, lddw >= K;  M >= 0
 *   dy, x, dw non-NULL (dy and x may be NULL when M == 0) and 16-byte aligned.  Anything else: PCAD_ERR_INVALID naming the argument, decided without a device.
 * The rows are cut into slabs that depend on (M, N, K) alone - never on the device - so the bits are the same on any GPU:
 *   tiles = ceil(N / 128) ceil(K / 128)     want = min(32, max(1, 256 / tiles))   (integer division)
 *   rows_per_slab = round_up(ceil(M / want), 256)     slabs = ceil(M / rows_per_slab)
 * Slab i holds rows [i rows_per_slab, min(M, (i + 1) rows_per_slab)); within a slab the rows are added in 32-row MFMA steps in index
 * order; with more than one slab each slab's partial goes to scratch and the partials are added in slab order.
 * pcad_linear_wgrad_slabs returns slabs and stores rows_per_slab (host only, no device; M == 0: 0 and 0; a refused shape: -1 and the
 * message in pcad_last_error()).
 *   scratch    pcad_linear_wgrad_scratch_bytes(M, N, K) = slabs > 1 ? round_up(slabs N K 4, 256) : 0 bytes (0 for a refused shape);
 *              may be NULL when that is 0
 * M == 0: with accumulate nothing is done, without it dw is written as zeros. */
int64_t pcad_linear_wgrad_slabs(int64_t M, int N, int K, int64_t* rows_per_slab_out);
size_t pcad_linear_wgrad_scratch_bytes(int64_t M, int N, int K);
int pcad_linear_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw,
                      int64_t M, int N, int K, int accumulate, void* scratch, size_t scratch_bytes, pcad_stream stream);

/* ---- LoRA dropout: the masked rank-r down-projection of a LoRA branch and its backward ------------------------
 * Replaces: `lora_A(F.dropout(x, p))` of a PEFT LoRA layer and its backward, without the dropped copy of x and without a mask tensor.
 * The mask is a pure function of (seed, stream_id, row, column).  For a drop probability p in [0, 1):
 *   T = floor(p 65536 + 0.5)   (T = 65536 is refused)        c = 65536 / (65536 - T) as fp32: the keep scale, unbiased for this mask
 *   Philox4x32-10 (multipliers 0xD2511F53, 0xCD9E8D57; Weyl constants 0x9E3779B9, 0xBB67AE85) with
 *   counter = (k >> 3, m, stream_lo, stream_hi), key = (seed_lo, seed_hi) gives the words w0..w3
 *   h = (w[(k & 7) >> 1] >> (16 (k & 1))) & 0xffff           keep(m, k) = (h >= T)
 * m is the row index within the call, k the column.  One generator call covers 8 consecutive columns; the mask does not depend on K,
 * on the leading dimension or on the dtype.  p = 0: T = 0, c = 1, everything is kept.
 *
 * Shared limits, each decided without a device (PCAD_ERR_INVALID naming the argument): r in {4, 8, 16}; K % 8 == 0, 8 <= K <= 8192;
 * ldx, lddx multiples of 8 and >= K; x, dx, A, t, u, dA 16-byte aligned; 0 <= M < 2^32; p with T <= 65535; dtype PCAD_BF16 / PCAD_F32.
 *
 * pcad_lora_dropout_mask writes keep(m, k) as bytes (1 / 0) into keep_u8 [M, K], row stride ldk >= K bytes.  It exists so that the
 * device generator can be compared bit for bit with a restatement; it is not on the training path. */
int pcad_lora_dropout_mask(uint8_t* keep_u8, int64_t M, int K, int64_t ldk, double p, uint64_t seed, uint64_t stream_id, pcad_stream stream);

/* t[m, j] = c sum_k keep(m, k) x[m, k] A[j, k]: fp32 products and sums, t fp32 [M, r] contiguous.
 *   x [M, K] dtype, row stride ldx;  A fp32 [r, K] contiguous
 * Per row the lane that owns columns 8 l .. 8 l + 7 of each 512-column chunk adds its products in column order, chunk after chunk; the
 * 64 lanes' sums are added by the xor butterfly (32, 16, ... 1) and the total is multiplied by c once.  M == 0: nothing is done. */
int pcad_lora_down(const void* x, int64_t ldx, const float* A, float* t, int64_t M, int K, int r, double p, uint64_t seed,
                   uint64_t stream_id, int dtype, pcad_stream stream);

/* The backward of pcad_lora_down for the same (p, seed, stream_id), with u = dL/dt fp32 [M, r] contiguous:
 *   dA[j, k] = c sum_m keep(m, k) u[m, j] x[m, k]                                    fp32 [r, K] contiguous, overwritten
 *   dx[m, k] = round_dtype(dx[m, k] + c keep(m, k) sum_j u[m, j] A[j, k])            [M, K] dtype, row stride lddx
 * This entry is a stated exception to "every output is overwritten": dx is updated IN PLACE - the caller hands over dx0 = dy W, the
 * gradient through the frozen weight, and receives the sum; a dropped element keeps dx0's bits.  dx or dA may be NULL (not
 * computed), not both; neither changes the other's bits.
 * The rows are cut into slabs by (M, K) and the constants of csrc/kernels.hpp alone - never by the device:
 *   chunks = ceil(K / 512)     want = min(256, max(1, 1024 / chunks))   (integer division)
 *   rows_per_slab = round_up(ceil(M / want), 64)     slabs = ceil(M / rows_per_slab)
 * Within a slab and a 512-column chunk, wave w of 4 adds rows w, w + 4, ... in index order, the four waves' sums are added in wave
 * order, the slab's partial goes to scratch [slab][r][K] and a second kernel adds the slabs in slab order and multiplies by c once.
 * The sum over j runs in index order.  No floating-point atomics.
 * pcad_lora_down_bwd_slabs returns slabs and stores rows_per_slab (host only; M == 0: 0 and 0; a refused shape: -1 and the message in
 * pcad_last_error()).
 *   scratch    pcad_lora_down_bwd_scratch_bytes(M, K, r) = round_up(slabs r K 4, 256) bytes (0 for a refused shape); needed only with
 *              dA, may be NULL when that is 0
 * M == 0: dA (when given) is written as zeros, nothing else is done. */
int64_t pcad_lora_down_bwd_slabs(int64_t M, int K, int r, int64_t* rows_per_slab_out);
size_t pcad_lora_down_bwd_scratch_bytes(int64_t M, int K, int r);
int pcad_lora_down_bwd(const void* x, int64_t ldx, const float* A, const float* u, void* dx, int64_t lddx, float* dA, void* scratch,
                       size_t scratch_bytes, int64_t M, int K, int r, double p, uint64_t seed, uint64_t stream_id, int dtype,
                       pcad_stream stream);

/* ---- The selective scan's backward in segments: long strands at a small batch ---------------------------------
 * pcad_selective_scan_bwd (include/pcad_train.h) gives one wave to (strand, 64 channels), and that wave walks all L steps alone; a call
 * of few long strands leaves most of the device idle.  This entry computes the same gradients - the formulas, operands, alignment
 * rules and refusals of pcad_selective_scan_bwd, every output overwritten - with every strand cut into segments that are walked in
 * parallel, one wave per (strand, segment, 64 channels).  csrc/scan_bwd_seg.hip; the kernel of the walk itself is the one of
 * libpcad_train.so (csrc/scan_bwd_kernel.hpp).
 *
 * Segment rule, T = 8 walk steps (the steps per stored state): steps = T ceil(ceil(L / segments) / T) steps per segment, so that
 * segments start on the boundaries of the stored states; G = ceil(L / steps) <= segments segments exist, segment g owns the walk
 * steps [g steps, min(L, (g + 1) steps)).  pcad_selective_scan_bwd_seg_steps returns steps (host only; 0: L < 1 or segments outside
 * [1, 64]).
 *
 * Both recurrences are linear in what they carry, with the same coefficients a_s[n] = exp(d_s A[c,n]):
 *   h_s = a_s h_{s-1} + d_s u_s B_s                       (the state, walked up)
 *   kc_{s-1} = a_s (dy_s C_s + kc_s)                      (kc_s = a_{s+1} k_{s+1}: the adjoint handed down)
 *   phase 1, per (strand, segment, 64 channels), all in parallel: from h = 0 up the segment -> e_g[n] and Dsum_g = sum d_s (g < G - 1);
 *            from kc = 0 down the segment -> kappa_g[n] (g > 0);  P_g[n] = exp(A[c,n] Dsum_g)
 *   phase 2, per (strand, channel, n), serial over the segments in a fixed order: H_0 = 0, H_{g+1} = P_g H_g + e_g ascending;
 *            K_{G-1} = 0, K_{g-1} = P_g K_g + kappa_g descending
 *   phase 3, the two-pass walk of pcad_selective_scan_bwd per (strand, segment, 64 channels): the states from H_g instead of zero, the
 *            adjoint from K_g instead of zero; dA, dD and dbias partials per (strand, segment), added in index order
 * All fp32.  The results differ from pcad_selective_scan_bwd's by fp32 rounding only (the carried values are re-associated), and a call
 * gives the same bits every time for given segments.  With G == 1 (segments == 1, or L <= steps) the unsegmented kernel runs and the
 * results are pcad_selective_scan_bwd's bit for bit.
 *   segments   1 .. 64 (else PCAD_ERR_INVALID)
 *   scratch    pcad_selective_scan_bwd_seg_scratch_bytes(S, L, E, segments) bytes (0 for a refused shape), 256-byte aligned: the sections of
 *              pcad_selective_scan_bwd's scratch - the states at the chunk boundaries, where H_g takes the slot of segment g's first
 *              chunk, and the partial sums, dA / dD / dbias now one row per (strand, segment) - followed by e [S, G, 16, E],
 *              kappa [S, G, 16, E] (K_{g-1} overwrites kappa_g in phase 2) and Dsum [S, G, E]
 * S == 0 or L == 0: OK, nothing is done. */
int pcad_selective_scan_bwd_seg_steps(int L, int segments);
size_t pcad_selective_scan_bwd_seg_scratch_bytes(int S, int L, int E, int segments);
int pcad_selective_scan_bwd_seg(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc,
                                const float* A, const float* Dskip, const float* delta_bias, const void* dout,
                                void* du, void* ddelta, void* dz, float* dbc, float* dA, float* dD, float* ddelta_bias,
                                void* scratch, size_t scratch_bytes, int S, int L, int E, int reverse, int dtype, int segments,
                                pcad_stream stream);

/* ---- The selective scan's training forward in segments ----------------------------------------------------------
 * The forward of pcad_selective_scan (include/pcad.h) on plain rows with an explicit delta - the call the training path makes -, with
 * every strand cut by the rule above (steps = pcad_selective_scan_bwd_seg_steps(L, segments), G = ceil(L / steps) segments: the forward's
 * cuts are the backward's) and one wave per (strand, segment, 64 channels).  csrc/scan_fwd_seg.hip.  Per strand and channel c, walk
 * step s visiting row t = s (reverse 0) or L - 1 - s (reverse 1):
 *   d_t = softplus(delta_t + delta_bias_c)     h_s[n] = exp(d_t A[c,n]) h_{s-1}[n] + d_t u_t B_t[n]     y_t = sum_n h_s[n] C_t[n] + Dskip_c u_t
 *   out_t = y_t silu(z_t)  (z given)  or  y_t
 *   phase 1, per (strand, segment g < G - 1, 64 channels): from h = 0 up the segment -> e_g[n] and Dsum_g = sum d_s
 *   phase 2, per (strand, channel, n), serial over g ascending: H_0 = 0, H_{g+1} = exp2(A[c,n] log2(e) Dsum_g) H_g + e_g
 *   phase 3, per (strand, segment, 64 channels): the walk from H_g; out_t rounded once to dtype and stored once
 * u and delta are read in dtype, everything in between is fp32.  No floating-point atomics: a call gives the same bits every time for
 * given segments.  The result differs from pcad_selective_scan's by fp32 rounding - also with G == 1 (segments == 1, or L <= steps),
 * which runs phase 3 alone from a zero state: a different kernel from pcad_selective_scan's.
 *   u, delta, y  [S, L, E] dtype;  z [S, L, ldz >= E] dtype or NULL (ungated);  bc fp32 [S L, 32] = B_t | C_t, 16-byte aligned
 *   A fp32 [E, 16] (raw, = -exp(A_log));  Dskip, delta_bias fp32 [E];  E % 64 == 0;  segments 1 .. 64
 *   scratch    pcad_selective_scan_fwd_seg_scratch_bytes(S, L, E, segments) bytes (0 for a refused shape), 256-byte aligned, two sections
 *              each a multiple of 256 bytes: e / H [S, G, 16, E] (H_g overwrites e_g in phase 2) and Dsum [S, G, E]
 * PCAD_ERR_INVALID also when S G E / 64 waves or S 16 E / 256 blocks do not fit a 32-bit grid.  S == 0 or L == 0: OK, nothing is done. */
size_t pcad_selective_scan_fwd_seg_scratch_bytes(int S, int L, int E, int segments);
int pcad_selective_scan_fwd_seg(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc,
                                const float* A, const float* Dskip, const float* delta_bias, void* y,
                                void* scratch, size_t scratch_bytes, int S, int L, int E, int reverse, int dtype, int segments,
                                pcad_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PCAD_BWD_H */
