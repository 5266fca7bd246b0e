/*
 * pcad.h — C ABI of the MI355X-native PlantCaduceus forward engine (libpcad.so).
 *
 * Drop-in boundary for ONE path of kuleshov-group/PlantCaduceus: the masked-LM forward that
 * `src/zero_shot_score.py:115` (`model(input_ids=curIDs)`) and `src/train_XGBoost.py:104`
 * (`model(input_ids=..., output_hidden_states=True)`) run, i.e. the third-party operators
 *   mamba_ssm.ops.selective_scan_interface.selective_scan_fn / mamba_inner_fn   (mamba-ssm==2.2.2)
 *   causal_conv1d.causal_conv1d_fn                                              (causal-conv1d==1.4.0)
 *   mamba_ssm.ops.triton.layer_norm.rms_norm_fn                                 (Triton fused add-norm)
 *   CaduceusMixer / RCPS wrappers                                               (HF-hub remote code)
 * pinned by reference env/requirements.txt:9-10 and env/environment.yml:12.
 *
 * Conventions
 *   - plain C: pointers and sizes only; no torch / HIP types in any signature (`pcad_stream` is a
 *     hipStream_t passed as void*).
 *   - every buffer and every stream is OWNED BY THE CALLER (ids, outputs, weights, weight arena, workspace); the library
 *     owns only the opaque handle (plus the HIP events of the optional profiling mode, freed with it).
 *     No allocation, no host synchronisation inside pcad_forward.
 *   - all work is enqueued on the caller's stream; a handle is bound to the current device and is not
 *     thread-safe; distinct handles on distinct devices are independent (one process per GPU).
 *   - status: 0 = OK, negative = error (enum below); message via thread-local pcad_last_error().
 *   - activation layout is token-major: [strand, position, channel] (channel contiguous).
 */
#ifndef PCAD_H
#define PCAD_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PCAD_VERSION 100 /* 0.1.0 */
#define PCAD_MAX_VOCAB 8
#define PCAD_MAX_POSITIONS 16

typedef void* pcad_stream;            /* hipStream_t */
typedef struct pcad_engine* pcad_handle;

enum pcad_status {
    PCAD_OK = 0,
    PCAD_ERR_INVALID = -1,      /* bad argument / unsupported shape */
    PCAD_ERR_UNBOUND = -2,      /* weights not bound */
    PCAD_ERR_WORKSPACE = -3,    /* workspace or arena too small / misaligned */
    PCAD_ERR_MISSING = -4,      /* a required tensor name was not supplied */
    PCAD_ERR_HIP = -5           /* HIP runtime error (launch failure, ...) */
};

enum pcad_dtype { PCAD_F32 = 0, PCAD_BF16 = 1 };

/* Model geometry (HF config.json of the snapshot; replaces CaduceusConfig -> Mamba(**ssm_cfg)).
 * pcad_create accepts d_model a multiple of 64 up to 2048, n_layer >= 1, expand >= 1, dt_rank 1 .. 256, both dtypes and
 * residual_in_fp32 0 or 1 (read on the bf16 model only; a bf16 residual stream is never norm-folded); anything else is
 * PCAD_ERR_INVALID with a message that names the field and its value. */
typedef struct pcad_config {
    int32_t d_model;            /* D */
    int32_t n_layer;
    int32_t d_state;            /* N, must be 16 */
    int32_t d_conv;             /* W, must be 4 */
    int32_t expand;             /* E = expand * D */
    int32_t dt_rank;            /* R */
    int32_t vocab;              /* padded vocabulary, must be 8 */
    float   eps;                /* RMSNorm epsilon (1e-5) */
    int32_t dtype;              /* pcad_dtype of activations / GEMM operands (torch_dtype of the model) */
    int32_t residual_in_fp32;   /* residual stream kept in fp32 (reference default) */
    int32_t complement[PCAD_MAX_VOCAB]; /* token id -> complementary base id (RCPS) */
} pcad_config;

/* A named tensor in the reference's state-dict naming, device memory, row-major. */
typedef struct pcad_tensor {
    const char* name;
    const void* data;
    int32_t     dtype;          /* pcad_dtype */
    int32_t     ndim;
    int64_t     shape[4];
} pcad_tensor;

int         pcad_version(void);
const char* pcad_last_error(void);
/* sha1 (16 hex digits) over the kernel sources the library was built from (csrc/source_hash.py): a loader that has the
 * sources beside it compares the two and refuses a stale binary (plantcaduceus_amd/engine.py, bench.py). */
const char* pcad_build_hash(void);

/* Replaces: AutoModelForMaskedLM.from_pretrained(...).to(device)  (src/zero_shot_score.py:91-97) */
int    pcad_create(const pcad_config* cfg, pcad_handle* out);
void   pcad_destroy(pcad_handle h);

/* Options (call before pcad_workspace_bytes / pcad_forward):
 *   "chunk_seqs"  windows per pass through the layer stack (0 = default: as many as the kernels' unsigned 32-bit in-tensor
 *                 offsets allow, (2^32 - 2 MiB) / (d_inner * elem) token-rows = 1 023 windows of 512 bp at l32 bf16, the batch
 *                 split evenly into the fewest such chunks - or into up to twice as many when that makes the chunk's token-rows a
 *                 multiple of 16 384, i.e. whole rounds of the persistent GEMMs: the fp32 model's 1 024 windows run as 4 x 256, not
 *                 3 x 342).  Results do not depend on it (rows are independent) - bit for bit
 *                 (the small-launch forms of "scan_segments" are chosen for the whole batch of the call, not per chunk)
 *                 whenever every chunking runs the same layer form, which holds for window lengths that are multiples of 128
 *                 (every shipped use); for other lengths "norm_fold" engages per chunk (whole 256-row tiles only), so two
 *                 chunkings of a bf16 batch can differ by bf16 rounding; the
 *                 workspace does: ~30 MB per window at l32 bf16, i.e. up to ~30 GB for one 1 023-window chunk (a batch of
 *                 1 024 runs as two chunks of 512 in a 15.3 GB workspace) - always size it with pcad_workspace_bytes.
 *   "workspace_limit_mb"  N > 0: chunks are sized so that pcad_workspace_bytes stays at or below N MiB whatever the batch (a server
 *                 holding several models on one GPU bounds each one's slab; the default chunking takes up to ~30 GB for a
 *                 1 023-window chunk at l32 bf16); smaller chunks cost throughput (1 024 windows as 16 chunks instead of 2: -7 %),
 *                 never results.  One window always runs, even if its workspace exceeds the limit.  0 (default): no limit.
 *   "last_layer_shortcut"  1 (default): when pcad_forward is given a list of positions, the LAST layer's scans stop at the
 *                 furthest evaluated row and its out_proj runs on the evaluated rows only (bit-identical outputs);  0: full layer.
 *   "gate_each"   1: SiLU(z) applied to each direction's scan output, each rounded, then summed — the reference's order
 *                 (two selective_scan_fn calls);  0 (default): applied once to the sum of both directions (same value in
 *                 exact arithmetic, one rounding fewer, faster).
 *   "norm_fold"   1 (default for the bf16 model; -1 restores "default"): the fused add + RMSNorm launch between two blocks is folded
 *                 into the GEMMs around it: out_proj's epilogue
 *                 adds its fp32 result to the fp32 residual stream in place and writes the rounded sum plus per-row partial sums of
 *                 squares (deterministic, no atomics); in_proj runs on that un-normalised operand with W_in . diag(w_norm) (folded
 *                 when the weights are bound) and multiplies by the row's rstd before it rounds.  Same value in exact arithmetic
 *                 as rms_norm_fn(prenorm=True, residual_in_fp32=True); rounding points move (the mixer output is not rounded
 *                 before it is added; in_proj's operand is round(res) instead of round(res * rstd * w)).  Used for chunks whose
 *                 token-rows are whole 256-row tiles (a d_model that is not a multiple of 256 - PlantCaduceus_l20's 384 - is padded
 *                 to the next one inside the workspace) with an fp32 residual stream,
 *                 never by pcad_forward_all_hidden (+4.5 % end to end, same-box A/B, profiles/r04_ab_runs.txt).  Decided once
 *                 per pcad_forward call: every chunk of the batch runs folded or none does.  The form needs extra weight copies
 *                 (+37 % of the arena at l32) that are carved and packed only if the options in force at
 *                 pcad_weight_arena_bytes / pcad_bind_weights time ask for it: set "norm_fold" 1 on an fp32 model BEFORE those
 *                 calls (afterwards pcad_forward refuses); turning it off later is always possible;
 *                 0 (default for the fp32 model, whose 1e-4 parity budget would pay for accumulating onto the residual: 2.2e-5 of
 *                 max after 32 layers instead of 1.3e-6): the reference's operation order (one add + RMSNorm launch per block).
 *   "f32_gemm_split"  1: the fp32 model's two big projections (in_proj, out_proj: 3/4 of its time on the fp32 MFMA instructions) run
 *                 as split-bf16 GEMMs (pcad_gemm_nt_split below: three bf16 products per fp32 product, fp32 accumulation and
 *                 result); everything else of the fp32 model is unchanged.  Measured 4e-7 of the logits' range against the fp32
 *                 oracle after 32 layers (the plain fp32 GEMMs: 1e-6), arg-max exact - inside north_star's 1e-4 - at about twice
 *                 the fp32 model's speed.  0 (default): fp32 MFMA.  Needs bf16 [hi | lo] weight copies (the size of the fp32 weights
 *                 again) packed at bind time: set it before pcad_weight_arena_bytes / pcad_bind_weights.  Ignored by the bf16 model
 *                 and while "norm_fold" 1 is forced.  Operands are stored once as [hi | lo] (the byte size of the fp32 tensor) and
 *                 the GEMMs' K-tile cursor wraps around them (hi.hi, lo.hi, hi.lo), so the chunk cap is the fp32 model's own,
 *                 (2^32 - 2 MiB) / (4 d_inner) token-rows.  "last_layer_shortcut" runs the evaluated rows through the same
 *                 split-bf16 product (bit-identical to the full layer).
 *   "untied_directions"  1: mamba_fwd and mamba_rev each have their own in_proj / out_proj (per-direction LoRA deltas merged into the
 *                 weights; a model trained with bidirectional_weight_tie = False).  pcad_bind_weights then REQUIRES
 *                 `mamba_rev.in_proj.weight` / `mamba_rev.out_proj.weight` of every layer (PCAD_ERR_INVALID names a missing one) and packs
 *                 them beside mamba_fwd's (with "f32_gemm_split" also their [hi | lo] copies): set it before pcad_weight_arena_bytes /
 *                 pcad_bind_weights (afterwards pcad_forward refuses).  Every forward entry then walks each layer in the strict
 *                 reference order ("reference_order" 2) with per-direction operands: one add + RMSNorm, in_proj twice, per direction
 *                 conv + SiLU on its own x (pcad_causal_conv1d_silu_dir), x_proj, the scan gated with its own z, its own out_proj
 *                 rounded to the model dtype; the two are summed and rounded.  The norm-folded form, the layer-0 table, the fused
 *                 conv + x_proj kernel and the pair walks are off (they read one x / z for both directions); the segmented scan, the
 *                 last-layer shortcut, chunking and "f32_gemm_split" work as usual.  pcad_workspace_bytes grows by the second x / z
 *                 pair.  0 (default): the tied form; of a pair of tied tensors the engine reads mamba_fwd's.  Nothing about the
 *                 tied form (launches, arena and workspace sizes, results) depends on this option existing.
 *   "reference_order"  one switch over the options above, for users who want every rounding point where the reference has it
 *                 (BiMambaWrapper "add" of two Mamba calls, rms_norm_fn(prenorm=True, residual_in_fp32=True), mamba_inner_fn):
 *                 0 (default): the engine's defaults ("gate_each" 0, "norm_fold" default, layer 0's in_proj as a table);
 *                 1: "gate_each" 1 + "norm_fold" 0 (hence no layer-0 table) - the only reordering left is the tied out_proj applied
 *                    once to y_fwd + y_rev (linearity) instead of once per direction;
 *                 2: strict - additionally each direction's scan output gets its own tied out_proj launch, each result is stored in
 *                    the model dtype, and the two are added and rounded, exactly BiMambaWrapper's `out + out_rev`: the rounding
 *                    points of oracle/c "ref_order".  What remains different from the reference is fp32 summation order inside the
 *                    GEMMs / scan and the exp / log implementations - the noise any two BLAS libraries have between them.
 *                 Cost at l32 bf16 (same box, profiles/r05_*): see INTEGRATION.md "Operation order".  Setting "gate_each" /
 *                 "norm_fold" afterwards overrides the respective part; level 2 is ignored while "norm_fold" is forced to 1.
 *   "scan_segments"  1 (default): when a launch has few scan waves (at most 768 for L >= 2 048: PlantCAD2's 8 192-bp windows in small
 *                 batches; at most 512 for shorter windows: up to 8 windows of 512 bp at l32) the scan of every strand is cut into up to 8 (short windows: 16, of at least 32 steps) segments that run as
 *                 separate workgroups (zero-state pass, carry, real pass: ~1.8x the arithmetic for up to 8x the parallelism;
 *                 results equal up to fp32 rounding of the carried decay product);  0: one workgroup walks the whole strand.
 *                 Launches with more waves than that but at most 3 584 per direction (3.5 per SIMD: 32 windows of 8 192 bp at the
 *                 PlantCAD2 Medium / Large widths, up to 56 windows of 512 bp at l32) take the PAIR form instead (round 6): both
 *                 directions of a layer run in one launch and walk half a strand per launch - forward rows [0, L/2) with reverse rows
 *                 [L/2, L), then the other halves from the kept states, each adding what the other direction's first launch left and
 *                 gating: twice the waves per launch, the same arithmetic, no extra pass (L % 64 == 0; never the last layer, whose
 *                 walks "last_layer_shortcut" shortens).  Against the plain two-launch form the bf16 model's gate-once sum is rounded
 *                 at the other direction's partial on half of the rows: equal to bf16 rounding of one addend (fp32: summation order;
 *                 with "gate_each" / "reference_order" >= 1: bit-identical in both dtypes).  +13 % at 32 x 8 192 bp (Medium), +12 % at 16 x 512 bp.
 *                 The same switch governs the K-split of the fused conv + x_proj kernel for launches of at most 64 row tiles (up to 8
 *                 windows of 512 bp): several blocks per row tile each walk a share of the channels and a second tiny kernel adds
 *                 their partial x_proj sums in a fixed order (deterministic; another fp32 summation order than the unsplit walk).
 *                 Both forms are selected from the batch size of the pcad_forward call (not from the chunk), so two calls with the
 *                 same batch agree bit for bit whatever "chunk_seqs" is; calls with different batch sizes may differ by fp32 rounding
 *                 of these sums when one of them is small enough to take a split form.
 *                 Never used by the benchmark batch (1 024 windows: 65 536 waves).
 *   "debug_repeat_class" / "debug_repeat"  measurement aid (tools/power_probe.py): every idempotent launch of ONE pcad_kernel_class
 *                 (in_proj, conv + x_proj, the forward-direction scan, the reference-order out_proj) is issued `debug_repeat` times
 *                 back to back, so that a forward is seconds of that kernel at the engine's own launch sizes while board power is
 *                 sampled; outputs are unchanged.  Default: class -1 (none), repeat 1.
 *   "poison_workspace"  1: debug aid — the workspace is filled with 0xFF bytes (NaN in every dtype) before each forward, so a
 *                 read of anything this forward did not write shows up as NaN outputs (tests/test_gpu_model.py).
 * The library reads NO environment variables unless PCAD_DEV=1 is set (developer A/B switches, see csrc/kernels.hpp). */
int    pcad_set_option(pcad_handle h, const char* key, int64_t value);

/* Asynchronous input validation.  The reference raises (nn.Embedding index error / tensor index error) for a token id
 * outside the vocabulary or an evaluated position outside the window; pcad_forward* never synchronise, so they report these
 * through a caller-owned DEVICE word: bit PCAD_STATUS_BAD_TOKEN / PCAD_STATUS_BAD_POSITION is OR-ed into *status by the
 * forward's last kernel (such an id is embedded as id & 7, such a position is clamped, so nothing is read out of bounds and
 * the affected rows are simply wrong).  The caller zeroes the word, and reads it at its next synchronisation point.
 * NULL (default): no reporting.  pcad_forward_loss adds PCAD_STATUS_BAD_LABEL: a label that is neither ignored nor inside the
 * vocabulary (the reference's cross entropy raises a device assert); such a position contributes nothing. */
enum pcad_status_bits { PCAD_STATUS_BAD_TOKEN = 1, PCAD_STATUS_BAD_POSITION = 2, PCAD_STATUS_BAD_LABEL = 4 };
int    pcad_set_status_buffer(pcad_handle h, int32_t* status);

/* Bytes of caller-owned device memory that pcad_bind_weights packs the model into (depends on "norm_fold" / "reference_order" as set
 * when it is called: query it after the options, right before binding). */
size_t pcad_weight_arena_bytes(pcad_handle h);

/* Pack the reference-named tensors (fp32 or bf16, device pointers) into `arena` in the engine's layouts
 * (padded x_proj / dt_proj, pre-exponentiated A, tied in_proj/out_proj stored once).  Tied duplicates
 * (`mamba_rev.in_proj/out_proj`, `lm_head`) may be absent (not `mamba_rev.in_proj/out_proj` under "untied_directions" 1).  The arena must outlive the handle. */
int    pcad_bind_weights(pcad_handle h, const pcad_tensor* tensors, int n,
                         void* arena, size_t arena_bytes, pcad_stream stream);

/* Workspace needed by pcad_forward for `batch` sequences of `seqlen` tokens (both strands). */
size_t pcad_workspace_bytes(pcad_handle h, int batch, int seqlen);

/* Replaces: outputs = model(input_ids=ids[, output_hidden_states=True])
 *           (src/zero_shot_score.py:115; src/train_XGBoost.py:104).
 *   ids        device int32 [B, L] token ids (0..7)
 *   positions  HOST int32 [P] sequence positions to evaluate, or NULL with P == 0 for all L positions
 *              (P <= PCAD_MAX_POSITIONS).  Let Q = P ? P : L.
 *   hidden_out device [B, Q, 2*D] in cfg.dtype, or NULL: hidden_states[-1] rows
 *              (= cat(H(ids)[p], reverse_channels(H(rc ids)[L-1-p])))
 *   logits_out device fp32 [B, Q, vocab], or NULL: RCPS LM-head logits (`.logits.float()`)
 */
int    pcad_forward(pcad_handle h, const int32_t* ids, int B, int L,
                    const int32_t* positions, int P,
                    void* hidden_out, float* logits_out,
                    void* workspace, size_t workspace_bytes, pcad_stream stream);

/* In-silico-mutagenesis form (reference pipelines/in-silico-mutagenesis -> src/zero_shot_score.py -input-vcf, one
 * masked forward per variant position): window b is evaluated at its own position pos_per_seq[b] (device int32 [B]; a value
 * outside [0, L) is clamped AND reported through pcad_set_status_buffer).  hidden_out [B, 1, 2*D] / logits_out [B, 1, vocab],
 * either may be NULL. */
int    pcad_forward_at(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* pos_per_seq,
                       void* hidden_out, float* logits_out,
                       void* workspace, size_t workspace_bytes, pcad_stream stream);

/* Per-layer mixer outputs for the last pcad_forward are not kept; this variant additionally writes
 * hidden_states[0..n_layer-1] (the inputs of every block) to `all_hidden` ([n_layer, B, L, 2*D],
 * cfg.dtype) — the `output_hidden_states=True` tuple of the reference minus its last entry. */
int    pcad_forward_all_hidden(pcad_handle h, const int32_t* ids, int B, int L,
                               void* all_hidden, void* hidden_out, float* logits_out,
                               void* workspace, size_t workspace_bytes, pcad_stream stream);

/* Sequence classification (fine-tuned PlantCAD2 models: CaduceusForSequenceClassification, RCPS, pooling_strategy).
 * The same layer walk as pcad_forward with positions == NULL (every row of the last layer is consumed: no last-layer shortcut),
 * ending in the pooled head instead of the LM head:
 *   hs_s[p]    = norm_f(res + h) of strand s's own row p (s = 0: the window, s = 1: its reverse complement), rounded to cfg.dtype
 *   pooled_s   = mean (fp32 sum / L, rounded once to cfg.dtype) / max / row 0 / row L-1 of hs_s over p  (pad tokens included)
 *   logits[n]  = round(round(round(pooled_0 . W[n]) + round(pooled_1 . W[n])) / 2)      (round: to cfg.dtype; fp32 accumulation)
 *   pooling    pcad_pooling;  score_w  DEVICE fp32 [num_labels, D], already rounded to cfg.dtype (the `score` Linear's weight);
 *   num_labels 1..PCAD_MAX_LABELS;  pooled_out DEVICE fp32 [B, 2, D] or NULL;  logits_out DEVICE fp32 [B, num_labels] (required).
 * The head's partials live in workspace buffers that are dead after the last out_proj: pcad_workspace_bytes is the forward's own.
 * Token ids outside the vocabulary are reported through pcad_set_status_buffer as by pcad_forward.
 * Replaces: CaduceusForSequenceClassification(...)(input_ids=ids).logits (HF-hub remote code, as loaded by the reference's
 *           src/lora_fine_tune.py load_base_model + PeftModel.from_pretrained). */
enum pcad_pooling { PCAD_POOL_MEAN = 0, PCAD_POOL_MAX = 1, PCAD_POOL_FIRST = 2, PCAD_POOL_LAST = 3 };
#define PCAD_MAX_LABELS 256
int    pcad_forward_pooled(pcad_handle h, const int32_t* ids, int B, int L, int pooling, const float* score_w, int num_labels,
                           float* pooled_out, float* logits_out, void* workspace, size_t workspace_bytes, pcad_stream stream);

/* Masked-LM loss (CaduceusForMaskedLM with labels; the --do_eval / --do_test half of the reference's src/HF_pre_train.py; DESIGN.md
 * §4g).  The same layer walk as pcad_forward with positions == NULL (every row may be consumed: no last-layer shortcut), ending in
 * the loss head instead of the LM head.  For every position p of window b whose label is not ignored:
 *   logit[v] = pcad_forward's logits_out[b, p, v]  (the same arithmetic and rounding points, bit for bit)
 *   nll      = logsumexp_v(logit) - logit[label]   (fp32, over all `vocab` logits, as F.cross_entropy)
 *   labels        DEVICE int32 [B, L]; ignored when == ignore_index or < 0; any other value outside [0, vocab) sets
 *                 PCAD_STATUS_BAD_LABEL (pcad_set_status_buffer) and contributes nothing
 *   loss_weights  DEVICE fp32 [B, L] per-token weights w, or NULL (w = 1); the weight of an ignored position is never read into a sum
 *   sums_out      DEVICE fp32 [B, 4] (required), per window: sum w nll, sum w, number of labelled positions, number of labelled
 *                 positions whose arg-max logit (first index on ties) equals the label
 *   nll_out       DEVICE fp32 [B, L] or NULL: nll (unweighted), 0 at ignored positions
 *   logits_out    DEVICE fp32 [B, L, vocab] or NULL: as pcad_forward writes them; when NULL, rows whose label is ignored are not read
 * Two stages (per-segment partials, then one fixed-order sum per window), no floating-point atomics; the segmentation depends on L
 * only, so with "scan_segments" 0 a window's results are bit-identical alone, in any batch and under any "chunk_seqs".  The partials
 * live in workspace buffers that are dead after the last out_proj: pcad_workspace_bytes is the forward's own. */
int    pcad_forward_loss(pcad_handle h, const int32_t* ids, const int32_t* labels, const float* loss_weights, int ignore_index,
                         int B, int L, float* sums_out, float* nll_out, float* logits_out,
                         void* workspace, size_t workspace_bytes, pcad_stream stream);

/* Nucleotide probabilities: the forward ending in the probability head instead of the LM head.  For every evaluated
 * (window b, position p):
 *   logit[v]  = pcad_forward's logits_out[b, q, v]  (the same arithmetic and rounding points, bit for bit)
 *   probs[j]  = exp(logit[cols[j]] - m) / sum_j exp(logit[cols[j]] - m),  m = max_j logit[cols[j]]     (fp32, as torch.softmax; the
 *               only roundings after the logits are fp32's own: four exp, three adds, four divisions)
 * Exactly one position form per call.  Let Q = L, P or P:
 *   1. positions == NULL, pos_per_window == NULL, P == 0: all L positions; pcad_forward's layer walk
 *   2. positions HOST int32 [P], 1 <= P <= PCAD_MAX_POSITIONS, shared by every window (each inside [0, L), else PCAD_ERR_INVALID);
 *      pcad_forward's layer walk, "last_layer_shortcut" included
 *   3. pos_per_window DEVICE int32 [B, P], 1 <= P <= PCAD_MAX_POSITIONS: window b is evaluated at its own P positions (P == 1:
 *      pcad_forward_at's form); a value outside [0, L) is clamped AND reported as PCAD_STATUS_BAD_POSITION; pcad_forward_at's
 *      layer walk (the full last layer)
 *   cols        HOST int32 [4]: the vocabulary columns of the four classes, each inside [0, vocab) (the reference: the token ids of
 *               a, c, g, t)
 *   probs_out   DEVICE fp32 [B, Q, 4], 16-byte aligned, or NULL;  logits_out  DEVICE fp32 [B, Q, vocab] or NULL (not both NULL)
 * One wave computes one (window, position) from that window's rows only and stores it once: with "scan_segments" 0 a window's
 * probabilities are bit-identical alone, in any batch and under any "chunk_seqs".  pcad_workspace_bytes is the forward's own.
 * PCAD_ERR_INVALID: cols outside [0, vocab); P outside its range; both position forms given.  Token ids outside the vocabulary are
 * reported through pcad_set_status_buffer as by pcad_forward.
 * Replaces: torch.softmax(model(input_ids=ids).logits[..., cols], dim=-1) at the read positions - src/zero_shot_score.py:116-119,
 *           _masked_probs / _unmasked_probs of src/zero-shot-eval.py:129-178, and the per-window boundary reads of its
 *           sv_effect (:425-472) in form 3. */
int    pcad_forward_probs(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* positions, int P,
                          const int32_t* pos_per_window, const int32_t* cols, float* probs_out, float* logits_out,
                          void* workspace, size_t workspace_bytes, pcad_stream stream);

/* Per-layer hidden states at the evaluated positions: chosen levels of the reference's `hidden_states` tuple
 * (output_hidden_states=True), only at the rows a caller reads, optionally as the reverse-complement-averaged fp32 embedding.
 *   layers      HOST int32 [NL], strictly increasing indices into the tuple, 1 <= NL <= n_layer + 1: 0 = the RCPSEmbedding output,
 *               k = the input of block k, n_layer = hidden_states[-1].  layers == NULL with NL == 0: all n_layer + 1 levels.
 *   positions   exactly one form, 1 <= P <= PCAD_MAX_POSITIONS: positions HOST int32 [P] shared by every window (each inside
 *               [0, L), else PCAD_ERR_INVALID), or pos_per_window DEVICE int32 [B, P] (a value outside [0, L) is clamped AND reported
 *               as PCAD_STATUS_BAD_POSITION).  There is no all-positions form: that is pcad_forward_all_hidden.
 *   out         DEVICE, 16-byte aligned.  average == 0: model dtype [NL, B, P, 2D], row = [forward strand's row | reverse-complement
 *               strand's row with channels reversed] - the rows [b, p, :] of pcad_forward_all_hidden's levels.  average != 0: fp32
 *               [NL, B, P, D] = (float(fwd[c]) + float(rc[c])) * 0.5f in straight channel order: what the reference's
 *               extract_embeddings forms from the plain row ((e[:D] + flip(e[D:])) / 2 on fp32), bit for bit.
 * Layer walk.  Only level n_layer requested: pcad_forward's walk for the shared list (norm fold and last-layer shortcut as that call
 * chooses them; the plain output is bit-equal to its hidden_out) and the full last layer for per-window lists (P == 1:
 * pcad_forward_at's walk and hidden_out).  Any level below n_layer requested: the unfolded walk of pcad_forward_all_hidden (no norm
 * fold), every level gathered right after it is produced, and only as deep as the highest requested level K: with K == n_layer all
 * blocks, the final norm and the head run as in that call; with K < n_layer blocks 0 .. K - 1 run and nothing after them (K == 0: no
 * block), the token ids being checked by a small kernel of their own.  For a shared list block K - 1 of such a call is shortened
 * as "last_layer_shortcut" shortens pcad_forward's last layer (scans stopped after the furthest evaluated row, out_proj on the
 * 2 B P gathered rows; "last_layer_shortcut" 0 turns it off; not taken where that block runs as a pair walk); per-window lists keep
 * the block whole.  In every case level k is bit-equal to all_hidden[k][b, p, :] (hidden_out[b, p, :] for k == n_layer) of a
 * pcad_forward_all_hidden call on the same batch under the same options.
 * pcad_workspace_bytes is the forward's own; nothing is allocated and nothing synchronises.  Token ids outside the vocabulary are
 * reported through pcad_set_status_buffer as by pcad_forward.
 * Replaces: model(input_ids=ids, output_hidden_states=True).hidden_states[k][:, p, :] and the strand averaging of
 *           src/train_XGBoost.py:104-110 (extract_embeddings) at any level k. */
int    pcad_forward_layers(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* positions, int P,
                           const int32_t* pos_per_window, const int32_t* layers, int NL, int average, void* out,
                           void* workspace, size_t workspace_bytes, pcad_stream stream);

/* ---- measurement: per-kernel-class timing with HIP events on the caller's stream -------------------- */
enum pcad_kernel_class {
    PCAD_K_NORM = 0, PCAD_K_GEMM_IN, PCAD_K_CONV, PCAD_K_GEMM_X, PCAD_K_SCAN, PCAD_K_GEMM_OUT, PCAD_K_HEAD,
    PCAD_K_GEMM_OUT_RES,   /* "norm_fold": out_proj + residual add + row statistics in one launch */
    PCAD_K_RSTD,           /* "norm_fold": the per-layer reduction of the row statistics (the layer-0 embedding kernel counts as PCAD_K_NORM) */
    PCAD_NUM_KERNEL_CLASSES
};
typedef struct pcad_kernel_stat {
    char    name[32];
    int64_t launches;
    double  total_ms;           /* sum of (stop - start) event times of this class's launches */
} pcad_kernel_stat;
/* on = 0: off; on = 1: every launch of pcad_forward is bracketed by a pair of hipEvents recorded on its stream;
 * on = N > 1: every N-th launch of each kernel class is (a sample over the same region at 1/N of the event overhead). */
int pcad_profile_enable(pcad_handle h, int on);
/* Waits for the recorded events, writes one entry per kernel class (<= max_out), resets the counters.
 * Returns the number of entries written (>= 0) or a negative status. */
int pcad_profile_read(pcad_handle h, pcad_kernel_stat* out, int max_out);

/* ---- per-operator entry points (unit parity against the operators they replace) ------------------ */

/* rms_norm_fn(x, weight, None, residual=residual, eps, prenorm=True, residual_in_fp32)
 *   x [rows, D] dtype; residual_in [rows, D] res_dtype or NULL; weight fp32 [D];
 *   y [rows, D] dtype; residual_out [rows, D] res_dtype or NULL.  D % 8 == 0, D <= 2048. */
int pcad_add_rmsnorm(const void* x, const void* residual_in, const float* weight,
                     void* y, void* residual_out, int64_t rows, int D, float eps,
                     int dtype, int res_dtype, pcad_stream stream);

/* causal_conv1d_fn(x, weight, bias, activation="silu"), both directions in one pass, token-major:
 *   x [S, L, ldx>=E] dtype (channel-contiguous rows); w_fwd/w_rev fp32 [E, 4]; b_fwd/b_rev fp32 [E]
 *   y_fwd[t] = silu(b + sum_k w[k] x[t-3+k])   (causal),  y_rev[t] = silu(b + sum_k w[k] x[t+3-k]) (anti-causal)
 *   y_fwd / y_rev [S, L, E] dtype; either may be NULL. */
int pcad_causal_conv1d_silu(const void* x, int64_t ldx, const float* w_fwd, const float* b_fwd,
                            const float* w_rev, const float* b_rev, void* y_fwd, void* y_rev,
                            int S, int L, int E, int dtype, pcad_stream stream);

/* causal_conv1d_fn(x, weight, bias, activation="silu") of ONE direction, token-major (what "untied_directions" runs per direction):
 *   reverse 0: y[t] = silu(b + sum_k w[k] x[t-3+k]) (causal);  1: y[t] = silu(b + sum_k w[k] x[t+3-k]) (anti-causal: the causal conv of
 *   the flipped strand, flipped back), per output in pcad_causal_conv1d_silu's arithmetic order (same taps, same x: same bits).
 *   x [S, L, ldx >= E] / y [S, L, ldy >= E] dtype, plain rows, or - x_blocked / y_blocked - the BLOCKED layout of pcad_conv_xproj_bidir
 *   below over the S * L rows (rows8 = S * L rounded up to 8; the ld is ignored; E * elem a multiple of 128 bytes);
 *   w fp32 [E, 4], b fp32 [E]; x, y, w 16-byte aligned; E, ldx, ldy multiples of 16 bytes. */
int pcad_causal_conv1d_silu_dir(const void* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy,
                                int S, int L, int E, int reverse, int x_blocked, int y_blocked, int dtype, pcad_stream stream);

/* The form the engine runs for the head of mamba_inner_fn — causal_conv1d_fn(x, w, b, "silu") of BOTH directions fused with
 * BOTH `x_dbl = x_proj(conv_out)` GEMMs, x read once (one kernel instead of causal_conv1d_fwd x2 + cuBLAS x2):
 *   x        [rows8, E] dtype in the BLOCKED layout: byte offset of (row r, byte cb of the row) =
 *            (((r >> 3) * (E*esz/128) + (cb >> 7)) << 10) + ((r & 7) << 7) + (cb & 127); rows8 = S*L rounded up to 8;
 *            E*esz a multiple of 128 bytes; (S*L + 16) * E * esz < 2^32
 *   w_*, b_* fp32 [E, 4] / [E] conv taps and bias per direction (fwd: causal, rev: anti-causal on the same rows)
 *   Rp       dt_rank padded: 64 (dt_rank R <= 64: every PlantCaduceus size, PlantCAD2 Small / Medium) or 96 (R in 65..96:
 *            PlantCAD2 Large)
 *   Wx_*     [Rp + 32, E] dtype: x_proj.weight packed as rows [0, R) = dt rows, zero rows [R, Rp), rows [Rp, Rp + 16) = B,
 *            [Rp + 16, Rp + 32) = C
 *   scratch  device buffer of pcad_conv_xproj_scratch_bytes(E, dtype) bytes (packed taps; written by this call)
 *   xc_*     [rows8, E] dtype, blocked: silu(conv) per direction
 *   dtl_*    [S*L, Rp] dtype: x_dbl[:, :R] zero-padded to Rp;   bc_* fp32 [S*L, 32] = B_t | C_t rounded to dtype */
size_t pcad_conv_xproj_scratch_bytes(int E, int dtype);
int pcad_conv_xproj_bidir(const void* x, const float* w_fwd, const float* b_fwd, const float* w_rev, const float* b_rev,
                          const void* Wx_fwd, const void* Wx_rev, void* scratch,
                          void* xc_fwd, void* dtl_fwd, float* bc_fwd, void* xc_rev, void* dtl_rev, float* bc_rev,
                          int S, int L, int E, int Rp, int dtype, pcad_stream stream);

/* pcad_conv_xproj_bidir with the arguments only the engine passes (csrc/convx.hip launch_convx), for operator-level tests of the forms
 * a small pcad_forward call runs.  x, w_*, b_*, xc_*, bc_*, Rp as above; every tensor 16-byte aligned.
 *   part_ws    NULL, or a device buffer of pcad_conv_xproj_split_scratch_bytes(S, L, E, dtype, Rp, policy_S) bytes (16-byte aligned):
 *              when the launch shape asks for it ("scan_segments" above: at most 64 row tiles of 128 rows) ks blocks per row tile each walk
 *              1 / ks of the channels, write their partial x_dbl there, and a second kernel adds the partials in index order.  xc is
 *              not affected (the conv is not split).  0 bytes: this shape is not split, and part_ws is ignored.
 *   policy_S   the strand count the K-split factor is chosen for (0: S) - the engine passes the strands of the whole pcad_forward call,
 *              so that a chunk of it runs the form the call runs; the scratch is sized for the S strands of the launch
 *   dtl_split  (fp32 only) dtl_* is written as bf16 [S*L, 2 Rp] = [hi | lo], hi = bf16(v), lo = bf16(v - hi): the operand of the scan's
 *              split dt_proj (pcad_selective_scan_engine dt_split)
 *   w_split    (fp32 only) x_proj runs as three bf16 MFMA products per fp32 product (hi.hi, lo.hi, hi.lo of "f32_gemm_split").  Wx_* is
 *              still given as fp32 [Rp + 32, E]; the entry packs each into its bf16 [Rp + 32, 2E] form (per 32 channels [hi (32) | lo (32)])
 *              inside `scratch`, as pcad_gemm_nt_split packs its operands
 *   scratch    256-byte aligned, scratch_bytes >= pcad_conv_xproj_scratch_bytes(E, dtype) rounded up to 256, plus - w_split -
 *              2 * (Rp + 32) * 2 E * 2 bytes; else PCAD_ERR_WORKSPACE (also for a part_ws that is too small) */
size_t pcad_conv_xproj_split_scratch_bytes(int S, int L, int E, int dtype, int Rp, int policy_S);
int pcad_conv_xproj_bidir_engine(const void* x, const float* w_fwd, const float* b_fwd, const float* w_rev, const float* b_rev,
                                 const void* Wx_fwd, const void* Wx_rev, void* scratch, size_t scratch_bytes, void* xc_fwd, void* dtl_fwd,
                                 float* bc_fwd, void* xc_rev, void* dtl_rev, float* bc_rev, void* part_ws, size_t part_ws_bytes,
                                 int policy_S, int dtl_split, int w_split, int S, int L, int E, int Rp, int dtype, pcad_stream stream);

/* selective_scan_fn(u, delta, A, B, C, D, z, delta_bias, delta_softplus=True), token-major:
 *   u, delta [S, L, E] dtype; z [S, L, ldz>=E] dtype or NULL; bc fp32 [S*L, 32] = B_t (16) | C_t (16) per token;
 *   A fp32 [E, 16] (negative real, NOT pre-scaled); Dskip, delta_bias fp32 [E];
 *   reverse != 0 walks t = L-1..0;  accumulate: 0 y = out;  1 y = round(out) + y (bi-directional "add" strategy: each
 *   direction gated and rounded, as the reference's two Mamba calls are);  2 y = (y + out_ungated) * silu(z), z required
 *   (the sum of both directions gated once - what the engine runs).  y [S, L, E] dtype. */
int pcad_selective_scan(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc,
                        const float* A, const float* Dskip, const float* delta_bias,
                        void* y, int S, int L, int E, int reverse, int accumulate,
                        int dtype, pcad_stream stream);

/* The form the engine runs — mamba_inner_fn's `delta = dt_proj.weight @ x_dbl[:, :R]` fused into the scan:
 *   delta[t, c] = round_dtype(sum_k dt_low[t, k] * Wdt[c, k]) computed on MFMA inside the kernel (never stored);
 *   dt_low [S*L, lddt>=Rp] dtype and Wdt [E, Rp] dtype, Rp % 64 == 0 with K zero-padded past dt_rank. */
int pcad_selective_scan_dtproj(const void* u, const void* dt_low, int64_t lddt, const void* Wdt, int Rp,
                               const void* z, int64_t ldz, const float* bc,
                               const float* A, const float* Dskip, const float* delta_bias,
                               void* y, int S, int L, int E, int reverse, int accumulate,
                               int dtype, pcad_stream stream);

/* pcad_selective_scan_dtproj in the layouts and with the arguments the engine passes (csrc/scan.hip launch_scan), for operator-level
 * tests of the instantiations and launch forms a pcad_forward call runs.  Fused dt_proj only.
 *   u, y       [rows8, E] dtype in the BLOCKED layout of pcad_conv_xproj_bidir over the S * L rows (rows8 = S * L rounded up to 8;
 *              E * elem a multiple of 128 bytes); z the same, or NULL (ungated).  With L % 8 == 0 (and, bf16, Rp 64 or 96) the
 *              instantiations with compile-time layouts run, otherwise the run-time-layout ones.  Padding rows are never written.
 *   dt_low     [S*L, lddt >= Rp] dtype, Wdt [E, Rp] dtype as in pcad_selective_scan_dtproj;  dt_split (fp32 only, Rp <= 96): both are
 *              bf16 [hi | lo] tensors, dt_low [S*L, lddt >= 2 Rp] and Wdt [E, 2 Rp], and dt_proj runs as three bf16 MFMA products
 *   A2, a_scale  the base-2 decay rate is A2 * a_scale: (A * log2(e), 1) as the engine stores it, or (A, log2(e))
 *   accumulate as in pcad_selective_scan; the prior content of y is the other direction's output
 *   seg_ws     NULL, or a device buffer of pcad_scan_segment_scratch_bytes(S, L, E, policy_S) bytes (16-byte aligned; too small:
 *              PCAD_ERR_WORKSPACE): when the launch shape asks for it ("scan_segments" above) every strand is cut into segments that run
 *              as separate workgroups - a pass from zero states, the carry h0[g] = exp2(A2 a_scale sum delta) (.) h0[g-1] + h_end[g-1],
 *              then the real pass.  Taken by the four launches the engine issues (forward accumulate 0; reverse with z, any accumulate);
 *              other launches, and shapes whose size query returns 0, run the plain walk.
 *   policy_S   the strand count the segment policy is evaluated for (0: S), as in pcad_conv_xproj_bidir_engine
 *   walk_len   0 or >= L: the whole strand; else only the first walk_len steps of the walk run (forward rows [0, walk_len), reverse rows
 *              [L - walk_len, L)) and the other rows of y are not written ("last_layer_shortcut").  Must be a multiple of 8.  Ignored
 *              when the walk is cut into segments.
 *   ysplit     NULL, or bf16 [rows8, 2E] blocked = [hi | lo] of the output, hi = bf16(y), lo = bf16(y - hi), written INSTEAD of y
 *              (out_proj's operand under "f32_gemm_split"): fp32, L % 8 == 0, z given, reverse with accumulate 1 or 2, whole walk, not
 *              segmented; anything else is PCAD_ERR_INVALID
 * PCAD_ERR_INVALID: whatever launch_scan rejects (shape / layout / form), walk_len % 8 != 0, misaligned tensors. */
size_t pcad_scan_segment_scratch_bytes(int S, int L, int E, int policy_S);
int pcad_selective_scan_engine(const void* u, const void* dt_low, int64_t lddt, const void* Wdt, int Rp, const void* z, const float* bc,
                               const float* A2, float a_scale, const float* Dskip, const float* delta_bias, void* y, void* ysplit,
                               void* seg_ws, size_t seg_ws_bytes, int policy_S, int walk_len, int dt_split, int S, int L, int E,
                               int reverse, int accumulate, int dtype, pcad_stream stream);

/* The PAIR walk ("scan_segments" above; csrc/scan.hip launch_scan_pair): both directions of a layer in one launch, half a strand each.
 * Per direction (*_fwd walks left to right, *_rev right to left on the same rows): u blocked, dt_low [S*L, lddt], Wdt [E, Rp], bc, A2
 * (already scaled by log2(e)), Dskip, delta_bias as in pcad_selective_scan_engine; z (required) and y blocked; L % 64 == 0; bf16: Rp 64
 * or 96.
 *   phases     bit 0: the first halves - forward rows [0, L/2) and reverse rows [L/2, L) from zero states, written ungated (gate_each:
 *              each gated and rounded), end states kept in ws;  bit 1: the second halves from those states, each adding what the OTHER
 *              direction's first half left in y: gate_each 0: y = (y + out) * silu(z);  1: y = round(out * silu(z)) + y - the same two
 *              rounded addends as two plain accumulate 1 launches.  3: both, in that order (the engine issues 1, then 2).
 *   ws         pcad_scan_pair_scratch_bytes(S, E) bytes, 16-byte aligned (too small: PCAD_ERR_WORKSPACE); carries the states from
 *              phase 1 to phase 2
 *   ysplit / dt_split  (fp32 only) as in pcad_selective_scan_engine; ysplit is written by phase 2 instead of y */
size_t pcad_scan_pair_scratch_bytes(int S, int E);
int pcad_selective_scan_pair(const void* u_fwd, const void* dt_low_fwd, const void* Wdt_fwd, const float* bc_fwd, const float* A2_fwd,
                             const float* Dskip_fwd, const float* delta_bias_fwd, const void* u_rev, const void* dt_low_rev,
                             const void* Wdt_rev, const float* bc_rev, const float* A2_rev, const float* Dskip_rev,
                             const float* delta_bias_rev, const void* z, int64_t lddt, int Rp, void* y, void* ysplit, void* ws,
                             size_t ws_bytes, int S, int L, int E, int gate_each, int phases, int dt_split, int dtype, pcad_stream stream);

/* F.linear(a, w): C[M,N] = A[M,K] . W[N,K]^T on MFMA.  lda/ldw/ldc in elements; K % (128/sizeof(elem)) == 0,
 * lda, ldw multiples of 16 bytes.  out_dtype: PCAD_F32 or `dtype`. */
int pcad_gemm_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc,
                 int64_t M, int N, int K, int dtype, int out_dtype, pcad_stream stream);

/* F.linear(a, w) of fp32 tensors on the bf16 matrix pipes - the form the fp32 model's in_proj / out_proj take with
 * pcad_set_option("f32_gemm_split", 1): each operand is carried as two bf16 values (hi = bf16(v), lo = bf16(v - hi): 16 mantissa
 * bits) and C = A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T is ONE bf16 GEMM of 3 K / 64 K-tiles whose cursor wraps around operands
 * stored once as [hi | lo] (A: hi, lo, hi;  W: hi, hi, lo), fp32 accumulation in that order, fp32 result (3/16 of the fp32-MFMA
 * cost per flop; operand error 2^-17, dropped term 2^-16 relative).
 *   A [M, K] (lda), W [N, K] (ldw), C [M, N] (ldc) fp32, K % 64 == 0; scratch: device buffer of
 *   pcad_gemm_nt_split_scratch_bytes(M, N, K) bytes (the split operands; the engine keeps the weights' split copy in its arena). */
size_t pcad_gemm_nt_split_scratch_bytes(int64_t M, int N, int K);
int pcad_gemm_nt_split(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int N, int K,
                       void* scratch, size_t scratch_bytes, pcad_stream stream);

/* out_proj of the "norm_fold" layer form as one operator (MFMA, 256 x 256 tiles only: M % 256 == 0, N % 256 == 0, K * elem a
 * multiple of 128 bytes, every tensor < 4 GiB):
 *   res [M, N] fp32 += A [M, K] . W [N, K]^T   (in place; the mixer output added to the fp32 residual stream).  res is in the
 *                       kernel's FRAGMENT layout - the order in which the GEMM's lanes hold a 256 x 256 tile, so that the
 *                       read-modify-write moves whole cache lines: element (row, col) lives at float offset
 *                         ((((tile * 4 + wave) * 8 + i) * 2 + jg) * 4 + k) * 256 + (16 lg + li) * 4 + r     with
 *                         tile = (row / 256) * (N / 256) + col / 256, wave = 2 ((row / 128) % 2) + (col / 128) % 2,
 *                         i = (row / 16) % 8, li = row % 16, jg = (col / 64) % 2, lg = (col / 16) % 4, k = (col / 4) % 4, r = col % 4
 *                       (csrc/common.hpp res_frag_off; plantcaduceus_amd.ops.to_res_fragment / from_res_fragment)
 *   C   [M, N] dtype  = round(res)              (plain rows: the next in_proj's operand)
 *   ssq [M, N / 128]  = per-row sums of squares of the updated res over each 128-column slab (deterministic partials whose
 *                       sum / N gives the next block's RMSNorm statistic)
 * Replaces: out_proj (F.linear) + the residual add of rms_norm_fn(..., prenorm=True, residual_in_fp32=True). */
int pcad_gemm_nt_residual(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, float* res, float* ssq,
                          int64_t M, int N, int K, int dtype, pcad_stream stream);

/* Engine forms of the GEMMs: the four launches above with the operands and arguments the engine passes (csrc/forward.hip), for
 * operator-level tests of the kernels and epilogues a pcad_forward call runs (tests/test_gpu_gemm_forms.py).  The entries pack nothing:
 * every tensor is taken as the caller built it.  Common to all four:
 *   A [M, K] (lda), W [N, K] (ldw) dtype, K * elem a multiple of 128 bytes, rows and base addresses 16-byte aligned
 *   a_blocked  A is in the BLOCKED layout of pcad_conv_xproj_bidir with rows of lda elements (lda * elem a multiple of 128 bytes): the
 *              byte at offset cb of row r lives at ((r / 8) * pieces + cb / 128) * 1024 + (r % 8) * 128 + cb % 128, pieces =
 *              lda * elem / 128; the buffer holds M rounded up to 8 rows (csrc/common.hpp blocked_off; plantcaduceus_amd.ops.to_blocked)
 *   ksplit     0, or the wrap-around K cursor of pcad_gemm_nt_split: A and W are bf16 [hi | lo] tensors of 2 Ko columns, K = 3 Ko,
 *              ksplit = Ko / 64, the result is fp32 = A_hi W_hi^T + A_lo W_hi^T + A_hi W_lo^T accumulated in that order.  dtype PCAD_BF16
 *              with out_dtype PCAD_F32 only, and only in pcad_gemm_nt_engine and pcad_gemm_nt_two
 * PCAD_ERR_INVALID: null / misaligned tensors, rows shorter than the operand, and whatever the launcher of the form rejects; nothing
 * is launched then.
 *
 * pcad_gemm_nt_engine (launch_gemm_nt: out_proj, and in_proj without "xzsplit"): C [M, N] (ldc) out_dtype, PCAD_F32 or dtype.  M >= 2048
 *   and N >= 512 with N % 16 == 0 run a 256 x 256 kernel (whole tiles: four waves, else eight), everything else the 256 x 128 kernel.
 * pcad_gemm_nt_xproj (launch_gemm_nt_split: x_proj wherever the fused conv + x_proj kernel is off): columns [0, nsplit) -> C [M, nsplit]
 *   (ldc) dtype, columns [nsplit, N) -> C2 [M, N - nsplit] (ldc2) fp32 holding values rounded to dtype; nsplit and N - nsplit multiples
 *   of 16.  Always the 256 x 128 kernel.
 * pcad_gemm_nt_two (launch_gemm_nt_two: in_proj): columns [0, nsplit) -> C1 [M, nsplit], [nsplit, N) -> C2 [M, N - nsplit], contiguous
 *   rows, or - out_blocked - both in the blocked layout (nsplit * elem and (N - nsplit) * elem multiples of 128 bytes; buffers of M rounded
 *   up to 8 rows, padding rows never written).  Always a 256 x 256 kernel: four waves for whole tiles with nsplit % 64 == 0, else eight.
 *   rscale     NULL, or fp32 [M]: row m of the result is multiplied by rscale[m] before it is rounded (the "norm_fold" in_proj, rscale =
 *              the row's rstd); whole 256 x 256 tiles and out_dtype == dtype only
 *   out_dtype  dtype, or PCAD_F32 with dtype PCAD_BF16 (the split-bf16 in_proj of the fp32 model, with ksplit)
 *   a_blocked  must be 0: the form has no blocked A
 * pcad_gemm_nt_residual_engine: pcad_gemm_nt_residual with a_blocked (the mixer output y as the scan leaves it). */
int pcad_gemm_nt_engine(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int N, int K, int a_blocked,
                        int ksplit, int dtype, int out_dtype, pcad_stream stream);
int pcad_gemm_nt_xproj(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, float* C2, int64_t ldc2, int nsplit,
                       int64_t M, int N, int K, int a_blocked, int ksplit, int dtype, pcad_stream stream);
int pcad_gemm_nt_two(const void* A, int64_t lda, const void* W, int64_t ldw, void* C1, void* C2, int nsplit, const float* rscale, int64_t M,
                     int N, int K, int a_blocked, int out_blocked, int ksplit, int dtype, int out_dtype, pcad_stream stream);
int pcad_gemm_nt_residual_engine(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, float* res, float* ssq, int64_t M, int N,
                                 int K, int a_blocked, int ksplit, int dtype, pcad_stream stream);

/* Rows of a [2B * L, E] activation tensor (plain rows) that a forward evaluated at positions p_0..p_{P-1} consumes after the
 * last mixer: strand b row p_q and strand B + b row L - 1 - p_q  ->  out [(strand * P + q), E].  positions: HOST int32 [P],
 * P <= PCAD_MAX_POSITIONS.  (The last-layer shortcut of pcad_forward; reference callers read one position:
 * src/zero_shot_score.py:117, src/train_XGBoost.py:105.) */
int pcad_gather_rows(const void* src, void* out, int B, int L, int E, const int32_t* positions, int P, int dtype,
                     pcad_stream stream);

/* The row kernel of pcad_forward_layers as one operator.  src: plain rows [2B * L, D] (assembled == 0: strand b row p_q and strand
 * B + b row L - 1 - p_q are read), or [B, P, 2D] rows already in hidden_states' layout (assembled != 0: pcad_final_head's
 * hidden_out; the positions only give P).  out: dtype [B, P, 2D] (average == 0) or fp32 [B, P, D] = (fwd + rc) * 0.5f
 * (average != 0).  positions (HOST int32 [P]) or pos_per_window (DEVICE int32 [B, P]; clamped and reported through `status`,
 * which may be NULL), exactly one, 1 <= P <= PCAD_MAX_POSITIONS.  D % 8 == 0; src and out 16-byte aligned.
 * Replaces: hidden_states[k][:, positions, :] (indexing + the flips of RCPSWrapper) and extract_embeddings' strand averaging. */
int pcad_layer_rows(const void* src, void* out, int B, int L, int D, const int32_t* positions, int P,
                    const int32_t* pos_per_window, int assembled, int average, int32_t* status, int dtype, pcad_stream stream);

/* The forward's last kernel as one operator: res + h -> norm_f -> RC re-assembly of hidden_states[-1] -> tied RCPS LM head, at
 * the shared positions (HOST int32 [P], P = 0: all L) or one position per window (pos_per_seq, DEVICE int32 [B]; then
 * positions must be NULL / P = 0).  h / res: [2B * L, D] (h: dtype, res: res_dtype); h_compact != 0: h holds only the evaluated
 * rows as pcad_gather_rows orders them; res_fragment_layout != 0: res (fp32) is in the fragment layout of pcad_gemm_nt_residual.  emb_f32: [vocab, D] fp32 (the dtype-rounded tied embedding / LM-head weight);
 * hidden_out [B, Q, 2D] dtype and logits_out [B, Q, vocab] fp32, either may be NULL.  ids (DEVICE [B, L]) and status (DEVICE
 * word) may be NULL: input validation as in pcad_set_status_buffer.
 * Replaces: norm_f (rms_norm_fn) x2, the flips / cats of RCPSWrapper's output and RCPSLMHead. */
int pcad_final_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                    void* hidden_out, float* logits_out, int B, int L, int D, float eps, const int32_t* positions, int P,
                    const int32_t* pos_per_seq, int h_compact, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                    int res_fragment_layout, pcad_stream stream);

/* The pooled head of pcad_forward_pooled as one operator, with pcad_final_head's inputs: h / res [2B * L, D] (h: dtype, res:
 * res_dtype; res_fragment_layout != 0: fp32 res in pcad_gemm_nt_residual's fragment layout, D % 256 == 0, 2 B L % 256 == 0),
 * norm_weight fp32 [D]; score_w, num_labels, pooled_out, logits_out as in pcad_forward_pooled, except that either output may be NULL
 * (not both; score_w may be NULL when logits_out is); ids / status as in pcad_final_head.  scratch: device buffer of
 * pcad_pooled_head_scratch_bytes(B, L, D, pooling) bytes, 256-byte aligned (the per-segment partials). */
size_t pcad_pooled_head_scratch_bytes(int B, int L, int D, int pooling);
int pcad_pooled_head(const void* h, const void* res, const float* norm_weight, const float* score_w, int num_labels,
                     float* pooled_out, float* logits_out, int B, int L, int D, float eps, int pooling, const int32_t* ids,
                     int32_t* status, int dtype, int res_dtype, int res_fragment_layout, void* scratch, size_t scratch_bytes,
                     pcad_stream stream);

/* The loss head of pcad_forward_loss as one operator, with pcad_final_head's inputs (all L positions; no positions / h_compact):
 * labels, loss_weights, ignore_index, sums_out, nll_out, logits_out as in pcad_forward_loss.  scratch: device buffer of
 * pcad_loss_head_scratch_bytes(B, L) bytes, 256-byte aligned (the per-segment partials). */
size_t pcad_loss_head_scratch_bytes(int B, int L);
int pcad_loss_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                   const int32_t* labels, const float* loss_weights, int ignore_index, float* sums_out, float* nll_out,
                   float* logits_out, int B, int L, int D, float eps, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                   int res_fragment_layout, void* scratch, size_t scratch_bytes, pcad_stream stream);

/* The probability head of pcad_forward_probs as one operator, with pcad_final_head's inputs (h_compact and res_fragment_layout
 * included; no hidden_out): cols (HOST int32 [4], each inside [0, PCAD_MAX_VOCAB)), probs_out [B, Q, 4] (16-byte aligned) and
 * logits_out [B, Q, vocab] (bit-equal to pcad_final_head's) as in pcad_forward_probs, either may be NULL (not both).  Positions:
 * positions (HOST int32 [P]; P == 0: all L) or pos_per_window (DEVICE int32 [B, P], 1 <= P <= PCAD_MAX_POSITIONS; clamped and
 * reported through `status`), never both; h_compact needs the shared list.
 * Replaces: pcad_final_head's logits + the host's column selection and torch.softmax. */
int pcad_probs_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                    const int32_t* cols, float* probs_out, float* logits_out, int B, int L, int D, float eps, const int32_t* positions,
                    int P, const int32_t* pos_per_window, int h_compact, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                    int res_fragment_layout, pcad_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PCAD_H */
