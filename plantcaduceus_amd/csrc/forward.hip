// The forward of libpcad.so: one request per entry point, one plan per call, the per-layer launch sequence as named phases.
// Forward = CaduceusForMaskedLM.forward restated per SURVEY.md Appendix A ("2B-strand form"): the RCPS
// network equals a plain bi-directional Mamba stack applied to [ids ; reverse_complement(ids)], so no flip
// or concatenation kernel exists here; the tied in_proj / out_proj run once per strand-layer.
#include "pcad_internal.hpp"
using namespace pcad;

namespace {
// ---- the request: each pcad_forward* entry fills it by field name after validating its own arguments ---------------------------
enum class Head { lm, pooled, loss, probs, layers };
struct ForwardRequest {
    Head head = Head::lm;
    const int32_t* ids = nullptr; int B = 0, L = 0;
    void* workspace = nullptr; size_t ws_bytes = 0; pcad_stream stream = nullptr;
    // evaluated positions: neither (all L), a shared HOST list, or a DEVICE list [B, Pw] per window (pcad_forward_at: Pw == 1)
    const int32_t* positions = nullptr; int P = 0;
    const int32_t* pos_per_window = nullptr; int Pw = 0;
    void* all_hidden = nullptr;        // pcad_forward_all_hidden: [n_layer, B, L, 2D]
    void* hidden_out = nullptr; float* logits_out = nullptr;       // Head::lm
    struct {       // pcad_forward_pooled: the pooled classification head in place of the LM head (pool.hip)
        int pooling, num_labels;
        const float* score_w; float *pooled_out, *logits_out;
    } pool = {};
    struct {       // pcad_forward_loss: the masked-LM loss head in place of the LM head (loss.hip)
        const int32_t* labels; const float* loss_weights; int ignore_index;
        float *sums_out, *nll_out, *logits_out;
    } loss = {};
    struct {       // pcad_forward_probs: the nucleotide-probability head in place of the LM head (probs.hip)
        ProbCols cols; float *probs_out, *logits_out;
    } probs = {};
    struct {       // pcad_forward_layers: chosen levels of hidden_states at the evaluated positions (layers.hip) in place of the LM head's outputs
        const int32_t* layers;         // host [NL], strictly increasing levels in [0, n_layer], or nullptr: all n_layer + 1
        int NL;
        bool inter, average;           // inter: a level below n_layer is requested: the unfolded walk of pcad_forward_all_hidden, up to block `top`
        int top;                       // the highest requested level
        void* out;                     // [NL, B, P, 2D] model dtype, or (average) [NL, B, P, D] fp32
    } lay = {};
};

// ---- the plan: what is fixed for the call, decided once before the first launch (no HIP call, no allocation) -------------------
struct ForwardPlan {
    int chunk, nchunks;     // windows per pass through the layer stack (api.hip chunk_for); passes
    bool fold, sp, untied;  // norm-folded layer form (every chunk folds or none does); split-bf16 GEMMs; per-direction in_proj / out_proj
    bool lay_inter, strict; // pcad_forward_layers with a level below n_layer; each direction's own out_proj, rounded, summed and rounded
    int depth;              // blocks to run: n_layer, or - pcad_forward_layers whose highest level lies below it - that level (0: none)
    int walk_len;           // last-layer shortcut: steps of the walks of the last EXECUTED block, depth - 1 (0: the full block)
    SmallForms forms;       // from the strands of the whole call; the same function sizes their scratch (api.hip carve_workspace)
    bool tab0;              // layer 0's in_proj of the folded form as a table look-up
    int Q;                  // evaluated positions per window
};

ForwardPlan plan_forward(const pcad_engine* e, const ForwardRequest& rq, const Positions& pos) {
    const int B = rq.B, L = rq.L, D = e->D, E = e->E, P = rq.P;
    ForwardPlan pl;
    pl.Q = rq.pos_per_window ? rq.Pw : (P ? P : L);
    pl.chunk = chunk_for(e, B, L);
    pl.nchunks = (B + pl.chunk - 1) / pl.chunk;
    // Norm-folded layer form (pcad_set_option("norm_fold", 0) restores the reference's order).  The reference's block is
    //     res = h + res (fp32);  u = round(res * rstd(res) * w_norm);  xz = round(u . W_in^T);  ...;  h = round(y . W_out^T)
    // (rms_norm_fn(..., prenorm=True, residual_in_fp32=True)).  Folded: out_proj's epilogue does
    // res += y . W_out^T in fp32 (the accumulators start as the residual values), writes round(res) and per-row partial sums of
    // squares; in_proj runs on round(res) with W_in . diag(w_norm) (folded at bind time) and multiplies by rstd[row] before it
    // rounds.  The add + norm launch and its read of h / write of u disappear; what moves is rounding: h is not rounded before it
    // is added, and the operand of in_proj is round(res) instead of round(res * rstd * w).  While a chunk runs in this form its
    // fp32 residual tensor is kept in the GEMM's fragment layout (common.hpp res_frag_off) so that the epilogue's
    // read-modify-write moves whole lines; only the embedding kernel, the folded out_proj and the head kernel touch it.
    // Default: on for the bf16 model only.  Accumulating the K products onto the (large) residual value instead of onto zero costs
    // the fp32 model precision it can see - hidden states 2.2e-5 of max after 32 layers against 1.3e-6 with the separate add
    // (profiles/r04h_gpu_tests.log; still inside north_star's 1e-4) - while under bf16 storage the difference is far below the
    // rounding noise (probabilities 8.1e-3 vs 8.6e-3 from the reference-order emulation).
    // Used when every GEMM of the chunk runs on the 4-wave kernel (whole 256 x 256 tiles: token-rows % 256 == 0; a d_model that is
    // not a multiple of 256 - l20's 384 - is padded to the next one with zero out_proj weight rows and zero residual columns) and the
    // residual stream is fp32; never for pcad_forward_all_hidden (hidden_states[i] are the mixer outputs h, which the folded form
    // never materialises).
    // Decided ONCE per forward - every chunk folds or none does - so that a result never depends on how the batch was cut
    // into chunks (an uneven split of odd-length windows could otherwise give one chunk whole 256-row tiles and another not).
    // pcad_forward_layers with a level below n_layer: hidden_states[i] are the mixer outputs, so the walk is pcad_forward_all_hidden's
    pl.lay_inter = rq.head == Head::layers && rq.lay.inter;
    pl.fold = fold_wanted(e) && e->fold_packed && !rq.all_hidden && !pl.lay_inter;
    for (int ck = 0; ck < pl.nchunks && pl.fold; ++ck) {
        const int Bc = (B - ck * pl.chunk) < pl.chunk ? (B - ck * pl.chunk) : pl.chunk;
        pl.fold = gemm_fold_shapes_ok((int64_t)2 * Bc * L, D, E, e->cfg.dtype);
    }
    // Untied directions ("untied_directions": per-direction LoRA deltas, bidirectional_weight_tie = False).  mamba_fwd and mamba_rev
    // no longer share in_proj / out_proj, so a layer is the strict reference order ("reference_order" 2) with per-direction operands:
    // one add + norm; in_proj twice (x_f, z_f / x_r, z_r); per direction conv + SiLU on its own x (conv.hip launch_conv_dir), x_proj
    // as a GEMM, the scan gated with its own z; each direction's own out_proj, each rounded, summed and rounded.  The fused conv +
    // x_proj kernel, the pair walks and the scan-written out_proj operand all read ONE x / z for both directions and are off; the
    // segmented scan and the last-layer shortcut take z per launch and stay on.
    pl.untied = e->untied && e->untied_packed;
    // Split-bf16 GEMMs of the fp32 model ("f32_gemm_split"; pack.hip): in_proj and out_proj - 3/4 of the fp32 model's time on the
    // fp32 MFMA instructions - run as bf16 GEMMs of 3 K / 64 K-tiles on [hi | lo] x [hi | lo] operands (wrap-around K cursor: hi.hi,
    // lo.hi, hi.lo; gemm.hip) with an fp32 result: operand error 2^-17, measured 4e-7 of the logits' range after 32 layers (fp32 MFMA:
    // 1e-6 from summation order alone).
    pl.sp = split_wanted(e) && e->split_packed;
    // strict reference order ("reference_order" 2; never with norm_fold): the reverse direction's gated output goes to its own
    // tensor (xc[0]: the forward scan, its only reader, has run) and each direction gets its own tied out_proj
    pl.strict = (e->ref_order == 2 || pl.untied) && !pl.fold;
    // Truncated walk (pcad_forward_layers whose highest requested level K lies below n_layer): nothing above block K - 1 is read, so
    // the walk stops there - no norm_f, no head (the token ids are checked by ids_check_kernel instead).  K == 0 runs no block.
    pl.forms = small_forms(e, B, L);
    pl.depth = pl.lay_inter && rq.lay.top < e->nl ? rq.lay.top : e->nl;
    const bool truncated = pl.depth < e->nl;
    // Last-layer shortcut (reference callers read ONE position: src/zero_shot_score.py:117,
    // src/train_XGBoost.py:105): with a shared list of P evaluated positions only rows p_q of the forward strands and L - 1 - p_q of
    // the reverse-complement strands of the LAST mixer's output are consumed.  The left-to-right scan stops after the furthest of
    // them, the right-to-left scan likewise (walk_len steps each), and the tied out_proj runs on the 2B * P gathered rows.  Same
    // arithmetic on the consumed rows (sequential walks, row-independent GEMM): results are bit-identical to the full layer.
    // In a truncated walk the shortened block is K - 1, the last one executed, and level K is gathered from its compact rows.  That
    // block must compute what pcad_forward_all_hidden computes on it, whose rows the level is bit-equal to: where that is a pair walk
    // (it rounds the gate-once sum elsewhere than plain walks do) the block stays whole.
    pl.walk_len = 0;
    if (e->shortcut && P > 0 && !rq.pos_per_window && !rq.all_hidden && (int64_t)P * E <= (int64_t)L * D &&
        (truncated ? pl.depth > 0 && !(pl.forms.pair && !pl.strict) : !pl.lay_inter)) {
        int pmin = pos.p[0], pmax = pos.p[0];
        for (int i = 1; i < P; ++i) { pmin = pos.p[i] < pmin ? pos.p[i] : pmin; pmax = pos.p[i] > pmax ? pos.p[i] : pmax; }
        const int need = (pmax + 1 > L - pmin) ? pmax + 1 : L - pmin;      // forward strands need row pmax, rc strands row L - 1 - pmin
        pl.walk_len = (need + 7) / 8 * 8;                                // whole 8-step groups (two prefetch chunks)
        if (pl.walk_len > L) pl.walk_len = L;
    }
    static const bool tab0 = dev_env("PCAD_NO_TAB0") == nullptr;     // layer 0's in_proj as a table look-up (in_proj_conv); PCAD_DEV=1 A/B switch
    pl.tab0 = tab0;
    return pl;
}

// One chunk = up to `chunk` windows (2x strands) walking the whole layer stack, chunks one after the other, everything on
// the caller's stream.  (Multi-stream schedules were built and measured twice and removed: chunks alternating between two
// streams gain nothing because the big kernels each fill the CUs, +1 %; the add+norm kernels on a side stream beside the other
// chunk's GEMM are zero-sum, in_proj stretches by the norm's duration, -4 %: DESIGN.md §8.)
struct Lane { Workspace w; int b0, Bc; };
// ---- the walk: the phases of one chunk over (engine, request, plan, stream); `c` is the chunk's Lane ----------------------------
struct Walk {
    pcad_engine* const e;
    const ForwardRequest& rq; const ForwardPlan& pl; const Positions& pos; const hipStream_t s;
    const int B, L, P, D, E, N, Rp, XP, dt, rdt;
    const int Dp;           // width of res / u while a chunk runs in the norm-folded form
    const size_t esz; const float eps;
    const int layP;         // pcad_forward_layers: evaluated positions per window
    Walk(pcad_engine* e_, const ForwardRequest& rq_, const ForwardPlan& pl_, const Positions& pos_)
        : e(e_), rq(rq_), pl(pl_), pos(pos_), s((hipStream_t)rq_.stream), B(rq_.B), L(rq_.L), P(rq_.P), D(e_->D), E(e_->E), N(e_->N),
          Rp(e_->Rp), XP(e_->XP), dt(e_->cfg.dtype), rdt(e_->rdt), Dp(fold_padded_width(e_->D)), esz(e_->esz), eps(e_->cfg.eps),
          layP(rq_.head == Head::layers ? pl_.Q : 0) {}
    // ---- predicates: each defined here once; what depends on the chunk's rows or on the layer takes them -----------------------
    // Measurement aid (tools/power_probe.py): every launch of ONE kernel class is issued `debug_repeat` times back to back, so a
    // forward becomes seconds of that kernel - the engine's own instantiation, layouts and launch sizes - while the host samples
    // board power and clocks.  Only launches that are idempotent are repeated (in_proj, conv + x_proj, the forward-direction scan,
    // the reference-order out_proj); outputs are unchanged.
    int reps(int cls) const { return e->rep_class == cls ? e->rep_count : 1; }
    // conv + x_proj of both directions in the fused kernel: its unsigned 32-bit in-tensor offsets bound the chunk's rows
    bool convx_fused(int64_t rows) const { return !pl.untied && e->convx && (rows + 16) * E * (int64_t)esz < ((int64_t)1 << 32); }
    // split-bf16 dt_proj inside the scan ("f32_gemm_split"): the fused conv + x_proj kernel wrote dt_low as bf16 [rows, 3 Rp]
    bool dts(int64_t rows) const { return pl.sp && convx_fused(rows); }
    // the last EXECUTED block (n_layer - 1, or depth - 1 of a truncated walk) with its walks shortened and out_proj on the gathered rows
    bool last_short(int li) const { return pl.walk_len > 0 && li + 1 == pl.depth; }
    bool truncated() const { return pl.depth < e->nl; }
    // "f32_gemm_split": out_proj's [hi | lo] operand is written by the gating (reverse) scan itself where it can (whole walk,
    // unsegmented, L % 8 == 0, one out_proj for both directions), instead of fp32 y + a conversion pass
    bool ys_from_scan(int li) const { return pl.sp && !pl.strict && !last_short(li) && L % 8 == 0 && e->blocked && e->xzsplit && pl.forms.G == 1; }
    // Pair walks (kernels.hpp scan_pair_wanted: few waves per launch - long windows in small batches): both directions in one
    // launch, half a strand each, twice; chosen from the strands of the whole call like the segmented form
    // (never the LAST layer: with a list of positions its walks are shortened plain walks - "last_layer_shortcut" - and the full
    // layer must stay bit-identical to them on the evaluated rows; block depth - 1 of a truncated walk is shortened only where it
    // would not be a pair walk - plan_forward - and otherwise runs pcad_forward_all_hidden's form of that block, pair walk included)
    bool pair(int64_t rows, int li) const { return pl.forms.pair && !pl.strict && li + 1 < e->nl && !last_short(li) && convx_fused(rows) && reps(PCAD_K_SCAN) == 1; }
    void* y_rev(const Lane& c) const { return pl.strict ? c.w.xc[0] : c.w.y; }
    const int32_t* ids_of(const Lane& c) const { return rq.ids + (int64_t)c.b0 * L; }
    const int32_t* ppw_of(const Lane& c) const { return rq.pos_per_window ? rq.pos_per_window + (size_t)c.b0 * rq.Pw : nullptr; }      // its rows of the [B, Pw] list
    // what every head reads of the lane: the last mixer output, the residual stream (folded form: fragment layout) and norm_f
    HeadInput head_in(const Lane& c) const {
        return {.h = c.w.h, .res = c.w.res, .w = e->normf_w, .B = c.Bc, .L = L, .D = D, .eps = eps, .dt = dt, .rdt = rdt, .res_frag = pl.fold ? Dp : 0,
                .ids = ids_of(c), .status = e->status};
    }
    // the evaluated rows of a [2 Bc L, E] mixer tensor -> u (dead since in_proj): the last-layer shortcut's operand
    hipError_t gather_rows(const Lane& c, const void* src) const {
        return launch_gather_rows({.src = src, .out = c.w.u, .B = c.Bc, .L = L, .E = E, .pos = pos, .dt = dt, .blocked = e->blocked}, s);
    }
    // the full-size tied out_proj of one [rows, E] tensor (y, or in the strict order each direction's own): fp32 / bf16 GEMM, or the
    // split-bf16 form (operand conversion unless the scan wrote it + bf16 GEMM with K' = 3E, fp32 result)
    // Also the last-layer shortcut's: src = the n_rows gathered rows, plain (a_blocked false).  d: whose weight (untied form only)
    hipError_t out_proj(const Lane& c, int li, const void* src, int64_t n_rows, void* dst, int d, bool a_blocked) const {
        const LayerWeights& W = e->layers[li];
        const void *Wo = pl.untied && d ? W.W_out_r : W.W_out, *Wo_s = pl.untied && d ? W.W_out_s_r : W.W_out_s;
        if (pl.sp) {
            if (!(ys_from_scan(li) && src == c.w.y))
                if (hipError_t er = launch_split_rows((const float*)src, E, c.w.ys, n_rows, E, a_blocked, a_blocked, s)) return er;
            return launch_gemm_nt({.A = c.w.ys, .lda = 2 * E, .W = Wo_s, .ldw = 2 * E, .M = n_rows, .N = D, .K = 3 * E, .dt = BF16, .a_blocked = a_blocked, .ksplit = E / 64},
                                  {.C = dst, .ldc = D, .out_dt = F32}, s);
        }
        return launch_gemm_nt({.A = src, .lda = E, .W = Wo, .ldw = E, .M = n_rows, .N = D, .K = E, .dt = dt, .a_blocked = a_blocked}, {.C = dst, .ldc = D, .out_dt = dt}, s);
    }
    // in_proj of the chunk's normalised rows u -> x | z: the split-bf16 form (bf16 [hi | lo] operands, fp32 outputs), two blocked
    // tensors, or one plain [rows, 2E] tensor in x.  d: whose weight (untied form only)
    hipError_t in_proj(const Lane& c, const LayerWeights& W, int64_t rows, int d, void* x, void* z) const {
        if (pl.sp)
            return launch_gemm_nt_two({.A = c.w.u, .lda = 2 * D, .W = d ? W.W_in_s_r : W.W_in_s, .ldw = 2 * D, .M = rows, .N = 2 * E, .K = 3 * D, .dt = BF16, .ksplit = D / 64},
                                      {.C1 = x, .C2 = z, .nsplit = E, .out_blocked = true, .out_dt = F32}, s);
        const GemmOperands g{.A = c.w.u, .lda = D, .W = d ? W.W_in_r : W.W_in, .ldw = D, .M = rows, .N = 2 * E, .K = D, .dt = dt};
        if (e->xzsplit) return launch_gemm_nt_two(g, {.C1 = x, .C2 = z, .nsplit = E, .out_blocked = true}, s);
        return launch_gemm_nt(g, {.C = x, .ldc = 2 * E, .out_dt = dt}, s);
    }
    int64_t ldxz() const { return e->xzsplit ? E : 2 * E; }        // elements between the rows of in_proj's x (and of z inside xz)
    // direction d's scan operands (dts: the [hi | lo] dt_proj weight and dt_low rows)
    ScanDirection scan_dir(const Lane& c, const LayerWeights& W, int d, bool dts) const {
        const DirWeights& dw = W.dir[d];
        return {.u = c.w.xc[d], .dt_low = c.w.dtl[d], .Wdt = dts ? dw.Wdt_s : dw.Wdt, .bc = c.w.bc[d], .A2 = dw.A2, .Dskip = dw.Dskip, .dbias = dw.dt_bias};
    }
    int64_t lddt(bool dts) const { return dts ? 2 * Rp : Rp; }
    // what a layer's scans of direction d share (ungated forward walk of the whole strand into y): operands and the engine's layouts
    ScanLaunch scan_of(const Lane& c, const LayerWeights& W, int d, bool dts) const {
        return {.dir = scan_dir(c, W, d, dts), .ldz = ldxz(), .lddt = lddt(dts), .Rp = Rp, .y = c.w.y, .S = 2 * c.Bc, .L = L, .E = E, .dt = dt,
                .uy_blocked = e->blocked, .z_blocked = e->xzsplit, .seg_ws = c.w.seg, .dt_split = dts,
                .policy_S = 2 * B};        // the strands of the whole call: every chunk runs the same form
    }
    int lay_slot(int level) const {        // pcad_forward_layers: slot of `level` in the output, or -1
        if (rq.head != Head::layers) return -1;
        if (!rq.lay.layers) return level;
        for (int i = 0; i < rq.lay.NL; ++i)
            if (rq.lay.layers[i] == level) return i;
        return -1;
    }
    void* lay_dst(int slot, int b0) const {      // indexed by the chunk's first window, as all_hidden is
        return (char*)rq.lay.out + ((size_t)slot * B + b0) * layP * (rq.lay.average ? (size_t)D * 4 : (size_t)2 * D * esz);
    }
    // hidden_states[level] (now in c.w.h as plain rows) -> pcad_forward_all_hidden's tensor / pcad_forward_layers' rows at the
    // evaluated positions, whichever the call asked for
    // compact: c.w.h holds only the [2 Bc, P, D] rows the shortcut's gather + small GEMM left (the shortened block of a truncated walk)
    int emit_level(Lane& c, int level, bool compact = false) const {
        if (rq.all_hidden) {
            char* dst = (char*)rq.all_hidden + ((size_t)level * B * L * 2 * D + (size_t)c.b0 * L * 2 * D) * esz;
            HIP_TRY(launch_assemble_hidden(c.w.h, dst, c.Bc, L, D, dt, s));
        }
        const int slot = lay_slot(level);
        if (slot >= 0)
            HIP_TRY(launch_layer_rows({.src = c.w.h, .out = lay_dst(slot, c.b0), .B = c.Bc, .L = L, .D = D, .dt = dt, .pos = pos, .pos_per_window = ppw_of(c), .P = layP,
                                       .average = rq.lay.average, .compact = compact, .status = e->status}, s));
        return PCAD_OK;
    }
    // A head's scratch goes to the buffers that are dead once the last out_proj has run (everything carved after h: xz, zb, xc,
    // dtl, bc, y, ...), so the forward's workspace size is unchanged: whether `need` bytes fit there (shown: what the message names if not `need`)
    int fits_dead(const Lane& c, size_t need, const char* who, const char* what, size_t shown = 0) const {
        const size_t avail = (size_t)((char*)rq.workspace + c.w.bytes - (char*)c.w.xz);
        if (need > avail) return fail(PCAD_ERR_WORKSPACE, "%s: the %s (%zu bytes) do not fit the dead buffers (%zu)", who, what, shown ? shown : need, avail);
        return PCAD_OK;
    }
    int level0(Lane& c) const {        // hidden_states[0] = RCPSEmbedding output, where asked for (never in the folded form): before block 0, if any
        if (pl.fold || !(rq.all_hidden || lay_slot(0) >= 0)) return PCAD_OK;
        HIP_TRY(launch_embed_only(ids_of(c), e->emb, e->comp, c.w.h, c.Bc, L, D, dt, s));
        return emit_level(c, 0);
    }
    int add_norm(Lane& c, int li) const {        // residual add + norm (layer 0: RCPS embedding + norm)
        const LayerWeights& W = e->layers[li];
        const EmbedRows emb{.ids = ids_of(c), .emb = e->emb, .comp8 = e->comp, .B = c.Bc, .L = L};
        if (pl.fold) {
            if (li == 0) {      // res = Emb[token] (fp32, fragment layout) [+ u = the same rows in the model dtype and rstd when layer 0's in_proj runs as a GEMM]
                ProfScope ps(e, PCAD_K_NORM, s);
                HIP_TRY(launch_embed_rmsnorm({.w = W.norm_w, .y = pl.tab0 ? nullptr : c.w.u, .res_out = c.w.res, .D = D, .eps = eps, .dt = dt, .rdt = rdt, .rstd_out = c.w.rstd, .Dp = Dp}, emb, s));
            }
            return PCAD_OK;     // later layers: the previous out_proj's epilogue already produced res, round(res) and rstd
        }
        if (li == 0) {
            ProfScope ps(e, PCAD_K_NORM, s);
            HIP_TRY(launch_embed_rmsnorm({.w = W.norm_w, .y = c.w.u, .res_out = c.w.res, .D = D, .eps = eps, .dt = dt, .rdt = rdt, .split_y = pl.sp}, emb, s));
        } else {
            ProfScope ps(e, PCAD_K_NORM, s);
            HIP_TRY(launch_add_rmsnorm({.x = c.w.h, .res_in = c.w.res, .w = W.norm_w, .y = c.w.u, .res_out = c.w.res, .rows = (int64_t)2 * c.Bc * L, .D = D, .eps = eps, .dt = dt, .rdt = rdt,
                                        .split_y = pl.sp}, s));
        }
        return PCAD_OK;
    }
    int in_proj_conv(Lane& c, int li) const {        // in_proj, conv + x_proj (both directions)
        const LayerWeights& W = e->layers[li];
        const int S = 2 * c.Bc;
        const int64_t rows = (int64_t)S * L;
        const bool sp = pl.sp;
        if (pl.untied) {
            for (int d = 0; d < 2; ++d) {       // each direction's own in_proj, then conv + SiLU on its own x
                void *xd = d ? c.w.xz2 : c.w.xz, *zd = d ? c.w.zb2 : c.w.zb;
                { ProfScope ps(e, PCAD_K_GEMM_IN, s);
                HIP_TRY(in_proj(c, W, rows, d, xd, zd)); }
                ProfScope ps(e, PCAD_K_CONV, s);
                ConvLaunch cv{.x = xd, .ldx = ldxz(), .ldy = E, .S = S, .L = L, .E = E, .dt = dt, .in_blocked = e->xzsplit, .out_blocked = e->blocked};
                const bool reverse = d == 1;
                ConvDirection& side = reverse ? cv.rev : cv.fwd;        // launch_conv_dir reads the side that `reverse` names
                side = {.w = W.dir[d].conv_w, .b = W.dir[d].conv_b, .y = c.w.xc[d]};
                HIP_TRY(launch_conv_dir(cv, reverse, s));
            }
            return PCAD_OK;
        }
        // in_proj (tied between directions: once per strand)
        // Layer 0 of the norm-folded form: the operand rows are the V = 8 embedding rows themselves, so in_proj's output is a look-up
        // (table built at bind time): one copy kernel instead of 1 / n_layer of the in_proj GEMMs.  PCAD_DEV=1 PCAD_NO_TAB0=1: the GEMM.
        if (pl.fold && li == 0 && pl.tab0) {
            ProfScope ps(e, PCAD_K_NORM, s);
            HIP_TRY(launch_embed_xz_gather(ids_of(c), e->comp, e->xz_tab0, c.w.xz, c.w.zb, c.Bc, L, E, dt, s));
        } else
        for (int rep = 0; rep < reps(PCAD_K_GEMM_IN); ++rep)
        { ProfScope ps(e, PCAD_K_GEMM_IN, s);
        if (pl.fold)        // on the un-normalised rows (Dp apart), W_in . diag(w_norm) folded at bind time: scaled by the row's rstd
            HIP_TRY(launch_gemm_nt_two({.A = c.w.u, .lda = Dp, .W = W.W_in_f, .ldw = D, .M = rows, .N = 2 * E, .K = D, .dt = dt},
                                       {.C1 = c.w.xz, .C2 = c.w.zb, .nsplit = E, .out_blocked = true, .rscale = c.w.rstd}, s));
        else HIP_TRY(in_proj(c, W, rows, 0, c.w.xz, c.w.zb)); }
        // conv1d + SiLU, causal and anti-causal from one read of x (fused with x_proj of both directions when possible)
        if (convx_fused(rows)) for (int rep = 0; rep < reps(PCAD_K_CONV); ++rep) {
            ProfScope ps(e, PCAD_K_CONV, s);
            ConvxLaunch cx{.x = c.w.xz, .convw = W.convw, .S = S, .L = L, .E = E, .dt = dt, .Rp = Rp,
                           .dtl_split = sp,        // dt_low as bf16 [hi | lo] for the scan's split dt_proj
                           .w_split = sp, .part_ws = c.w.cxp, .policy_S = 2 * B};
            for (int d = 0; d < 2; ++d) cx.dir[d] = {.Wx = sp ? W.dir[d].Wx_s : W.dir[d].Wx, .xc = c.w.xc[d], .dtl = c.w.dtl[d], .bc = c.w.bc[d]};
            HIP_TRY(launch_convx(cx, s));
        } else {
            ProfScope ps(e, PCAD_K_CONV, s);
            HIP_TRY(launch_conv_bidir({.x = c.w.xz, .ldx = ldxz(), .fwd = {.w = W.dir[0].conv_w, .b = W.dir[0].conv_b, .y = c.w.xc[0]},
                                       .rev = {.w = W.dir[1].conv_w, .b = W.dir[1].conv_b, .y = c.w.xc[1]}, .S = S, .L = L, .E = E, .dt = dt,
                                       .in_blocked = e->xzsplit, .out_blocked = e->blocked}, s));
        }
        return PCAD_OK;
    }
    int scans(Lane& c, int li) const {        // x_proj + fused dt_proj/scan, both directions
        const LayerWeights& W = e->layers[li];
        const int S = 2 * c.Bc;
        const int64_t rows = (int64_t)S * L;
        const bool dts = this->dts(rows), strict = pl.strict, ys_from_scan = this->ys_from_scan(li);
        if (pair(rows, li)) {
            ScanPairLaunch pw{.fwd = scan_dir(c, W, 0, dts), .rev = scan_dir(c, W, 1, dts), .z = c.w.zb, .lddt = lddt(dts), .Rp = Rp, .y = c.w.y,
                              .S = S, .L = L, .E = E, .dt = dt, .gate_each = !e->gate_once, .ws = c.w.pair, .ysplit = ys_from_scan ? c.w.ys : nullptr,
                              .dt_split = dts};
            for (int ph = 1; ph <= 2; ++ph) {
                ProfScope ps(e, PCAD_K_SCAN, s);
                pw.phases = ph;
                HIP_TRY(launch_scan_pair(pw, s));
            }
            return PCAD_OK;
        }
        for (int d = 0; d < 2; ++d) {
            const DirWeights& dw = W.dir[d];
            // x_proj -> dt_low [rows, Rp] (model dtype, zero padded) and B_t | C_t [rows, 32] (fp32 side output)
            if (!convx_fused(rows)) { ProfScope ps(e, PCAD_K_GEMM_X, s);
            HIP_TRY(launch_gemm_nt_split({.A = c.w.xc[d], .lda = E, .W = dw.Wx, .ldw = E, .M = rows, .N = XP, .K = E, .dt = dt, .a_blocked = e->blocked},
                                         {.C = c.w.dtl[d], .ldc = Rp, .C2 = c.w.bc[d], .ldc2 = 2 * N, .nsplit = Rp}, s)); }
            const ScanLaunch base = scan_of(c, W, d, dts);
            // dt_proj (on MFMA inside the scan) + bias + softplus + recurrence + D skip + SiLU(z) gate
            for (int rep = 1; rep < (d == 0 ? reps(PCAD_K_SCAN) : 1); ++rep)         // measurement aid: the forward-direction launch is idempotent
                HIP_TRY(launch_scan(base, s));       // ungated, whole walk, into y
            ProfScope ps(e, PCAD_K_SCAN, s);
            const void* zp = e->xzsplit ? c.w.zb : (const void*)((const char*)c.w.xz + (size_t)E * esz);
            if (pl.untied && d == 1) zp = e->xzsplit ? c.w.zb2 : (const void*)((const char*)c.w.xz2 + (size_t)E * esz);      // its own in_proj's z
            // gate_once: the forward scan stores its ungated output, the reverse scan adds its own and applies SiLU(z)
            // to the sum (one SiLU per element instead of two, z read once; a rounding-order difference from
            // y_f*g + y_r*g, like the out_proj fold below).  PCAD_GATE_EACH=1: each direction gated and rounded.
            const bool gated = strict || !e->gate_once || d == 1;
            ScanLaunch sc = base;
            sc.z = gated ? zp : nullptr;
            sc.y = d == 1 ? y_rev(c) : c.w.y;
            sc.reverse = d == 1;
            sc.accumulate = strict ? 0 : (d == 1 ? (e->gate_once ? 2 : 1) : 0);
            sc.walk_len = last_short(li) ? pl.walk_len : 0;
            sc.ysplit = d == 1 && ys_from_scan ? c.w.ys : nullptr;
            HIP_TRY(launch_scan(sc, s));
        }
        return PCAD_OK;
    }
    // out = round(out_proj(y_fwd)) + round(out_proj(y_rev)), rounded: BiMambaWrapper's "add" of two Mamba calls that each end
    // in their own (tied) out_proj.  Second output: u (dead since in_proj); last-layer shortcut: the gathered rows go
    // through u, the second small output to xz (dead since the scans).
    int out_proj_strict(Lane& c, int li) const {
        const int S = 2 * c.Bc;
        const int64_t rows = (int64_t)S * L;
        if (last_short(li)) {
            ProfScope ps(e, PCAD_K_HEAD, s);
            // the gathered rows of one direction (in u) through the tied out_proj: the same product as the full-size launch
            // (split-bf16 with "f32_gemm_split": bit-identical rows)
            HIP_TRY(gather_rows(c, c.w.y));
            HIP_TRY(out_proj(c, li, c.w.u, (int64_t)S * P, c.w.h, 0, false));
            HIP_TRY(gather_rows(c, y_rev(c)));
            HIP_TRY(out_proj(c, li, c.w.u, (int64_t)S * P, c.w.xz, 1, false));
            HIP_TRY(launch_add_round(c.w.h, c.w.xz, (int64_t)S * P * D, dt, s));
            return truncated() ? emit_level(c, li + 1, true) : PCAD_OK;
        }
        { ProfScope ps(e, PCAD_K_GEMM_OUT, s);
        HIP_TRY(out_proj(c, li, c.w.y, rows, c.w.h, 0, e->blocked)); }
        { ProfScope ps(e, PCAD_K_GEMM_OUT, s);
        HIP_TRY(out_proj(c, li, y_rev(c), rows, c.w.u, 1, e->blocked)); }
        { ProfScope ps(e, PCAD_K_NORM, s);
        HIP_TRY(launch_add_round(c.w.h, c.w.u, rows * D, dt, s)); }
        return li + 1 < e->nl ? emit_level(c, li + 1) : PCAD_OK;
    }
    int out_proj_shortcut(Lane& c, int li) const {       // out_proj on the evaluated rows only: gather (-> u, dead since in_proj) and a small GEMM (-> first rows of h)
        ProfScope ps(e, PCAD_K_HEAD, s);          // counted with the head: not a full-size out_proj launch
        HIP_TRY(gather_rows(c, c.w.y));
        // split: the same split-bf16 product as the full-size out_proj (same operand values, same K order: bit-identical rows)
        HIP_TRY(out_proj(c, li, c.w.u, (int64_t)2 * c.Bc * P, c.w.h, 0, false));
        return truncated() ? emit_level(c, li + 1, true) : PCAD_OK;      // a truncated walk: level `depth` from the compact rows
    }
    int out_proj_folded(Lane& c, int li) const {     // out_proj + residual add + the next block's norm statistics in one launch
        const LayerWeights& W = e->layers[li];
        const int64_t rows = (int64_t)2 * c.Bc * L;
        { ProfScope ps(e, PCAD_K_GEMM_OUT_RES, s);
        HIP_TRY(launch_gemm_nt_res({.A = c.w.y, .lda = E, .W = W.W_out_p, .ldw = E, .M = rows, .N = Dp, .K = E, .dt = dt, .a_blocked = e->blocked},
                                   {.C = c.w.u, .res = (float*)c.w.res, .ssq = c.w.ssq}, s)); }
        ProfScope ps(e, PCAD_K_RSTD, s);
        HIP_TRY(launch_rstd(c.w.ssq, c.w.rstd, rows, Dp / 128, D, eps, s));
        return PCAD_OK;
    }
    int out_proj_plain(Lane& c, int li) const {      // out_proj on (y_fwd + y_rev): the two tied out_proj calls folded by linearity
        for (int rep = 0; rep < reps(PCAD_K_GEMM_OUT); ++rep)
        { ProfScope ps(e, PCAD_K_GEMM_OUT, s);
        HIP_TRY(out_proj(c, li, c.w.y, (int64_t)2 * c.Bc * L, c.w.h, 0, e->blocked)); }
        return li + 1 < e->nl ? emit_level(c, li + 1) : PCAD_OK;
    }
    int mixer_out(Lane& c, int li) const {
        return pl.strict ? out_proj_strict(c, li) : last_short(li) ? out_proj_shortcut(c, li)
               : pl.fold && li + 1 < e->nl ? out_proj_folded(c, li) : out_proj_plain(c, li);
    }
    // ---- heads: to add one, add its fields to ForwardRequest, a Head value, a function here and its case in head() --------------
    int head_lm(Lane& c) const {
        void* hout = rq.hidden_out ? (char*)rq.hidden_out + ((size_t)c.b0 * pl.Q * 2 * D) * esz : nullptr;
        float* lout = rq.logits_out ? rq.logits_out + (size_t)c.b0 * pl.Q * e->V : nullptr;
        if (!hout && !lout) return PCAD_OK;
        ProfScope ps(e, PCAD_K_HEAD, s);
        HIP_TRY(launch_final_head({.in = head_in(c), .emb_f32 = e->emb_f32, .comp8 = e->comp, .hidden_out = hout, .logits_out = lout, .pos = pos,
                                   .pos_per_seq = ppw_of(c), .h_compact = pl.walk_len > 0}, s));
        return PCAD_OK;
    }
    int head_pooled(Lane& c) const {
        const auto& pool = rq.pool;
        const size_t part = pool_partial_bytes(c.Bc, L, D, pool.pooling);
        if (int rc = fits_dead(c, part, "pcad_forward_pooled", "head's partials")) return rc;
        ProfScope ps(e, PCAD_K_HEAD, s);
        HIP_TRY(launch_pooled_head({.in = head_in(c), .score_w = pool.score_w, .NL = pool.num_labels, .pooled_out = pool.pooled_out ? pool.pooled_out + (size_t)c.b0 * 2 * D : nullptr,
                                    .logits_out = pool.logits_out + (size_t)c.b0 * pool.num_labels, .pooling = pool.pooling, .part = c.w.xz}, s));
        return PCAD_OK;
    }
    int head_loss(Lane& c) const {       // per-segment partials in the dead buffers, as the pooled head's
        const auto& loss = rq.loss;
        if (int rc = fits_dead(c, loss_partial_bytes(c.Bc, L), "pcad_forward_loss", "head's partials")) return rc;
        const size_t o = (size_t)c.b0 * L;
        ProfScope ps(e, PCAD_K_HEAD, s);
        HIP_TRY(launch_loss_head({.in = head_in(c), .emb_f32 = e->emb_f32, .comp8 = e->comp, .labels = loss.labels + o, .loss_w = loss.loss_weights ? loss.loss_weights + o : nullptr,
                                  .ignore_index = loss.ignore_index, .sums_out = loss.sums_out + (size_t)c.b0 * 4, .nll_out = loss.nll_out ? loss.nll_out + o : nullptr,
                                  .logits_out = loss.logits_out ? loss.logits_out + o * e->V : nullptr, .part = c.w.xz}, s));
        return PCAD_OK;
    }
    int head_probs(Lane& c) const {
        const auto& probs = rq.probs; const int Qp = pl.Q;
        ProfScope ps(e, PCAD_K_HEAD, s);
        HIP_TRY(launch_probs_head({.in = head_in(c), .emb_f32 = e->emb_f32, .comp8 = e->comp, .cols = probs.cols,
                                   .probs_out = probs.probs_out ? probs.probs_out + (size_t)c.b0 * Qp * 4 : nullptr,
                                   .logits_out = probs.logits_out ? probs.logits_out + (size_t)c.b0 * Qp * e->V : nullptr, .pos = pos, .pos_per_window = ppw_of(c),
                                   .Pw = rq.Pw, .h_compact = pl.walk_len > 0}, s));
        return PCAD_OK;
    }
    int head_layers(Lane& c) const {
        // hidden_states[-1]: the final head's assembled rows [Bc, P, 2D] (per-window lists with P > 1: [P, Bc, 2D], one launch per slot
        // on that slot's column of the list) go to xz, the column copy of the chunk's per-window list behind them - both dead
        // once the last out_proj has run, so the forward's workspace size is unchanged.  The head runs even when the last
        // level is not requested: it is what validates the token ids.
        const int32_t* ppw = ppw_of(c);
        char* rows_tmp = (char*)c.w.xz;
        const size_t slot_bytes = (size_t)c.Bc * 2 * D * esz, rows_bytes = align_up(slot_bytes * layP);
        const bool columns = ppw && layP > 1;
        if (int rc = fits_dead(c, rows_bytes + (columns ? align_up((size_t)c.Bc * layP * 4) : 0), "pcad_forward_layers", "last level's rows", rows_bytes)) return rc;
        const int slot = lay_slot(e->nl);
        // the assembled rows -> the caller's tensor; sb / sq: rows_tmp's rows between two windows / two slots
        auto emit = [&](int64_t sb, int64_t sq) {
            return launch_layer_rows({.src = rows_tmp, .out = lay_dst(slot, c.b0), .B = c.Bc, .L = L, .D = D, .dt = dt, .pos = pos, .P = layP, .assembled = true, .sb = sb, .sq = sq,
                                      .average = rq.lay.average}, s);
        };
        FinalHeadLaunch fh{.in = head_in(c), .emb_f32 = e->emb_f32, .comp8 = e->comp, .hidden_out = rows_tmp, .pos = pos, .h_compact = pl.walk_len > 0};
        ProfScope ps(e, PCAD_K_HEAD, s);
        if (ppw) {
            const int32_t* col = ppw;                // P == 1: the list is its own column (pcad_forward_at's launch)
            if (columns) {
                col = (const int32_t*)(rows_tmp + rows_bytes);
                HIP_TRY(launch_position_columns(ppw, (int32_t*)(rows_tmp + rows_bytes), c.Bc, layP, s));
            }
            fh.h_compact = false;
            for (int q = 0; q < layP; ++q) {         // slot q of every window: [P, Bc, 2D]
                fh.hidden_out = rows_tmp + slot_bytes * q;
                fh.pos_per_seq = col + (size_t)q * c.Bc;
                HIP_TRY(launch_final_head(fh, s));
            }
            if (slot >= 0) HIP_TRY(emit(1, c.Bc));
        } else {
            HIP_TRY(launch_final_head(fh, s));      // [Bc, P, 2D]
            if (slot >= 0) HIP_TRY(emit(layP, 1));
        }
        return PCAD_OK;
    }
    // A truncated walk runs neither norm_f nor the head; what the head would have reported about the chunk's token ids is reported here
    int ids_check(Lane& c) const {
        ProfScope ps(e, PCAD_K_HEAD, s);
        HIP_TRY(launch_ids_check(ids_of(c), (int64_t)c.Bc * L, e->status, s));
        return PCAD_OK;
    }
    int head(Lane& c) const {
        if (truncated()) return ids_check(c);
        return rq.head == Head::pooled ? head_pooled(c) : rq.head == Head::loss ? head_loss(c) : rq.head == Head::probs ? head_probs(c)
               : rq.head == Head::layers ? head_layers(c) : head_lm(c);
    }
    // ---- one chunk: to add a layer form, add its per-call decision to ForwardPlan and its branch to the phase it replaces -------
    int run() const {
        for (int ck = 0; ck < pl.nchunks; ++ck) {
            Lane c;
            c.b0 = ck * pl.chunk;
            c.Bc = (B - c.b0) < pl.chunk ? (B - c.b0) : pl.chunk;
            c.w = carve_workspace(e, rq.workspace, c.Bc, L, B);
            if (int rc = level0(c)) return rc;
            for (int li = 0; li < pl.depth; ++li) {
                if (int rc = add_norm(c, li)) return rc;
                if (int rc = in_proj_conv(c, li)) return rc;
                if (int rc = scans(c, li)) return rc;
                if (int rc = mixer_out(c, li)) return rc;
            }
            if (int rc = head(c)) return rc;
        }
        return PCAD_OK;
    }
};

int forward_impl(pcad_handle h, const ForwardRequest& rq) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_forward: null handle");
    pcad_engine* e = h; const int B = rq.B, L = rq.L;
    if (!e->bound) return fail(PCAD_ERR_UNBOUND, "pcad_forward: weights not bound");
    if (B < 0 || L <= 0) return fail(PCAD_ERR_INVALID, "pcad_forward: bad B=%d L=%d", B, L);
    if (B == 0) return PCAD_OK;
    if (!rq.ids || !rq.workspace) return fail(PCAD_ERR_INVALID, "pcad_forward: null ids/workspace");
    Positions pos;
    if (int rc = positions_arg("pcad_forward", rq.positions, rq.P, L, &pos)) return rc;
    if (((uintptr_t)rq.workspace) % 256) return fail(PCAD_ERR_WORKSPACE, "workspace must be 256-byte aligned");
    const size_t need = pcad_workspace_bytes(h, B, L);
    if (rq.ws_bytes < need) return fail(PCAD_ERR_WORKSPACE, "workspace too small: %zu < %zu", rq.ws_bytes, need);
    // debug aid (race / uninitialised-read screen): every byte of the workspace starts as 0xFF, so a kernel that consumes a
    // value no kernel of THIS forward produced turns the outputs into NaN instead of silently reusing the previous call's data
    if (e->poison) HIP_TRY(hipMemsetAsync(rq.workspace, 0xFF, need, (hipStream_t)rq.stream));
    // (also when the fold is only the DEFAULT of this model - a bf16 engine bound under "norm_fold" 0 / "reference_order" >= 1 and switched
    // back afterwards: running unfolded would silently cost 4.5 % and differ from a freshly bound engine; like "f32_gemm_split" it is refused)
    if (fold_wanted(e) && !e->fold_packed)
        return fail(PCAD_ERR_INVALID, "pcad_forward: the norm-folded layer form (\"norm_fold\" %s) was enabled after pcad_bind_weights, under options that "
                                      "did not ask for it; its weight copies are packed at bind time - set \"norm_fold\" / \"reference_order\" before "
                                      "pcad_weight_arena_bytes / pcad_bind_weights (turning the form OFF afterwards is always possible)",
                    e->norm_fold == 1 ? "1" : "default");
    if (split_wanted(e) && !e->split_packed)
        return fail(PCAD_ERR_INVALID, "pcad_forward: \"f32_gemm_split\" 1 was set after pcad_bind_weights; the split weight copies are packed at "
                                      "bind time - set the option before pcad_weight_arena_bytes / pcad_bind_weights");
    if (e->untied && !e->untied_packed)
        return fail(PCAD_ERR_INVALID, "pcad_forward: \"untied_directions\" 1 was set after pcad_bind_weights; mamba_rev's in_proj / out_proj are packed at "
                                      "bind time - set the option before pcad_weight_arena_bytes / pcad_bind_weights");
    const ForwardPlan pl = plan_forward(e, rq, pos);
    return Walk(e, rq, pl, pos).run();
}

}  // namespace

extern "C" {

int pcad_forward(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* positions, int P, void* hidden_out,
                 float* logits_out, void* workspace, size_t workspace_bytes, pcad_stream stream) {
    ForwardRequest rq;
    rq.head = Head::lm; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.positions = positions; rq.P = P; rq.hidden_out = hidden_out; rq.logits_out = logits_out;
    return forward_impl(h, rq);
}

int pcad_forward_pooled(pcad_handle h, const int32_t* ids, int B, int L, int pooling, const float* score_w, int num_labels,
                        float* pooled_out, float* logits_out, void* workspace, size_t workspace_bytes, pcad_stream stream) {
    if (pooling < PCAD_POOL_MEAN || pooling > PCAD_POOL_LAST) return fail(PCAD_ERR_INVALID, "pcad_forward_pooled: bad pooling %d", pooling);
    if (num_labels < 1 || num_labels > PCAD_MAX_LABELS)
        return fail(PCAD_ERR_INVALID, "pcad_forward_pooled: num_labels=%d out of range [1, %d]", num_labels, PCAD_MAX_LABELS);
    if (!score_w || !logits_out) return fail(PCAD_ERR_INVALID, "pcad_forward_pooled: null score_w / logits_out");
    ForwardRequest rq;
    rq.head = Head::pooled; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.pool.pooling = pooling; rq.pool.score_w = score_w; rq.pool.num_labels = num_labels;
    rq.pool.pooled_out = pooled_out; rq.pool.logits_out = logits_out;
    return forward_impl(h, rq);
}

int pcad_forward_loss(pcad_handle h, const int32_t* ids, const int32_t* labels, const float* loss_weights, int ignore_index, int B,
                      int L, float* sums_out, float* nll_out, float* logits_out, void* workspace, size_t workspace_bytes,
                      pcad_stream stream) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_forward_loss: null handle");
    if (B < 0 || L <= 0) return fail(PCAD_ERR_INVALID, "pcad_forward_loss: bad B=%d L=%d", B, L);
    if (B > 0 && (!labels || !sums_out)) return fail(PCAD_ERR_INVALID, "pcad_forward_loss: null labels / sums_out");
    ForwardRequest rq;
    rq.head = Head::loss; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.loss.labels = labels; rq.loss.loss_weights = loss_weights; rq.loss.ignore_index = ignore_index;
    rq.loss.sums_out = sums_out; rq.loss.nll_out = nll_out; rq.loss.logits_out = logits_out;
    return forward_impl(h, rq);
}

int pcad_forward_probs(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* positions, int P, const int32_t* pos_per_window,
                       const int32_t* cols, float* probs_out, float* logits_out, void* workspace, size_t workspace_bytes,
                       pcad_stream stream) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_forward_probs: null handle");
    if (positions && pos_per_window) return fail(PCAD_ERR_INVALID, "pcad_forward_probs: positions and pos_per_window are exclusive");
    if (P < 0 || P > PCAD_MAX_POSITIONS || (P > 0 && !positions && !pos_per_window) || (P == 0 && (positions || pos_per_window)))
        return fail(PCAD_ERR_INVALID, "pcad_forward_probs: bad positions (P=%d)", P);
    if (!probs_out && !logits_out) return fail(PCAD_ERR_INVALID, "pcad_forward_probs: no output requested");
    if (((uintptr_t)probs_out) % 16) return fail(PCAD_ERR_INVALID, "pcad_forward_probs: probs_out must be 16-byte aligned");
    ForwardRequest rq;
    rq.head = Head::probs; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    if (int rc = probs_cols_arg("pcad_forward_probs", cols, h->V < PCAD_MAX_VOCAB ? h->V : PCAD_MAX_VOCAB, &rq.probs.cols)) return rc;
    rq.probs.probs_out = probs_out; rq.probs.logits_out = logits_out;
    // shared positions: pcad_forward's walk (last-layer shortcut included); per-window lists: pcad_forward_at's (the full last layer)
    if (pos_per_window) { rq.pos_per_window = pos_per_window; rq.Pw = P; } else { rq.positions = positions; rq.P = P; }
    return forward_impl(h, rq);
}

int pcad_forward_layers(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* positions, int P, const int32_t* pos_per_window,
                        const int32_t* layers, int NL, int average, void* out, void* workspace, size_t workspace_bytes, pcad_stream stream) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: null handle");
    if ((positions != nullptr) == (pos_per_window != nullptr))
        return fail(PCAD_ERR_INVALID, "pcad_forward_layers: exactly one of positions and pos_per_window (the all-positions form is pcad_forward_all_hidden)");
    if (P < 1 || P > PCAD_MAX_POSITIONS) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: bad positions (P=%d)", P);
    const int nl = h->nl;
    if (layers ? (NL < 1 || NL > nl + 1) : NL != 0) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: bad layers (NL=%d, n_layer=%d)", NL, nl);
    for (int i = 0; i < NL; ++i) {
        if (layers[i] < 0 || layers[i] > nl) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: level %d outside [0, %d]", layers[i], nl);
        if (i > 0 && layers[i] <= layers[i - 1]) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: levels must be strictly increasing");
    }
    if (!out || ((uintptr_t)out) % 16) return fail(PCAD_ERR_INVALID, "pcad_forward_layers: out must be a 16-byte aligned pointer");
    ForwardRequest rq;
    rq.head = Head::layers; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.lay.layers = layers; rq.lay.NL = layers ? NL : nl + 1; rq.lay.inter = !layers || layers[0] < nl;
    rq.lay.top = layers ? layers[NL - 1] : nl;
    rq.lay.average = average != 0; rq.lay.out = out;
    // the last level alone: pcad_forward's walk for a shared list (norm fold and last-layer shortcut as that call chooses them), the
    // full last layer for per-window lists (P == 1: pcad_forward_at's walk); any level below it: pcad_forward_all_hidden's walk, which
    // stops after block `top` - 1 when `top` < n_layer (plan_forward: depth)
    if (pos_per_window) { rq.pos_per_window = pos_per_window; rq.Pw = P; } else { rq.positions = positions; rq.P = P; }
    return forward_impl(h, rq);
}

int pcad_forward_at(pcad_handle h, const int32_t* ids, int B, int L, const int32_t* pos_per_seq, void* hidden_out,
                    float* logits_out, void* workspace, size_t workspace_bytes, pcad_stream stream) {
    if (!pos_per_seq) return fail(PCAD_ERR_INVALID, "pcad_forward_at: null pos_per_seq");
    ForwardRequest rq;
    rq.head = Head::lm; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.pos_per_window = pos_per_seq; rq.Pw = 1; rq.hidden_out = hidden_out; rq.logits_out = logits_out;
    return forward_impl(h, rq);
}

int pcad_forward_all_hidden(pcad_handle h, const int32_t* ids, int B, int L, void* all_hidden, void* hidden_out,
                            float* logits_out, void* workspace, size_t workspace_bytes, pcad_stream stream) {
    if (!all_hidden) return fail(PCAD_ERR_INVALID, "pcad_forward_all_hidden: null all_hidden");
    ForwardRequest rq;
    rq.head = Head::lm; rq.ids = ids; rq.B = B; rq.L = L; rq.workspace = workspace; rq.ws_bytes = workspace_bytes; rq.stream = stream;
    rq.all_hidden = all_hidden; rq.hidden_out = hidden_out; rq.logits_out = logits_out;
    return forward_impl(h, rq);
}

}  // extern "C"
