// What api.hip, forward.hip and ops_api.hip share.  Internal to libpcad.so: nothing here is part of include/pcad.h.
#pragma once
#include <hip/hip_runtime.h>
#include <vector>
#include "../../include/pcad.h"
#include "kernels.hpp"

namespace pcad {
int fail(int code, const char* fmt, ...);      // api.hip: sets the calling thread's pcad_last_error text, returns `code`

#define HIP_TRY(expr)                                                                             \
    do {                                                                                          \
        hipError_t _e = (expr);                                                                   \
        if (_e != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", #expr, hipGetErrorString(_e)); \
    } while (0)

inline size_t align_up(size_t v, size_t a = 256) { return (v + a - 1) / a * a; }

struct DirWeights {
    float *conv_w, *conv_b;   // [E,4], [E]
    void* Wx;                 // [XP, E] dtype
    void* Wx_s;               // [XP, 2E] bf16, per 32-channel K-tile [hi | lo] ("f32_gemm_split": x_proj inside the fused conv kernel), else nullptr
    void* Wdt;                // [E, Rp] dtype
    void* Wdt_s;              // [E, 2 Rp] bf16 = [hi | lo] of Wdt ("f32_gemm_split": the fp32 model's dt_proj on the bf16 pipes), else nullptr
    float *dt_bias, *A2, *Dskip;
};
struct LayerWeights {
    float* convw;    // conv taps of both directions packed per K-tile for the fused conv+x_proj kernel
    float* norm_w;   // [D]
    void* W_in;      // [2E, D]
    void* W_in_f;    // [2E, D] = W_in . diag(norm_w), rounded once from the source precision: in_proj of the norm-folded form
    void* W_out;     // [D, E]
    void* W_out_p;   // [Dp, E]: W_out with zero rows up to Dp = round_up(D, 256) for the folded out_proj (== W_out when D % 256 == 0)
    void* W_in_s;    // [2E, 2D] bf16 = [hi | lo] of W_in: split-bf16 in_proj of the fp32 model ("f32_gemm_split"), else nullptr
    void* W_out_s;   // [D, 2E] bf16 = [hi | lo] of W_out
    // "untied_directions": mamba_rev's own in_proj / out_proj (W_in / W_out above are then mamba_fwd's), and their [hi | lo] copies; else nullptr
    void *W_in_r, *W_out_r, *W_in_s_r, *W_out_s_r;
    DirWeights dir[2];
};
}  // namespace pcad

struct pcad_engine {
    pcad_config cfg;
    int D, E, N, R, Rp, XP, V, nl;
    int esz;        // bytes per activation element
    int rdt;        // residual dtype
    int chunk;      // PCAD_CHUNK_SEQS override: sequences per pass through the layer stack (0: derive from chunk_rows)
    int64_t chunk_rows;   // token-rows (2 strands x L per window) per pass through the layer stack
    bool gate_once; // SiLU(z) applied once to y_fwd + y_rev (reverse scan) instead of once per direction
    bool convx;     // conv + x_proj of both directions in one kernel (needs xzsplit and Rp == 64 or 96: dt_rank <= 96); PCAD_NO_CONVX=1: off
    bool xzsplit;   // in_proj writes x and z as two blocked tensors (needs `blocked`); PCAD_PLAIN_XZ=1 turns it off (A/B knob)
    bool blocked;   // xc and y in the blocked layout (common.hpp::blocked_off); PCAD_PLAIN_LAYOUT=1 turns it off (A/B knob)
    bool segments = true;  // pcad_set_option("scan_segments", 0): never cut the scan of long strands into segments
    bool shortcut = true;  // pcad_set_option("last_layer_shortcut", 0): run the last layer in full even when only a few positions are evaluated
    int ref_order = 0;      // pcad_set_option("reference_order", 0 / 1 / 2): see include/pcad.h; 2 = each direction's tied out_proj on its own
    int norm_fold = -1;     // pcad_set_option("norm_fold", 0 / 1); -1 (default): on for the bf16 model, off for the fp32 model (api.hip fold_wanted)
    int rep_class = -1, rep_count = 1;   // pcad_set_option("debug_repeat_class" / "debug_repeat"): measurement aid, see forward.hip Walk::reps
    bool poison = false;   // pcad_set_option("poison_workspace", 1): debug — fill the workspace with 0xFF (NaN patterns) before every forward
    bool bound = false;
    int64_t ws_limit = 0;       // pcad_set_option("workspace_limit_mb"): chunks are sized so that the workspace stays below it (0: no limit)
    bool f32_split = false;     // pcad_set_option("f32_gemm_split", 1): the fp32 model's in_proj / out_proj as split-bf16 GEMMs (split_wanted)
    bool split_packed = false;  // ... and their [hi | lo] weight copies exist in the arena (decided like fold_packed)
    bool untied = false;        // pcad_set_option("untied_directions", 1): mamba_fwd and mamba_rev each run their own in_proj / out_proj
    bool untied_packed = false; // ... and mamba_rev's weights exist in the arena (decided like fold_packed)
    bool fold_packed = false;   // the norm-folded form's extra weight copies (W_in_f, xz_tab0, padded W_out) exist in the arena: decided
                                // from the options in force when pcad_weight_arena_bytes / pcad_bind_weights run (fold_wanted)
    int32_t* status = nullptr;   // caller-owned device word for asynchronous input-validation flags (pcad_set_status_buffer)
    std::vector<pcad::LayerWeights> layers;
    void* xz_tab0 = nullptr;    // [V, 2E] dtype: layer 0's in_proj output per token id (norm-folded form), built at bind time
    void* emb = nullptr;        // [V, D] dtype
    float* emb_f32 = nullptr;   // [V, D] fp32 copy of the dtype-rounded table
    float* normf_w = nullptr;
    int32_t* comp = nullptr;    // [8] device
    // optional per-kernel-class timing with HIP events recorded on the caller's stream
    bool prof = false;
    int prof_stride = 1;                                  // bracket every prof_stride-th launch of a class
    int64_t prof_seen[PCAD_NUM_KERNEL_CLASSES] = {0};
    std::vector<std::pair<hipEvent_t, hipEvent_t>> prof_ev[PCAD_NUM_KERNEL_CLASSES];
    std::vector<hipEvent_t> prof_pool;
    double prof_ms[PCAD_NUM_KERNEL_CLASSES] = {0};
    int64_t prof_n[PCAD_NUM_KERNEL_CLASSES] = {0};
};

namespace pcad {
bool fold_wanted(const pcad_engine* e);      // whether the options ask for the norm-folded layer form on this model at all (api.hip)
bool split_wanted(const pcad_engine* e);     // ... for the split-bf16 GEMMs
// The small-launch forms of one pcad_forward call (kernels.hpp): chosen from the strands of the WHOLE call, not per chunk, so that
// results never depend on the chunking.  carve_workspace carves a form's scratch exactly when the form runs; the walk asks here too.
struct SmallForms {
    int G = 1;            // segments per strand of the segmented scan (1: plain walks)
    bool pair = false;    // pair walks, where the layer allows them (forward.hip Walk::pair)
    int ksplit = 1;       // K-split factor of the fused conv + x_proj kernel (1: none)
};
SmallForms small_forms(const pcad_engine* e, int B, int L);
struct Workspace {
    void *res, *u, *h, *xz, *zb, *xc[2], *dtl[2], *y;
    void *xz2, *zb2;   // "untied_directions": the reverse direction's own in_proj output (laid out as xz / zb); else nullptr
    void* ys;        // "f32_gemm_split": out_proj's operand, bf16 [rows8, 2E] blocked = [hi | lo] of y; else nullptr
    float* bc[2];
    float *rstd, *ssq;   // norm-folded form: rstd [rows]; partial sums of squares [rows, D / 128]
    float* seg;      // segmented-scan scratch (long sequences with few strands), or nullptr
    float* pair;     // state hand-over of the pair walks (kernels.hpp scan_pair_wanted), or nullptr
    float* cxp;      // K-split scratch of the fused conv + x_proj kernel (small launches), or nullptr
    size_t bytes;
};
Workspace carve_workspace(const pcad_engine* e, void* base, int Bc, int L, int Bpol);
int chunk_for(const pcad_engine* e, int B, int L);
hipEvent_t prof_event(pcad_engine* e);
constexpr size_t kProfCap = 1 << 16;
struct ProfScope {   // records start/stop events around one launch when profiling is on
    pcad_engine* e; int cls; hipStream_t s; hipEvent_t a = nullptr, b = nullptr;
    ProfScope(pcad_engine* e_, int cls_, hipStream_t s_) : e(e_), cls(cls_), s(s_) {
        // at most kProfCap un-read event pairs per class: a caller that never calls pcad_profile_read cannot grow the lists
        if (e->prof && (e->prof_seen[cls]++ % e->prof_stride) == 0 && e->prof_ev[cls].size() < kProfCap) {
            a = prof_event(e); b = prof_event(e);
            if (a) (void)hipEventRecord(a, s);
        }
    }
    ~ProfScope() {
        if (a && b) { (void)hipEventRecord(b, s); e->prof_ev[cls].push_back({a, b}); }
    }
};

// argument checks shared by entry points (api.hip); who: the entry's name in the message
int positions_arg(const char* who, const int32_t* positions, int P, int L, Positions* pos);
int probs_cols_arg(const char* who, const int32_t* cols, int vocab, ProbCols* out);

}  // namespace pcad
