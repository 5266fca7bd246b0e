// C-ABI of libpcad.so (include/pcad.h): handle, options, status buffer, weight arena and binding, workspace carving, chunking, profiling.
// The layer walk and the pcad_forward* entries: forward.hip; the per-operator entries: ops_api.hip; shared: pcad_internal.hpp.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <string>

#include "build_hash.h"
#include "pcad_internal.hpp"

using namespace pcad;

static thread_local char g_err[512] = "";

int pcad::fail(int code, const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
    return code;
}

int pcad::positions_arg(const char* who, const int32_t* positions, int P, int L, Positions* pos) {
    if (P < 0 || P > PCAD_MAX_POSITIONS || (P > 0 && !positions)) return fail(PCAD_ERR_INVALID, "%s: bad positions (P=%d)", who, P);
    pos->n = P;
    for (int i = 0; i < 16; ++i) pos->p[i] = 0;
    for (int i = 0; i < P; ++i) {
        if (positions[i] < 0 || positions[i] >= L) return fail(PCAD_ERR_INVALID, "%s: position %d out of range [0,%d)", who, positions[i], L);
        pos->p[i] = positions[i];
    }
    return PCAD_OK;
}

int pcad::probs_cols_arg(const char* who, const int32_t* cols, int vocab, ProbCols* out) {
    if (!cols) return fail(PCAD_ERR_INVALID, "%s: null cols", who);
    for (int j = 0; j < 4; ++j) {
        if (cols[j] < 0 || cols[j] >= vocab) return fail(PCAD_ERR_INVALID, "%s: cols[%d]=%d outside [0, %d)", who, j, cols[j], vocab);
        out->c[j] = cols[j];
    }
    return PCAD_OK;
}

// ---- arena carving (identical walk for size query and binding) ------------------------------------
struct Carver {
    char* base;
    size_t off = 0;
    explicit Carver(void* b) : base((char*)b) {}
    void* take(size_t bytes) {
        void* p = base ? base + off : nullptr;
        off += align_up(bytes);
        return p;
    }
};

// whether the options ask for the norm-folded layer form on this model at all (per-forward shape conditions come on top)
bool pcad::fold_wanted(const pcad_engine* e) {
    const bool want = e->norm_fold == 1 || (e->norm_fold < 0 && e->cfg.dtype == PCAD_BF16);
    // never with "untied_directions": the folded out_proj adds ONE product onto the residual, the untied form has two to round and sum
    return want && !e->untied && e->rdt == F32 && e->xzsplit && e->blocked;
}

// "f32_gemm_split": fp32 model only, and never together with the norm-folded form (whose GEMM epilogues are fp32-in / fp32-out)
bool pcad::split_wanted(const pcad_engine* e) {
    return e->f32_split && e->cfg.dtype == PCAD_F32 && !fold_wanted(e) && e->xzsplit && e->blocked && e->D % 64 == 0 && e->E % 64 == 0;
}

// token-rows per pass through the layer stack: the kernels address their tensors with unsigned 32-bit byte offsets; the widest
// per-row tensor is E * esz bytes (x, z, xc, y; with the split-bf16 GEMMs out_proj's operand is 2 E bf16 columns = the same 4 E bytes)
static int64_t chunk_row_limit(const pcad_engine* e) {
    const int64_t per_row = (int64_t)e->E * e->esz;
    return ((((int64_t)1 << 32) - ((int64_t)2 << 20)) / per_row) & ~(int64_t)7;
}

static void carve_weights(pcad_engine* e, Carver& c) {
    const size_t D = e->D, E = e->E, N = e->N, V = e->V, esz = e->esz;
    // the folded form's copies (a second in_proj weight per layer, the layer-0 table, out_proj padded to 256 rows) are carved only
    // when the fold can engage: +37 % of the arena at l32 that an fp32 model or "norm_fold" 0 / "reference_order" never reads
    const bool pf = fold_wanted(e);
    const bool ps = split_wanted(e);
    e->emb = c.take(V * D * esz);
    e->emb_f32 = (float*)c.take(V * D * 4);
    e->normf_w = (float*)c.take(D * 4);
    e->comp = (int32_t*)c.take(8 * 4);
    e->xz_tab0 = pf ? c.take(V * 2 * E * esz) : nullptr;
    e->layers.resize(e->nl);
    for (auto& L : e->layers) {
        L.norm_w = (float*)c.take(D * 4);
        L.convw = (float*)c.take(convx_packed_bytes((int)E, e->cfg.dtype));
        L.W_in = c.take(2 * E * D * esz);
        L.W_in_f = pf ? c.take(2 * E * D * esz) : nullptr;
        L.W_out = c.take(D * E * esz);
        L.W_out_p = pf && (size_t)fold_padded_width((int)D) != D ? c.take((size_t)fold_padded_width((int)D) * E * esz) : L.W_out;
        L.W_in_s = ps ? c.take(2 * E * 2 * D * 2) : nullptr;
        L.W_out_s = ps ? c.take(D * 2 * E * 2) : nullptr;
        L.W_in_r = e->untied ? c.take(2 * E * D * esz) : nullptr;
        L.W_out_r = e->untied ? c.take(D * E * esz) : nullptr;
        L.W_in_s_r = e->untied && ps ? c.take(2 * E * 2 * D * 2) : nullptr;
        L.W_out_s_r = e->untied && ps ? c.take(D * 2 * E * 2) : nullptr;
        for (int d = 0; d < 2; ++d) {
            DirWeights& w = L.dir[d];
            w.conv_w = (float*)c.take(E * 4 * 4);
            w.conv_b = (float*)c.take(E * 4);
            w.Wx = c.take((size_t)e->XP * E * esz);
            w.Wx_s = ps && e->convx ? c.take((size_t)e->XP * 2 * E * 2) : nullptr;
            w.Wdt = c.take(E * (size_t)e->Rp * esz);
            w.Wdt_s = ps && e->convx ? c.take(E * (size_t)e->Rp * 2 * 2) : nullptr;
            w.dt_bias = (float*)c.take(E * 4);
            w.A2 = (float*)c.take(E * N * 4);
            w.Dskip = (float*)c.take(E * 4);
        }
    }
}

SmallForms pcad::small_forms(const pcad_engine* e, int B, int L) {
    SmallForms f;
    if (!e->segments) return f;      // "scan_segments" 0 turns all three off: each trades a different fp32 summation order for parallelism
    f.G = scan_segments(2 * B, L, e->E, nullptr);
    f.pair = e->convx && scan_pair_wanted(2 * B, L, e->E);
    f.ksplit = e->convx ? convx_ksplit(2 * B, L, e->E, e->cfg.dtype) : 1;
    return f;
}

// Bpol: windows of the whole pcad_forward call - the small-launch forms (segmented scan, conv + x_proj K-split) are chosen for the
// call, not per chunk, so that results never depend on the chunking
Workspace pcad::carve_workspace(const pcad_engine* e, void* base, int Bc, int L, int Bpol) {
    Carver c(base);
    const size_t rows = (size_t)2 * Bc * L;
    const size_t D = e->D, E = e->E, esz = e->esz;
    Workspace w;
    const size_t Dp = fold_padded_width((int)D);       // the folded form keeps res / u Dp = round_up(D, 256) columns wide
    w.res = c.take(rows * Dp * (e->rdt == F32 ? 4 : esz));
    const bool sp = split_wanted(e);
    w.u = c.take(rows * Dp * esz);                     // split: bf16 [rows, 2D] = [hi | lo] (the same 4 D bytes per row)
    w.h = c.take(rows * D * esz);
    const size_t rows8 = (rows + 7) / 8 * 8;   // the blocked layout (x, z, xc, y): whole 8-row blocks
    // in_proj output: plain xz [rows, 2E]; or (xzsplit) x [rows8, E] in `xz` and z [rows8, E] in `zb`, both blocked
    w.xz = c.take((e->xzsplit ? rows8 : rows * 2) * E * esz);
    w.zb = e->xzsplit ? c.take(rows8 * E * esz) : nullptr;
    w.xc[0] = c.take(rows8 * E * esz);
    w.xc[1] = c.take(rows8 * E * esz);
    // dt_low (x_proj columns [0, Rp), zero padded past R); split: bf16 [rows, 2 Rp] = [hi | lo]
    const size_t dtl_bytes = sp && e->convx ? rows * e->Rp * 2 * 2 : rows * e->Rp * esz;
    w.dtl[0] = c.take(dtl_bytes);
    w.dtl[1] = c.take(dtl_bytes);
    w.bc[0] = (float*)c.take(rows * 2 * e->N * 4);   // B_t | C_t rows, fp32 (values rounded to the model dtype)
    w.bc[1] = (float*)c.take(rows * 2 * e->N * 4);
    w.y = c.take(rows8 * E * esz);
    w.ys = sp ? c.take(rows8 * 2 * E * 2) : nullptr;
    w.rstd = (float*)c.take(rows * 4);
    w.ssq = (float*)c.take(rows * (Dp / 128) * 4);
    const SmallForms f = small_forms(e, Bpol, L);
    w.seg = f.G > 1 ? (float*)c.take(scan_segment_bytes(2 * Bc, L, (int)E, 2 * Bpol)) : nullptr;
    w.pair = f.pair ? (float*)c.take(scan_pair_bytes(2 * Bc, (int)E)) : nullptr;
    // small launches: the conv + x_proj kernel splits its channel walk over several blocks per row tile ("scan_segments" 0 turns this
    // off together with the segmented scan: both trade a different fp32 summation order for parallelism on an otherwise empty chip)
    w.cxp = f.ksplit > 1 ? (float*)c.take(convx_split_bytes(2 * Bc, L, (int)E, e->cfg.dtype, e->Rp, 2 * Bpol)) : nullptr;
    // carved last, so that every other buffer sits where it does with the option off (and, like everything after h, these are dead
    // once the last out_proj has run: the heads' partials may cover them)
    w.xz2 = e->untied ? c.take((e->xzsplit ? rows8 : rows * 2) * E * esz) : nullptr;
    w.zb2 = e->untied && e->xzsplit ? c.take(rows8 * E * esz) : nullptr;
    w.bytes = c.off;
    return w;
}

static const char* const kClassNames[PCAD_NUM_KERNEL_CLASSES] = {
    "add_rmsnorm", "gemm_in_proj", "conv1d_bidir", "gemm_x_proj", "selective_scan", "gemm_out_proj", "final_head",
    "gemm_out_proj_res", "rstd_reduce"};

hipEvent_t pcad::prof_event(pcad_engine* e) {
    if (!e->prof_pool.empty()) {
        hipEvent_t ev = e->prof_pool.back();
        e->prof_pool.pop_back();
        return ev;
    }
    hipEvent_t ev = nullptr;
    if (hipEventCreate(&ev) != hipSuccess) return nullptr;
    return ev;
}

static const pcad_tensor* find(const std::map<std::string, const pcad_tensor*>& m, const std::string& k) {
    auto it = m.find(k);
    return it == m.end() ? nullptr : it->second;
}

static int64_t numel(const pcad_tensor* t) {
    int64_t n = 1;
    for (int i = 0; i < t->ndim; ++i) n *= t->shape[i];
    return n;
}

// windows per chunk for a batch of B windows of L positions: the fewest chunks within the row limit, evenly sized (no small
// tail chunk)
int pcad::chunk_for(const pcad_engine* e, int B, int L) {
    int64_t cap = chunk_row_limit(e) / (2 * (int64_t)L);
    if (e->chunk > 0 && e->chunk < cap) cap = e->chunk;
    if (cap < 1) cap = 1;
    if (cap > B) cap = B;
    if (e->ws_limit > 0 && carve_workspace(e, nullptr, (int)cap, L, B).bytes > (size_t)e->ws_limit) {
        int64_t lo = 1, hi = cap;                     // largest chunk whose workspace fits (the size is monotone in the chunk)
        while (lo < hi) {
            const int64_t mid = (lo + hi + 1) / 2;
            if (carve_workspace(e, nullptr, (int)mid, L, B).bytes <= (size_t)e->ws_limit) lo = mid; else hi = mid - 1;
        }
        cap = lo;                                     // one window always runs, whatever the limit
    }
    int64_t n = (B + cap - 1) / cap;
    // Whole rounds of the persistent GEMMs: a chunk whose token-rows are a multiple of 16 384 (64 m-tiles of 256 rows) gives every CU
    // the same number of output tiles and every XCD whole groups of the tile walk.  When the fewest-chunks split misses that (the fp32
    // model's 1 024-window batch: 3 chunks of 342 windows = 1 368 m-tiles) and a split into up to twice as many chunks hits it
    // (4 x 256 windows), take that one: +1.6 % on the fp32 + f32_gemm_split model (profiles/r06_f32_split_ab.txt r06v).  Never when
    // the caller set "chunk_seqs" / "workspace_limit_mb"; results do not depend on the chunking.
    if (e->chunk == 0 && e->ws_limit == 0) {
        auto whole = [&](int64_t m) { const int64_t c = (B + m - 1) / m; return (2 * c * (int64_t)L) % 16384 == 0; };
        if (!whole(n))
            for (int64_t m = n + 1; m <= 2 * n && m <= B; ++m)
                if (whole(m)) { n = m; break; }
    }
    return (int)((B + n - 1) / n);
}

extern "C" {

int pcad_version(void) { return PCAD_VERSION; }
const char* pcad_build_hash(void) { return PCAD_BUILD_HASH; }
const char* pcad_last_error(void) { return g_err; }

int pcad_create(const pcad_config* cfg, pcad_handle* out) {
    if (!cfg || !out) return fail(PCAD_ERR_INVALID, "pcad_create: null argument");
    if (cfg->d_state != 16) return fail(PCAD_ERR_INVALID, "d_state=%d unsupported (16 only)", cfg->d_state);
    if (cfg->d_conv != 4) return fail(PCAD_ERR_INVALID, "d_conv=%d unsupported (4 only)", cfg->d_conv);
    if (cfg->vocab != 8) return fail(PCAD_ERR_INVALID, "padded vocab=%d unsupported (8 only)", cfg->vocab);
    if (cfg->d_model <= 0 || cfg->d_model % 64 || cfg->d_model > 2048)
        return fail(PCAD_ERR_INVALID, "d_model=%d must be a multiple of 64, <= 2048", cfg->d_model);
    if (cfg->expand < 1) return fail(PCAD_ERR_INVALID, "expand=%d must be >= 1", cfg->expand);
    if (cfg->n_layer < 1) return fail(PCAD_ERR_INVALID, "n_layer=%d must be >= 1", cfg->n_layer);
    if (cfg->dt_rank < 1 || cfg->dt_rank > 256) return fail(PCAD_ERR_INVALID, "dt_rank=%d must be in 1 .. 256", cfg->dt_rank);
    if (cfg->dtype != PCAD_F32 && cfg->dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "bad dtype %d", cfg->dtype);
    for (int i = 0; i < 8; ++i)
        if (cfg->complement[i] < 0 || cfg->complement[i] > 7) return fail(PCAD_ERR_INVALID, "bad complement map");
    pcad_engine* e = new pcad_engine();
    e->cfg = *cfg;
    e->D = cfg->d_model; e->E = cfg->expand * cfg->d_model; e->N = 16; e->R = cfg->dt_rank; e->V = 8;
    e->nl = cfg->n_layer;
    e->Rp = padded_dt_rank(e->R);        // K of dt_proj: 64 up to dt_rank 64, else the next multiple of 32 (PlantCAD2 Large: 96)
    e->XP = e->Rp + 2 * e->N;            // x_proj rows: [dt (R) | 0-pad | B (16) | C (16)]
    e->esz = cfg->dtype == PCAD_BF16 ? 2 : 4;
    e->rdt = (cfg->residual_in_fp32 || cfg->dtype == PCAD_F32) ? F32 : BF16;
    const char* ck = dev_env("PCAD_CHUNK_SEQS");       // PCAD_DEV=1 only; the ABI's knob is pcad_set_option("chunk_seqs")
    // Token-rows per chunk: bounded by the kernels' unsigned 32-bit in-tensor byte offsets (rows * E * esz < 2^32 in the scan,
    // the fused conv+x_proj kernel and the 4-wave GEMM): (2^32 - 2 MiB) / (E * esz) rows = 1023 windows of 512 bp at l32 bf16
    // (30 GB of workspace), 85 windows of 8 192 bp at the l28 width.  Fewer, larger launches: 1024 windows as 4 chunks instead of
    // 16 measured +6 % (each of the 193 launches per chunk pays a fill/drain of the chip), and for long windows the chunk is what
    // sets the scan's wave count (strands x E/64): 80 windows of 8 192 bp as one chunk instead of two, +20 %.  Floor: one launch
    // of the scan should fill the chip's 4096 wave slots (2 strands x E/64 waves per window).
    e->chunk = ck ? atoi(ck) : 0;
    if (e->chunk < 0) e->chunk = 0;
    e->chunk_rows = 0;        // derived per call from the options in force: chunk_row_limit()
    // developer A/B switches (honoured only with PCAD_DEV=1): plain layouts / unfused conv
    e->blocked = dev_env("PCAD_PLAIN_LAYOUT") == nullptr && (e->E * e->esz) % 128 == 0;
    e->xzsplit = e->blocked && dev_env("PCAD_PLAIN_XZ") == nullptr && e->E % 16 == 0;
    e->convx = e->xzsplit && (e->Rp == 64 || e->Rp == 96) && dev_env("PCAD_NO_CONVX") == nullptr;
    e->gate_once = true;                  // pcad_set_option("gate_each", 1) restores the per-direction gate
    *out = e;
    return PCAD_OK;
}

void pcad_destroy(pcad_handle h) {
    if (!h) return;
    for (int c = 0; c < PCAD_NUM_KERNEL_CLASSES; ++c)
        for (auto& pr : h->prof_ev[c]) { (void)hipEventDestroy(pr.first); (void)hipEventDestroy(pr.second); }
    for (auto ev : h->prof_pool) (void)hipEventDestroy(ev);
    delete h;
}

int pcad_set_option(pcad_handle h, const char* key, int64_t value) {
    if (!h || !key) return fail(PCAD_ERR_INVALID, "pcad_set_option: null argument");
    const std::string k(key);
    if (k == "chunk_seqs") {
        if (value < 0 || value > (1 << 20)) return fail(PCAD_ERR_INVALID, "chunk_seqs=%lld out of range", (long long)value);
        h->chunk = (int)value;
    } else if (k == "gate_each") {
        h->gate_once = value == 0;
    } else if (k == "norm_fold") {
        h->norm_fold = value < 0 ? -1 : (value != 0 ? 1 : 0);
    } else if (k == "workspace_limit_mb") {
        if (value < 0 || value > ((int64_t)1 << 30)) return fail(PCAD_ERR_INVALID, "workspace_limit_mb=%lld out of range", (long long)value);
        h->ws_limit = value << 20;
    } else if (k == "f32_gemm_split") {
        h->f32_split = value != 0;
    } else if (k == "untied_directions") {
        h->untied = value != 0;
    } else if (k == "reference_order") {
        // one switch for "every rounding point where the reference has it" (BiMambaWrapper + rms_norm_fn + mamba_inner_fn):
        //   1  = gate_each 1 + norm_fold 0 (which also means no layer-0 in_proj table): only the tied out_proj fold remains
        //   2  = 1 + each direction's out_proj computed and stored in the model dtype, then summed and rounded ("add" strategy)
        //   0  = the engine's defaults
        if (value < 0 || value > 2) return fail(PCAD_ERR_INVALID, "reference_order=%lld out of range (0, 1, 2)", (long long)value);
        h->ref_order = (int)value;
        h->gate_once = value == 0;
        h->norm_fold = value == 0 ? -1 : 0;
    } else if (k == "debug_repeat_class") {
        if (value < -1 || value >= PCAD_NUM_KERNEL_CLASSES) return fail(PCAD_ERR_INVALID, "debug_repeat_class=%lld out of range", (long long)value);
        h->rep_class = (int)value;
    } else if (k == "debug_repeat") {
        if (value < 1 || value > 10000) return fail(PCAD_ERR_INVALID, "debug_repeat=%lld out of range", (long long)value);
        h->rep_count = (int)value;
    } else if (k == "poison_workspace") {
        h->poison = value != 0;
    } else if (k == "scan_segments") {
        h->segments = value != 0;
    } else if (k == "last_layer_shortcut") {
        h->shortcut = value != 0;
    } else {
        return fail(PCAD_ERR_INVALID, "pcad_set_option: unknown option '%s'", key);
    }
    return PCAD_OK;
}

int pcad_set_status_buffer(pcad_handle h, int32_t* status) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_set_status_buffer: null handle");
    if (((uintptr_t)status) % 4) return fail(PCAD_ERR_INVALID, "pcad_set_status_buffer: misaligned pointer");
    h->status = status;
    return PCAD_OK;
}

size_t pcad_weight_arena_bytes(pcad_handle h) {
    if (!h) return 0;
    pcad_engine tmp = *h;
    Carver c(nullptr);
    carve_weights(&tmp, c);
    return c.off;
}

int pcad_bind_weights(pcad_handle h, const pcad_tensor* tensors, int n, void* arena, size_t arena_bytes,
                      pcad_stream stream) {
    if (!h || !tensors || !arena) return fail(PCAD_ERR_INVALID, "pcad_bind_weights: null argument");
    if (((uintptr_t)arena) % 256) return fail(PCAD_ERR_WORKSPACE, "weight arena must be 256-byte aligned");
    if (arena_bytes < pcad_weight_arena_bytes(h))
        return fail(PCAD_ERR_WORKSPACE, "weight arena too small: %zu < %zu", arena_bytes, pcad_weight_arena_bytes(h));
    hipStream_t s = (hipStream_t)stream;
    pcad_engine* e = h;
    Carver c(arena);
    carve_weights(e, c);
    std::map<std::string, const pcad_tensor*> m;
    for (int i = 0; i < n; ++i) {
        if (!tensors[i].name || !tensors[i].data) return fail(PCAD_ERR_INVALID, "tensor %d has null name/data", i);
        if (tensors[i].dtype != PCAD_F32 && tensors[i].dtype != PCAD_BF16)
            return fail(PCAD_ERR_INVALID, "tensor %s: bad dtype", tensors[i].name);
        m[tensors[i].name] = &tensors[i];
    }
    const int D = e->D, E = e->E, N = e->N, R = e->R, Rp = e->Rp, V = e->V, dt = e->cfg.dtype;
    const std::string pre = "caduceus.backbone.";

    // missing_fmt: the entry's own PCAD_ERR_INVALID text for a tensor that only an option asks for
    auto need = [&](const std::string& k, int64_t expect, const char* missing_fmt = nullptr) -> const pcad_tensor* {
        const pcad_tensor* t = find(m, k);
        if (!t) {
            if (missing_fmt) fail(PCAD_ERR_INVALID, missing_fmt, k.c_str()); else fail(PCAD_ERR_MISSING, "missing tensor %s", k.c_str());
            return nullptr;
        }
        if (numel(t) != expect) {
            fail(PCAD_ERR_INVALID, "tensor %s has %lld elements, expected %lld", k.c_str(), (long long)numel(t),
                 (long long)expect);
            return nullptr;
        }
        return t;
    };
#define NEED(var, key, ...)                              \
    const pcad_tensor* var = need((key), __VA_ARGS__);   \
    if (!var) return g_err[0] == 'm' ? PCAD_ERR_MISSING : PCAD_ERR_INVALID

    NEED(t_emb, pre + "embeddings.word_embeddings.embedding.weight", (int64_t)V * D);
    HIP_TRY(launch_pack2d(t_emb->data, t_emb->dtype, D, e->emb, dt, D, V, D, V, D, s));
    // fp32 copy of the dtype-rounded table (what F.linear sees through the tied lm_head weight)
    HIP_TRY(launch_pack2d(e->emb, dt, D, e->emb_f32, F32, D, V, D, V, D, s));
    NEED(t_nf, pre + "norm_f.weight", (int64_t)D);
    HIP_TRY(launch_pack2d(t_nf->data, t_nf->dtype, D, e->normf_w, F32, D, 1, D, 1, D, s));
    HIP_TRY(hipMemcpyAsync(e->comp, e->cfg.complement, 8 * sizeof(int32_t), hipMemcpyHostToDevice, s));
    // the source array lives in the handle, so the async copy's host buffer stays valid

    for (int i = 0; i < e->nl; ++i) {
        LayerWeights& L = e->layers[i];
        const std::string lp = pre + "layers." + std::to_string(i) + ".";
        NEED(t_norm, lp + "norm.weight", (int64_t)D);
        HIP_TRY(launch_pack2d(t_norm->data, t_norm->dtype, D, L.norm_w, F32, D, 1, D, 1, D, s));
        const std::string mf = lp + "mixer.submodule.mamba_fwd.";
        NEED(t_in, mf + "in_proj.weight", (int64_t)2 * E * D);
        HIP_TRY(launch_pack2d(t_in->data, t_in->dtype, D, L.W_in, dt, D, 2 * E, D, 2 * E, D, s));
        if (L.W_in_f) HIP_TRY(launch_pack_scale_cols(t_in->data, t_in->dtype, D, L.norm_w, L.W_in_f, dt, D, 2 * E, D, s));
        NEED(t_out, mf + "out_proj.weight", (int64_t)D * E);
        HIP_TRY(launch_pack2d(t_out->data, t_out->dtype, E, L.W_out, dt, E, D, E, D, E, s));
        if (L.W_out_p != L.W_out) HIP_TRY(launch_pack2d(t_out->data, t_out->dtype, E, L.W_out_p, dt, E, D, E, fold_padded_width(D), E, s));
        if (L.W_in_s) HIP_TRY(launch_pack_split_w(t_in->data, t_in->dtype, D, L.W_in_s, 2 * E, D, s));
        if (L.W_out_s) HIP_TRY(launch_pack_split_w(t_out->data, t_out->dtype, E, L.W_out_s, D, E, s));
        if (e->untied) {      // mamba_rev's own in_proj / out_proj: required, not defaulted to mamba_fwd's
            const std::string mr = lp + "mixer.submodule.mamba_rev.";
            NEED(t_in_r, mr + "in_proj.weight", (int64_t)2 * E * D, "\"untied_directions\" 1 needs tensor %s");
            NEED(t_out_r, mr + "out_proj.weight", (int64_t)D * E, "\"untied_directions\" 1 needs tensor %s");
            HIP_TRY(launch_pack2d(t_in_r->data, t_in_r->dtype, D, L.W_in_r, dt, D, 2 * E, D, 2 * E, D, s));
            HIP_TRY(launch_pack2d(t_out_r->data, t_out_r->dtype, E, L.W_out_r, dt, E, D, E, D, E, s));
            if (L.W_in_s_r) HIP_TRY(launch_pack_split_w(t_in_r->data, t_in_r->dtype, D, L.W_in_s_r, 2 * E, D, s));
            if (L.W_out_s_r) HIP_TRY(launch_pack_split_w(t_out_r->data, t_out_r->dtype, E, L.W_out_s_r, D, E, s));
        }
        for (int d = 0; d < 2; ++d) {
            DirWeights& w = L.dir[d];
            const std::string mp = lp + "mixer.submodule.mamba_" + (d == 0 ? "fwd." : "rev.");
            NEED(t_cw, mp + "conv1d.weight", (int64_t)E * 4);
            HIP_TRY(launch_pack2d(t_cw->data, t_cw->dtype, 4, w.conv_w, F32, 4, E, 4, E, 4, s));
            NEED(t_cb, mp + "conv1d.bias", (int64_t)E);
            HIP_TRY(launch_pack2d(t_cb->data, t_cb->dtype, E, w.conv_b, F32, E, 1, E, 1, E, s));
            NEED(t_x, mp + "x_proj.weight", (int64_t)(R + 2 * N) * E);
            // rows [0,R) -> [0,R); zero rows [R,Rp); rows [R, R+2N) -> [Rp, Rp+2N)
            const size_t esz_src = t_x->dtype == PCAD_BF16 ? 2 : 4;
            HIP_TRY(launch_pack2d(t_x->data, t_x->dtype, E, w.Wx, dt, E, R, E, Rp, E, s));
            HIP_TRY(launch_pack2d((const char*)t_x->data + (size_t)R * E * esz_src, t_x->dtype, E,
                                  (char*)w.Wx + (size_t)Rp * E * e->esz, dt, E, 2 * N, E, 2 * N, E, s));
            if (w.Wx_s) HIP_TRY(launch_pack_convx_wsplit((const float*)w.Wx, E, w.Wx_s, e->XP, E, s));     // from the padded fp32 copy
            NEED(t_dw, mp + "dt_proj.weight", (int64_t)E * R);
            HIP_TRY(launch_pack2d(t_dw->data, t_dw->dtype, R, w.Wdt, dt, Rp, E, R, E, Rp, s));
            if (w.Wdt_s) HIP_TRY(launch_pack_split_w(w.Wdt, dt, Rp, w.Wdt_s, E, Rp, s));         // from the zero-padded fp32 copy
            NEED(t_db, mp + "dt_proj.bias", (int64_t)E);
            HIP_TRY(launch_pack2d(t_db->data, t_db->dtype, E, w.dt_bias, F32, E, 1, E, 1, E, s));
            NEED(t_A, mp + "A_log", (int64_t)E * N);
            HIP_TRY(launch_pack_A(t_A->data, t_A->dtype, w.A2, (int64_t)E * N, 1.4426950408889634f, s));
            NEED(t_D, mp + "D", (int64_t)E);
            HIP_TRY(launch_pack2d(t_D->data, t_D->dtype, E, w.Dskip, F32, E, 1, E, 1, E, s));
        }
        if ((E * e->esz) % 128 == 0)
            HIP_TRY(launch_pack_convw(L.dir[0].conv_w, L.dir[0].conv_b, L.dir[1].conv_w, L.dir[1].conv_b, L.convw, E, dt, s));
    }
#undef NEED
    // layer 0's in_proj (norm-folded form) as a table over the V token ids: emb and layer 0's folded in_proj weight are packed above
    if (e->xz_tab0) HIP_TRY(launch_embed_inproj_table(e->emb, e->layers[0].W_in_f, e->xz_tab0, V, D, 2 * E, e->cfg.eps, dt, s));
    e->fold_packed = fold_wanted(e);
    e->split_packed = split_wanted(e);
    e->untied_packed = e->untied;
    e->bound = true;
    return PCAD_OK;
}

size_t pcad_workspace_bytes(pcad_handle h, int batch, int seqlen) {
    if (!h || batch <= 0 || seqlen <= 0) return 0;
    // chunks run one after the other in ONE workspace slab
    return carve_workspace(h, nullptr, chunk_for(h, batch, seqlen), seqlen, batch).bytes;
}

int pcad_profile_enable(pcad_handle h, int on) {
    if (!h) return fail(PCAD_ERR_INVALID, "pcad_profile_enable: null handle");
    h->prof = on != 0;
    h->prof_stride = on > 1 ? on : 1;
    for (int c = 0; c < PCAD_NUM_KERNEL_CLASSES; ++c) h->prof_seen[c] = 0;
    return PCAD_OK;
}

int pcad_profile_read(pcad_handle h, pcad_kernel_stat* out, int max_out) {
    if (!h || !out) return fail(PCAD_ERR_INVALID, "pcad_profile_read: null argument");
    for (int c = 0; c < PCAD_NUM_KERNEL_CLASSES; ++c) {
        for (auto& pr : h->prof_ev[c]) {
            HIP_TRY(hipEventSynchronize(pr.second));
            float ms = 0.f;
            HIP_TRY(hipEventElapsedTime(&ms, pr.first, pr.second));
            h->prof_ms[c] += ms;
            h->prof_n[c] += 1;
            h->prof_pool.push_back(pr.first);
            h->prof_pool.push_back(pr.second);
        }
        h->prof_ev[c].clear();
    }
    int n = 0;
    for (int c = 0; c < PCAD_NUM_KERNEL_CLASSES && n < max_out; ++c, ++n) {
        snprintf(out[n].name, sizeof(out[n].name), "%s", kClassNames[c]);
        out[n].launches = h->prof_n[c];
        out[n].total_ms = h->prof_ms[c];
        h->prof_n[c] = 0;
        h->prof_ms[c] = 0.0;
    }
    return n;
}
}  // extern "C"
