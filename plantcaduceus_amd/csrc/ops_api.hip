// The per-operator entry points of libpcad.so (include/pcad.h): argument checks + the launch; nothing here touches a handle.
#include "pcad_internal.hpp"
using namespace pcad;

// what the head operators (final / pooled / loss / probs) check alike: residual layout, dtypes, shape; `who`: the entry's name
static int head_args(const char* who, int B, int L, int D, int dtype, int res_dtype, int res_fragment_layout) {
    if (res_fragment_layout && (res_dtype != PCAD_F32 || D % 256 || ((int64_t)2 * B * L) % 256))
        return fail(PCAD_ERR_INVALID, "%s: the fragment layout needs an fp32 residual, D %% 256 == 0 and 2 B L %% 256 == 0", who);
    if ((dtype != PCAD_F32 && dtype != PCAD_BF16) || (res_dtype != PCAD_F32 && res_dtype != PCAD_BF16) || (dtype == PCAD_F32 && res_dtype != PCAD_F32))
        return fail(PCAD_ERR_INVALID, "%s: bad dtype / res_dtype", who);
    if (B < 0 || L <= 0 || D <= 0 || D % 8 || D > 2048) return fail(PCAD_ERR_INVALID, "%s: bad B / L / D", who);
    return PCAD_OK;
}
// the checked arguments as the launchers' HeadInput
static HeadInput head_input(const void* h, const void* res, const float* norm_weight, int B, int L, int D, float eps, int dtype, int res_dtype,
                            int res_fragment_layout, const int32_t* ids, int32_t* status) {
    return {.h = h, .res = res, .w = norm_weight, .B = B, .L = L, .D = D, .eps = eps, .dt = dtype, .rdt = res_dtype, .res_frag = res_fragment_layout ? D : 0,
            .ids = ids, .status = status};
}

extern "C" {

int pcad_add_rmsnorm(const void* x, const void* residual_in, const float* weight, void* y, void* residual_out,
                     int64_t rows, int D, float eps, int dtype, int res_dtype, pcad_stream stream) {
    if (!x || !weight || !y) return fail(PCAD_ERR_INVALID, "pcad_add_rmsnorm: null argument");
    if (rows < 0 || D <= 0 || D % 8 || D > 2048) return fail(PCAD_ERR_INVALID, "pcad_add_rmsnorm: bad rows/D");
    HIP_TRY(launch_add_rmsnorm({.x = x, .res_in = residual_in, .w = weight, .y = y, .res_out = residual_out, .rows = rows, .D = D, .eps = eps, .dt = dtype, .rdt = res_dtype},
                               (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_causal_conv1d_silu(const void* x, int64_t ldx, const float* w_fwd, const float* b_fwd, const float* w_rev,
                            const float* b_rev, void* y_fwd, void* y_rev, int S, int L, int E, int dtype,
                            pcad_stream stream) {
    if (!x || !w_fwd || !b_fwd || !w_rev || !b_rev) return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu: null argument");
    if (S < 0 || L < 0 || E <= 0 || E % 8 || ldx < E || ldx % 8)
        return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu: bad shape (E and ldx must be multiples of 8)");
    HIP_TRY(launch_conv_bidir({.x = x, .ldx = ldx, .fwd = {.w = w_fwd, .b = b_fwd, .y = y_fwd}, .rev = {.w = w_rev, .b = b_rev, .y = y_rev},
                               .S = S, .L = L, .E = E, .dt = dtype}, (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_causal_conv1d_silu_dir(const void* x, int64_t ldx, const float* w, const float* b, void* y, int64_t ldy, int S, int L, int E,
                                int reverse, int x_blocked, int y_blocked, int dtype, pcad_stream stream) {
    if (!x || !w || !b || !y) return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu_dir: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu_dir: bad dtype");
    const int esz = dtype == PCAD_BF16 ? 2 : 4, V = 16 / esz;
    if (S < 0 || L < 0 || E <= 0 || E % V || (!x_blocked && (ldx < E || ldx % V)) || (!y_blocked && (ldy < E || ldy % V)))
        return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu_dir: bad shape (E, ldx and ldy * elem must be multiples of 16 bytes; ldx, ldy >= E)");
    if ((x_blocked || y_blocked) && ((int64_t)E * esz) % 128)
        return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu_dir: the blocked layout needs E * elem to be a multiple of 128 bytes");
    if (((uintptr_t)x) % 16 || ((uintptr_t)y) % 16 || ((uintptr_t)w) % 16)
        return fail(PCAD_ERR_INVALID, "pcad_causal_conv1d_silu_dir: x, y and w must be 16-byte aligned");
    ConvLaunch cv{.x = x, .ldx = ldx, .ldy = ldy, .S = S, .L = L, .E = E, .dt = dtype, .in_blocked = x_blocked != 0, .out_blocked = y_blocked != 0};
    ConvDirection& side = reverse ? cv.rev : cv.fwd;        // launch_conv_dir reads the side that `reverse` names
    side = {.w = w, .b = b, .y = y};
    HIP_TRY(launch_conv_dir(cv, reverse != 0, (hipStream_t)stream));
    return PCAD_OK;
}

size_t pcad_conv_xproj_scratch_bytes(int E, int dtype) {
    if (E <= 0 || (dtype != PCAD_F32 && dtype != PCAD_BF16) || (E * (dtype == PCAD_BF16 ? 2 : 4)) % 128) return 0;
    return convx_packed_bytes(E, dtype);
}

int pcad_conv_xproj_bidir(const void* x, const float* w_fwd, const float* b_fwd, const float* w_rev, const float* b_rev,
                          const void* Wx_fwd, const void* Wx_rev, void* scratch, void* xc_fwd, void* dtl_fwd,
                          float* bc_fwd, void* xc_rev, void* dtl_rev, float* bc_rev, int S, int L, int E, int Rp, int dtype,
                          pcad_stream stream) {
    if (!x || !w_fwd || !b_fwd || !w_rev || !b_rev || !Wx_fwd || !Wx_rev || !scratch || !xc_fwd || !dtl_fwd || !bc_fwd ||
        !xc_rev || !dtl_rev || !bc_rev)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir: bad dtype");
    if (Rp != 64 && Rp != 96) return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir: Rp must be 64 (dt_rank <= 64) or 96 (dt_rank 65..96)");
    const int64_t esz = dtype == PCAD_BF16 ? 2 : 4;
    if (S < 0 || L < 0 || E <= 0 || (E * esz) % 128)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir: E * elem must be a multiple of 128 bytes");
    if (((int64_t)S * L + 16) * E * esz >= ((int64_t)1 << 32))
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir: (S*L + 16) * E * elem must be < 2^32 (32-bit in-tensor offsets)");
    if (S == 0 || L == 0) return PCAD_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_pack_convw(w_fwd, b_fwd, w_rev, b_rev, (float*)scratch, E, dtype, s));
    HIP_TRY(launch_convx({.x = x, .convw = (const float*)scratch,
                          .dir = {{.Wx = Wx_fwd, .xc = xc_fwd, .dtl = dtl_fwd, .bc = bc_fwd}, {.Wx = Wx_rev, .xc = xc_rev, .dtl = dtl_rev, .bc = bc_rev}},
                          .S = S, .L = L, .E = E, .dt = dtype, .Rp = Rp}, s));
    return PCAD_OK;
}

size_t pcad_conv_xproj_split_scratch_bytes(int S, int L, int E, int dtype, int Rp, int policy_S) {
    if (S <= 0 || L <= 0 || E <= 0 || policy_S < 0 || (dtype != PCAD_F32 && dtype != PCAD_BF16) || (Rp != 64 && Rp != 96) ||
        (E * (dtype == PCAD_BF16 ? 2 : 4)) % 128)
        return 0;
    return convx_split_bytes(S, L, E, dtype, Rp, policy_S);
}

int pcad_conv_xproj_bidir_engine(const void* x, const float* w_fwd, const float* b_fwd, const float* w_rev, const float* b_rev,
                                 const void* Wx_fwd, const void* Wx_rev, void* scratch, size_t scratch_bytes, void* xc_fwd, void* dtl_fwd,
                                 float* bc_fwd, void* xc_rev, void* dtl_rev, float* bc_rev, void* part_ws, size_t part_ws_bytes,
                                 int policy_S, int dtl_split, int w_split, int S, int L, int E, int Rp, int dtype, pcad_stream stream) {
    if (!x || !w_fwd || !b_fwd || !w_rev || !b_rev || !Wx_fwd || !Wx_rev || !scratch || !xc_fwd || !dtl_fwd || !bc_fwd ||
        !xc_rev || !dtl_rev || !bc_rev)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: bad dtype");
    if (Rp != 64 && Rp != 96) return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: Rp must be 64 (dt_rank <= 64) or 96 (dt_rank 65..96)");
    if ((dtl_split || w_split) && dtype != PCAD_F32)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: dtl_split / w_split are forms of the fp32 model");
    const int64_t esz = dtype == PCAD_BF16 ? 2 : 4;
    if (S < 0 || L < 0 || E <= 0 || policy_S < 0 || (E * esz) % 128)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: E * elem must be a multiple of 128 bytes; S, L, policy_S >= 0");
    if (((int64_t)S * L + 16) * E * esz >= ((int64_t)1 << 32))
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: (S*L + 16) * E * elem must be < 2^32 (32-bit in-tensor offsets)");
    if (((uintptr_t)x) % 16 || ((uintptr_t)xc_fwd) % 16 || ((uintptr_t)xc_rev) % 16 || ((uintptr_t)dtl_fwd) % 16 || ((uintptr_t)dtl_rev) % 16 ||
        ((uintptr_t)bc_fwd) % 16 || ((uintptr_t)bc_rev) % 16 || ((uintptr_t)Wx_fwd) % 16 || ((uintptr_t)Wx_rev) % 16)
        return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: tensors must be 16-byte aligned");
    // scratch: the packed taps, then - w_split - the two [hi | lo] x_proj weights (bf16 [Rp + 32, 2E] each)
    const size_t taps = align_up(convx_packed_bytes(E, dtype)), wsb = (size_t)(Rp + 32) * 2 * E * 2;
    if (((uintptr_t)scratch) % 256 || scratch_bytes < taps + (w_split ? 2 * wsb : 0))
        return fail(PCAD_ERR_WORKSPACE, "pcad_conv_xproj_bidir_engine: scratch must be 256-byte aligned and hold the packed taps%s",
                    w_split ? " and both split x_proj weights" : "");
    if (part_ws && (((uintptr_t)part_ws) % 16 || part_ws_bytes < convx_split_bytes(S, L, E, dtype, Rp, policy_S)))
        return fail(PCAD_ERR_WORKSPACE, "pcad_conv_xproj_bidir_engine: part_ws must be 16-byte aligned and pcad_conv_xproj_split_scratch_bytes large");
    if (S == 0 || L == 0) return PCAD_OK;
    hipStream_t s = (hipStream_t)stream;
    HIP_TRY(launch_pack_convw(w_fwd, b_fwd, w_rev, b_rev, (float*)scratch, E, dtype, s));
    const void *W0 = Wx_fwd, *W1 = Wx_rev;
    if (w_split) {
        void* p0 = (char*)scratch + taps;
        void* p1 = (char*)p0 + wsb;
        HIP_TRY(launch_pack_convx_wsplit((const float*)Wx_fwd, E, p0, Rp + 32, E, s));
        HIP_TRY(launch_pack_convx_wsplit((const float*)Wx_rev, E, p1, Rp + 32, E, s));
        W0 = p0; W1 = p1;
    }
    hipError_t err = launch_convx({.x = x, .convw = (const float*)scratch,
                                   .dir = {{.Wx = W0, .xc = xc_fwd, .dtl = dtl_fwd, .bc = bc_fwd}, {.Wx = W1, .xc = xc_rev, .dtl = dtl_rev, .bc = bc_rev}},
                                   .S = S, .L = L, .E = E, .dt = dtype, .Rp = Rp, .dtl_split = dtl_split != 0, .w_split = w_split != 0,
                                   .part_ws = (float*)part_ws, .policy_S = policy_S}, s);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "pcad_conv_xproj_bidir_engine: unsupported shape / form");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_conv_xproj_bidir_engine: %s", hipGetErrorString(err));
    return PCAD_OK;
}

static int scan_args_ok(const void* u, const float* bc, const float* A, const float* Dskip, const float* delta_bias,
                        void* y, int S, int L, int E) {
    if (!u || !bc || !A || !Dskip || !delta_bias || !y) return fail(PCAD_ERR_INVALID, "pcad_selective_scan: null argument");
    if (S < 0 || L < 0 || E <= 0 || E % 64) return fail(PCAD_ERR_INVALID, "pcad_selective_scan: E must be a multiple of 64");
    if (((uintptr_t)bc) % 16) return fail(PCAD_ERR_INVALID, "pcad_selective_scan: bc must be 16-byte aligned");
    return PCAD_OK;
}

int pcad_selective_scan(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc, const float* A,
                        const float* Dskip, const float* delta_bias, void* y, int S, int L, int E, int reverse,
                        int accumulate, int dtype, pcad_stream stream) {
    if (!delta) return fail(PCAD_ERR_INVALID, "pcad_selective_scan: null delta");
    if (int rc = scan_args_ok(u, bc, A, Dskip, delta_bias, y, S, L, E)) return rc;
    if (S == 0 || L == 0) return PCAD_OK;
    // raw A is scaled by log2(e) when the kernel loads it into registers (the engine passes pre-scaled A)
    HIP_TRY(launch_scan({.dir = {.u = u, .bc = bc, .A2 = A, .Dskip = Dskip, .dbias = delta_bias}, .delta = delta, .z = z, .ldz = ldz,
                         .a_scale = 1.4426950408889634f, .y = y, .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0, .accumulate = accumulate},
                        (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_selective_scan_dtproj(const void* u, const void* dt_low, int64_t lddt, const void* Wdt, int Rp, const void* z,
                               int64_t ldz, const float* bc, const float* A, const float* Dskip,
                               const float* delta_bias, void* y, int S, int L, int E, int reverse, int accumulate,
                               int dtype, pcad_stream stream) {
    if (!dt_low || !Wdt) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_dtproj: null dt_low / Wdt");
    if (Rp <= 0 || Rp % 32 || lddt < Rp || ((uintptr_t)dt_low) % 16 || ((uintptr_t)Wdt) % 16 ||
        (lddt * (dtype == PCAD_BF16 ? 2 : 4)) % 16)
        return fail(PCAD_ERR_INVALID, "pcad_selective_scan_dtproj: Rp must be a multiple of 32 (zero padded), rows 16-byte aligned");
    if (int rc = scan_args_ok(u, bc, A, Dskip, delta_bias, y, S, L, E)) return rc;
    if (S == 0 || L == 0) return PCAD_OK;
    HIP_TRY(launch_scan({.dir = {.u = u, .dt_low = dt_low, .Wdt = Wdt, .bc = bc, .A2 = A, .Dskip = Dskip, .dbias = delta_bias}, .z = z, .ldz = ldz,
                         .lddt = lddt, .Rp = Rp, .a_scale = 1.4426950408889634f, .y = y, .S = S, .L = L, .E = E, .dt = dtype,
                         .reverse = reverse != 0, .accumulate = accumulate},
                        (hipStream_t)stream));
    return PCAD_OK;
}

size_t pcad_scan_segment_scratch_bytes(int S, int L, int E, int policy_S) {
    if (S <= 0 || L <= 0 || E <= 0 || E % 64 || policy_S < 0) return 0;
    return scan_segment_bytes(S, L, E, policy_S);
}

size_t pcad_scan_pair_scratch_bytes(int S, int E) {
    if (S <= 0 || E <= 0 || E % 64) return 0;
    return scan_pair_bytes(S, E);
}

// what the two engine-form scan entries check alike: dtype, shape, the fused dt_proj operand's rows
static int scan_engine_args(const char* who, int S, int L, int E, int Rp, int64_t lddt, int dt_split, int dtype) {
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype", who);
    if (S < 0 || L < 0 || E <= 0 || E % 64) return fail(PCAD_ERR_INVALID, "%s: E must be a multiple of 64; S, L >= 0", who);
    if (dt_split && dtype != PCAD_F32) return fail(PCAD_ERR_INVALID, "%s: dt_split is a form of the fp32 model", who);
    const int64_t desz = dtype == PCAD_BF16 || dt_split ? 2 : 4;       // dt_low / Wdt elements
    if (Rp <= 0 || Rp % 32 || lddt < (dt_split ? 2 : 1) * (int64_t)Rp || (lddt * desz) % 16)
        return fail(PCAD_ERR_INVALID, "%s: Rp must be a multiple of 32 (zero padded), lddt >= Rp (dt_split: 2 Rp), rows 16-byte aligned", who);
    return PCAD_OK;
}

int pcad_selective_scan_engine(const void* u, const void* dt_low, int64_t lddt, const void* Wdt, int Rp, const void* z, const float* bc,
                               const float* A2, float a_scale, const float* Dskip, const float* delta_bias, void* y, void* ysplit,
                               void* seg_ws, size_t seg_ws_bytes, int policy_S, int walk_len, int dt_split, int S, int L, int E,
                               int reverse, int accumulate, int dtype, pcad_stream stream) {
    if (!u || !dt_low || !Wdt || !bc || !A2 || !Dskip || !delta_bias || !y) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_engine: null argument");
    if (int rc = scan_engine_args("pcad_selective_scan_engine", S, L, E, Rp, lddt, dt_split, dtype)) return rc;
    if (accumulate < 0 || accumulate > 2 || (accumulate == 2 && !z)) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_engine: accumulate must be 0, 1 or 2 (2 needs z)");
    if (policy_S < 0 || walk_len < 0 || walk_len % 8)
        return fail(PCAD_ERR_INVALID, "pcad_selective_scan_engine: walk_len must be a whole number of 8-step groups; policy_S >= 0");
    if (((uintptr_t)u) % 16 || ((uintptr_t)y) % 16 || ((uintptr_t)z) % 16 || ((uintptr_t)ysplit) % 16 || ((uintptr_t)dt_low) % 16 ||
        ((uintptr_t)Wdt) % 16 || ((uintptr_t)bc) % 16 || ((uintptr_t)A2) % 16)
        return fail(PCAD_ERR_INVALID, "pcad_selective_scan_engine: tensors must be 16-byte aligned");
    if (seg_ws && (((uintptr_t)seg_ws) % 16 || seg_ws_bytes < scan_segment_bytes(S, L, E, policy_S)))
        return fail(PCAD_ERR_WORKSPACE, "pcad_selective_scan_engine: seg_ws must be 16-byte aligned and pcad_scan_segment_scratch_bytes large");
    hipError_t err = launch_scan({.dir = {.u = u, .dt_low = dt_low, .Wdt = Wdt, .bc = bc, .A2 = A2, .Dskip = Dskip, .dbias = delta_bias}, .z = z, .ldz = E,
                                  .lddt = lddt, .Rp = Rp, .a_scale = a_scale, .y = y, .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0,
                                  .accumulate = accumulate, .uy_blocked = true, .z_blocked = true, .seg_ws = (float*)seg_ws, .walk_len = walk_len,
                                  .ysplit = ysplit, .dt_split = dt_split != 0, .policy_S = policy_S},
                                 (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_engine: unsupported shape / form (see include/pcad.h)");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_selective_scan_engine: %s", hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_selective_scan_pair(const void* u_fwd, const void* dt_low_fwd, const void* Wdt_fwd, const float* bc_fwd, const float* A2_fwd,
                             const float* Dskip_fwd, const float* delta_bias_fwd, const void* u_rev, const void* dt_low_rev,
                             const void* Wdt_rev, const float* bc_rev, const float* A2_rev, const float* Dskip_rev,
                             const float* delta_bias_rev, const void* z, int64_t lddt, int Rp, void* y, void* ysplit, void* ws,
                             size_t ws_bytes, int S, int L, int E, int gate_each, int phases, int dt_split, int dtype, pcad_stream stream) {
    if (!u_fwd || !dt_low_fwd || !Wdt_fwd || !bc_fwd || !A2_fwd || !Dskip_fwd || !delta_bias_fwd || !u_rev || !dt_low_rev || !Wdt_rev ||
        !bc_rev || !A2_rev || !Dskip_rev || !delta_bias_rev || !z || !y || !ws)
        return fail(PCAD_ERR_INVALID, "pcad_selective_scan_pair: null argument");
    if (int rc = scan_engine_args("pcad_selective_scan_pair", S, L, E, Rp, lddt, dt_split, dtype)) return rc;
    if (ysplit && dtype != PCAD_F32) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_pair: ysplit is a form of the fp32 model");
    if (phases < 1 || phases > 3) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_pair: phases must be 1, 2 or 3");
    const void* al[] = {u_fwd, dt_low_fwd, Wdt_fwd, bc_fwd, A2_fwd, u_rev, dt_low_rev, Wdt_rev, bc_rev, A2_rev, z, y, ysplit};
    for (const void* p : al)
        if (((uintptr_t)p) % 16) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_pair: tensors must be 16-byte aligned");
    if (((uintptr_t)ws) % 16 || ws_bytes < scan_pair_bytes(S, E))
        return fail(PCAD_ERR_WORKSPACE, "pcad_selective_scan_pair: ws must be 16-byte aligned and pcad_scan_pair_scratch_bytes large");
    hipError_t err = launch_scan_pair({.fwd = {.u = u_fwd, .dt_low = dt_low_fwd, .Wdt = Wdt_fwd, .bc = bc_fwd, .A2 = A2_fwd, .Dskip = Dskip_fwd, .dbias = delta_bias_fwd},
                                       .rev = {.u = u_rev, .dt_low = dt_low_rev, .Wdt = Wdt_rev, .bc = bc_rev, .A2 = A2_rev, .Dskip = Dskip_rev, .dbias = delta_bias_rev},
                                       .z = z, .lddt = lddt, .Rp = Rp, .y = y, .S = S, .L = L, .E = E, .dt = dtype, .gate_each = gate_each != 0,
                                       .ws = (float*)ws, .ysplit = ysplit, .dt_split = dt_split != 0, .phases = phases},
                                      (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_pair: unsupported shape (L %% 64 == 0; bf16: Rp 64 or 96; see include/pcad.h)");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_selective_scan_pair: %s", hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_gemm_nt(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int N, int K,
                 int dtype, int out_dtype, pcad_stream stream) {
    if (!A || !W || !C) return fail(PCAD_ERR_INVALID, "pcad_gemm_nt: null argument");
    hipError_t err = launch_gemm_nt({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype}, {.C = C, .ldc = ldc, .out_dt = out_dtype},
                                    (hipStream_t)stream);
    if (err == hipErrorInvalidValue)
        return fail(PCAD_ERR_INVALID, "pcad_gemm_nt: K*elem must be a multiple of 128 bytes; A/W 16-byte aligned rows");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_gemm_nt: %s", hipGetErrorString(err));
    return PCAD_OK;
}

size_t pcad_gemm_nt_split_scratch_bytes(int64_t M, int N, int K) {
    if (M <= 0 || N <= 0 || K <= 0) return 0;
    return align_up((size_t)M * 2 * K * 2) + align_up((size_t)N * 2 * K * 2);       // bf16 [M, 2K] = [hi | lo] of A, bf16 [N, 2K] of W
}

int pcad_gemm_nt_split(const float* A, int64_t lda, const float* W, int64_t ldw, float* C, int64_t ldc, int64_t M, int N, int K,
                       void* scratch, size_t scratch_bytes, pcad_stream stream) {
    if (!A || !W || !C || !scratch) return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_split: null argument");
    if (M < 0 || N <= 0 || K <= 0 || K % 64 || lda < K || ldw < K || ldc < N)
        return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_split: K must be a multiple of 64; lda, ldw >= K; ldc >= N");
    if (((uintptr_t)scratch) % 256 || scratch_bytes < pcad_gemm_nt_split_scratch_bytes(M, N, K))
        return fail(PCAD_ERR_WORKSPACE, "pcad_gemm_nt_split: scratch must be 256-byte aligned and pcad_gemm_nt_split_scratch_bytes large");
    if (M == 0) return PCAD_OK;
    hipStream_t s = (hipStream_t)stream;
    void* As = scratch;
    void* Ws = (char*)scratch + align_up((size_t)M * 2 * K * 2);
    HIP_TRY(launch_split_rows(A, lda, As, M, K, false, false, s));                // [hi | lo]
    HIP_TRY(launch_pack_split_w(W, PCAD_F32, ldw, Ws, N, K, s));                  // [hi | lo]
    // 3 K / 64 K-tiles, the cursor wrapping around both operands: a_hi w_hi + a_lo w_hi + a_hi w_lo
    hipError_t err = launch_gemm_nt({.A = As, .lda = 2 * (int64_t)K, .W = Ws, .ldw = 2 * (int64_t)K, .M = M, .N = N, .K = 3 * K, .dt = BF16, .ksplit = K / 64},
                                    {.C = C, .ldc = ldc, .out_dt = F32}, s);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_gemm_nt_split: %s", hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_gemm_nt_residual(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, float* res, float* ssq, int64_t M, int N,
                          int K, int dtype, pcad_stream stream) {
    if (!A || !W || !res || !ssq || !C) return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_residual: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_residual: bad dtype");
    if (M < 0 || N <= 0 || K <= 0 || M % 256 || N % 256 || M * (int64_t)N * 4 >= ((int64_t)1 << 32))
        return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_residual: M and N must be multiples of 256 and M * N * 4 < 2^32");
    hipError_t err = launch_gemm_nt_res({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype}, {.C = C, .res = res, .ssq = ssq},
                                        (hipStream_t)stream);
    if (err == hipErrorInvalidValue)
        return fail(PCAD_ERR_INVALID, "pcad_gemm_nt_residual: K*elem must be a multiple of 128 bytes; 16-byte aligned rows; tensors < 4 GiB");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_gemm_nt_residual: %s", hipGetErrorString(err));
    return PCAD_OK;
}

// ---- the GEMM launch forms of the engine (csrc/forward.hip) as operators: pcad.h "engine forms of the GEMMs" --------------------------
// what the four entries check alike: dtype, shape, rows that hold the operand, 16-byte alignment.  ksplit: A and W are bf16 [hi | lo]
// tensors of 2 K / 3 columns.  -> the operands, or a PCAD_ERR_INVALID
static int gemm_engine_args(const char* who, const void* A, int64_t lda, const void* W, int64_t ldw, int64_t M, int N, int K, int a_blocked,
                            int ksplit, int dtype) {
    if (!A || !W) return fail(PCAD_ERR_INVALID, "%s: null argument", who);
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype", who);
    const int64_t esz = dtype == PCAD_BF16 ? 2 : 4;
    if (M < 0 || N <= 0 || K <= 0 || ksplit < 0 || (K * esz) % 128) return fail(PCAD_ERR_INVALID, "%s: K * elem must be a multiple of 128 bytes; M >= 0, N > 0, ksplit >= 0", who);
    const int64_t cols = ksplit ? 2 * (int64_t)ksplit * 64 : K;                        // columns the cursor reads of either operand
    if (lda < cols || ldw < cols || (lda * esz) % 16 || (ldw * esz) % 16 || (a_blocked && (lda * esz) % 128))
        return fail(PCAD_ERR_INVALID, "%s: lda, ldw must hold the operand's columns in 16-byte aligned rows (blocked A: lda * elem a multiple of 128 bytes)", who);
    if (((uintptr_t)A) % 16 || ((uintptr_t)W) % 16) return fail(PCAD_ERR_INVALID, "%s: A and W must be 16-byte aligned", who);
    return PCAD_OK;
}

static int gemm_engine_result(const char* who, hipError_t err) {
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: unsupported shape / form (see include/pcad.h)", who);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_gemm_nt_engine(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, int64_t M, int N, int K, int a_blocked,
                        int ksplit, int dtype, int out_dtype, pcad_stream stream) {
    const char* who = "pcad_gemm_nt_engine";
    if (!C) return fail(PCAD_ERR_INVALID, "%s: null argument", who);
    if (int rc = gemm_engine_args(who, A, lda, W, ldw, M, N, K, a_blocked, ksplit, dtype)) return rc;
    if (out_dtype != PCAD_F32 && out_dtype != dtype) return fail(PCAD_ERR_INVALID, "%s: out_dtype must be PCAD_F32 or dtype", who);
    if (ldc < N || (ldc * (out_dtype == PCAD_BF16 ? 2 : 4)) % 16 || ((uintptr_t)C) % 16)
        return fail(PCAD_ERR_INVALID, "%s: ldc >= N; C in 16-byte aligned rows", who);
    return gemm_engine_result(who, launch_gemm_nt({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype, .a_blocked = a_blocked != 0, .ksplit = ksplit},
                                                  {.C = C, .ldc = ldc, .out_dt = out_dtype}, (hipStream_t)stream));
}

int pcad_gemm_nt_xproj(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, int64_t ldc, float* C2, int64_t ldc2, int nsplit,
                       int64_t M, int N, int K, int a_blocked, int ksplit, int dtype, pcad_stream stream) {
    const char* who = "pcad_gemm_nt_xproj";
    if (!C || !C2) return fail(PCAD_ERR_INVALID, "%s: null argument", who);
    if (int rc = gemm_engine_args(who, A, lda, W, ldw, M, N, K, a_blocked, ksplit, dtype)) return rc;
    const int64_t esz = dtype == PCAD_BF16 ? 2 : 4;
    if (nsplit <= 0 || nsplit >= N || nsplit % 16 || (N - nsplit) % 16 || ldc < nsplit || ldc2 < N - nsplit)
        return fail(PCAD_ERR_INVALID, "%s: 0 < nsplit < N, both in whole 16-column groups; ldc >= nsplit, ldc2 >= N - nsplit", who);
    if ((ldc * esz) % 16 || (ldc2 * 4) % 16 || ((uintptr_t)C) % 16 || ((uintptr_t)C2) % 16)
        return fail(PCAD_ERR_INVALID, "%s: C and C2 in 16-byte aligned rows", who);
    return gemm_engine_result(who, launch_gemm_nt_split({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype, .a_blocked = a_blocked != 0, .ksplit = ksplit},
                                                        {.C = C, .ldc = ldc, .C2 = C2, .ldc2 = ldc2, .nsplit = nsplit}, (hipStream_t)stream));
}

int pcad_gemm_nt_two(const void* A, int64_t lda, const void* W, int64_t ldw, void* C1, void* C2, int nsplit, const float* rscale, int64_t M,
                     int N, int K, int a_blocked, int out_blocked, int ksplit, int dtype, int out_dtype, pcad_stream stream) {
    const char* who = "pcad_gemm_nt_two";
    if (!C1 || !C2) return fail(PCAD_ERR_INVALID, "%s: null argument", who);
    if (int rc = gemm_engine_args(who, A, lda, W, ldw, M, N, K, a_blocked, ksplit, dtype)) return rc;
    if (out_dtype != PCAD_F32 && out_dtype != dtype) return fail(PCAD_ERR_INVALID, "%s: out_dtype must be PCAD_F32 or dtype", who);
    if (nsplit <= 0 || nsplit >= N || nsplit % 16 || N % 16) return fail(PCAD_ERR_INVALID, "%s: 0 < nsplit < N, both multiples of 16", who);
    if (((uintptr_t)C1) % 16 || ((uintptr_t)C2) % 16 || ((uintptr_t)rscale) % 4) return fail(PCAD_ERR_INVALID, "%s: C1 and C2 must be 16-byte aligned", who);
    return gemm_engine_result(who, launch_gemm_nt_two({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype, .a_blocked = a_blocked != 0, .ksplit = ksplit},
                                                      {.C1 = C1, .C2 = C2, .nsplit = nsplit, .out_blocked = out_blocked != 0, .rscale = rscale, .out_dt = out_dtype},
                                                      (hipStream_t)stream));
}

int pcad_gemm_nt_residual_engine(const void* A, int64_t lda, const void* W, int64_t ldw, void* C, float* res, float* ssq, int64_t M, int N,
                                 int K, int a_blocked, int ksplit, int dtype, pcad_stream stream) {
    const char* who = "pcad_gemm_nt_residual_engine";
    if (!C || !res || !ssq) return fail(PCAD_ERR_INVALID, "%s: null argument", who);
    if (int rc = gemm_engine_args(who, A, lda, W, ldw, M, N, K, a_blocked, ksplit, dtype)) return rc;
    if (M % 256 || N % 256 || M * (int64_t)N * 4 >= ((int64_t)1 << 32))
        return fail(PCAD_ERR_INVALID, "%s: M and N must be multiples of 256 and M * N * 4 < 2^32", who);
    if (((uintptr_t)C) % 16 || ((uintptr_t)res) % 16 || ((uintptr_t)ssq) % 4) return fail(PCAD_ERR_INVALID, "%s: C and res must be 16-byte aligned", who);
    return gemm_engine_result(who, launch_gemm_nt_res({.A = A, .lda = lda, .W = W, .ldw = ldw, .M = M, .N = N, .K = K, .dt = dtype, .a_blocked = a_blocked != 0, .ksplit = ksplit},
                                                      {.C = C, .res = res, .ssq = ssq}, (hipStream_t)stream));
}

int pcad_gather_rows(const void* src, void* out, int B, int L, int E, const int32_t* positions, int P, int dtype, pcad_stream stream) {
    if (!src || !out) return fail(PCAD_ERR_INVALID, "pcad_gather_rows: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_gather_rows: bad dtype");
    if (B < 0 || L <= 0 || E <= 0 || (E * (dtype == PCAD_BF16 ? 2 : 4)) % 16 || P < 1)
        return fail(PCAD_ERR_INVALID, "pcad_gather_rows: bad shape (E * elem must be a multiple of 16 bytes, P >= 1)");
    Positions pos;
    if (int rc = positions_arg("pcad_gather_rows", positions, P, L, &pos)) return rc;
    if (B == 0) return PCAD_OK;
    HIP_TRY(launch_gather_rows({.src = src, .out = out, .B = B, .L = L, .E = E, .pos = pos, .dt = dtype}, (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_layer_rows(const void* src, void* out, int B, int L, int D, const int32_t* positions, int P, const int32_t* pos_per_window,
                    int assembled, int average, int32_t* status, int dtype, pcad_stream stream) {
    if (!src || !out) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: null argument");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: bad dtype");
    if (B < 0 || L <= 0 || D <= 0 || D % 8) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: bad B / L / D (D must be a multiple of 8)");
    if (((uintptr_t)src) % 16 || ((uintptr_t)out) % 16) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: src and out must be 16-byte aligned");
    if ((positions != nullptr) == (pos_per_window != nullptr)) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: exactly one of positions and pos_per_window");
    if (P < 1) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: bad positions (P=%d)", P);
    Positions pos;
    if (int rc = positions_arg("pcad_layer_rows", pos_per_window ? nullptr : positions, pos_per_window ? 0 : P, L, &pos)) return rc;
    if (P > PCAD_MAX_POSITIONS) return fail(PCAD_ERR_INVALID, "pcad_layer_rows: bad positions (P=%d)", P);
    if (B == 0) return PCAD_OK;
    HIP_TRY(launch_layer_rows({.src = src, .out = out, .B = B, .L = L, .D = D, .dt = dtype, .pos = pos, .pos_per_window = assembled ? nullptr : pos_per_window, .P = P,
                               .assembled = assembled != 0, .sb = P, .sq = 1, .average = average != 0, .status = status}, (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_final_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                    void* hidden_out, float* logits_out, int B, int L, int D, float eps, const int32_t* positions, int P,
                    const int32_t* pos_per_seq, int h_compact, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                    int res_fragment_layout, pcad_stream stream) {
    if (!h || !res || !norm_weight || !emb_f32 || !complement) return fail(PCAD_ERR_INVALID, "pcad_final_head: null argument");
    if (int rc = head_args("pcad_final_head", B, L, D, dtype, res_dtype, res_fragment_layout)) return rc;
    if (pos_per_seq && (positions || P)) return fail(PCAD_ERR_INVALID, "pcad_final_head: positions and pos_per_seq are exclusive");
    if (h_compact && (pos_per_seq || P == 0)) return fail(PCAD_ERR_INVALID, "pcad_final_head: h_compact needs a shared list of positions");
    Positions pos;
    if (int rc = positions_arg("pcad_final_head", positions, P, L, &pos)) return rc;
    if (B == 0) return PCAD_OK;
    HIP_TRY(launch_final_head({.in = head_input(h, res, norm_weight, B, L, D, eps, dtype, res_dtype, res_fragment_layout, ids, status), .emb_f32 = emb_f32,
                               .comp8 = complement, .hidden_out = hidden_out, .logits_out = logits_out, .pos = pos, .pos_per_seq = pos_per_seq,
                               .h_compact = h_compact != 0}, (hipStream_t)stream));
    return PCAD_OK;
}

size_t pcad_pooled_head_scratch_bytes(int B, int L, int D, int pooling) {
    if (B <= 0 || L <= 0 || D <= 0 || pooling < PCAD_POOL_MEAN || pooling > PCAD_POOL_LAST) return 0;
    return align_up(pool_partial_bytes(B, L, D, pooling));
}

int pcad_pooled_head(const void* h, const void* res, const float* norm_weight, const float* score_w, int num_labels,
                     float* pooled_out, float* logits_out, int B, int L, int D, float eps, int pooling, const int32_t* ids,
                     int32_t* status, int dtype, int res_dtype, int res_fragment_layout, void* scratch, size_t scratch_bytes,
                     pcad_stream stream) {
    if (!h || !res || !norm_weight || !scratch) return fail(PCAD_ERR_INVALID, "pcad_pooled_head: null argument");
    if (!pooled_out && !logits_out) return fail(PCAD_ERR_INVALID, "pcad_pooled_head: no output requested");
    if (logits_out && (!score_w || num_labels < 1 || num_labels > PCAD_MAX_LABELS))
        return fail(PCAD_ERR_INVALID, "pcad_pooled_head: logits need score_w and 1 <= num_labels <= %d", PCAD_MAX_LABELS);
    if (pooling < PCAD_POOL_MEAN || pooling > PCAD_POOL_LAST) return fail(PCAD_ERR_INVALID, "pcad_pooled_head: bad pooling %d", pooling);
    if (int rc = head_args("pcad_pooled_head", B, L, D, dtype, res_dtype, res_fragment_layout)) return rc;
    if (B == 0) return PCAD_OK;
    if (((uintptr_t)scratch) % 256 || scratch_bytes < pcad_pooled_head_scratch_bytes(B, L, D, pooling))
        return fail(PCAD_ERR_WORKSPACE, "pcad_pooled_head: scratch must be 256-byte aligned and pcad_pooled_head_scratch_bytes large");
    HIP_TRY(launch_pooled_head({.in = head_input(h, res, norm_weight, B, L, D, eps, dtype, res_dtype, res_fragment_layout, ids, status), .score_w = score_w,
                                .NL = num_labels, .pooled_out = pooled_out, .logits_out = logits_out, .pooling = pooling, .part = scratch}, (hipStream_t)stream));
    return PCAD_OK;
}

size_t pcad_loss_head_scratch_bytes(int B, int L) {
    if (B <= 0 || L <= 0) return 0;
    return align_up(loss_partial_bytes(B, L));
}

int pcad_loss_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                   const int32_t* labels, const float* loss_weights, int ignore_index, float* sums_out, float* nll_out,
                   float* logits_out, int B, int L, int D, float eps, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                   int res_fragment_layout, void* scratch, size_t scratch_bytes, pcad_stream stream) {
    if (!h || !res || !norm_weight || !emb_f32 || !complement || !labels || !sums_out || !scratch)
        return fail(PCAD_ERR_INVALID, "pcad_loss_head: null argument");
    if (int rc = head_args("pcad_loss_head", B, L, D, dtype, res_dtype, res_fragment_layout)) return rc;
    if (B == 0) return PCAD_OK;
    if (((uintptr_t)scratch) % 256 || scratch_bytes < pcad_loss_head_scratch_bytes(B, L))
        return fail(PCAD_ERR_WORKSPACE, "pcad_loss_head: scratch must be 256-byte aligned and pcad_loss_head_scratch_bytes large");
    HIP_TRY(launch_loss_head({.in = head_input(h, res, norm_weight, B, L, D, eps, dtype, res_dtype, res_fragment_layout, ids, status), .emb_f32 = emb_f32,
                              .comp8 = complement, .labels = labels, .loss_w = loss_weights, .ignore_index = ignore_index, .sums_out = sums_out, .nll_out = nll_out,
                              .logits_out = logits_out, .part = scratch}, (hipStream_t)stream));
    return PCAD_OK;
}

int pcad_probs_head(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                    const int32_t* cols, float* probs_out, float* logits_out, int B, int L, int D, float eps, const int32_t* positions,
                    int P, const int32_t* pos_per_window, int h_compact, const int32_t* ids, int32_t* status, int dtype, int res_dtype,
                    int res_fragment_layout, pcad_stream stream) {
    if (!h || !res || !norm_weight || !emb_f32 || !complement) return fail(PCAD_ERR_INVALID, "pcad_probs_head: null argument");
    if (!probs_out && !logits_out) return fail(PCAD_ERR_INVALID, "pcad_probs_head: no output requested");
    if (((uintptr_t)probs_out) % 16) return fail(PCAD_ERR_INVALID, "pcad_probs_head: probs_out must be 16-byte aligned");
    if (int rc = head_args("pcad_probs_head", B, L, D, dtype, res_dtype, res_fragment_layout)) return rc;
    if (positions && pos_per_window) return fail(PCAD_ERR_INVALID, "pcad_probs_head: positions and pos_per_window are exclusive");
    if (P < 0 || P > PCAD_MAX_POSITIONS || (P > 0 && !positions && !pos_per_window) || (P == 0 && (positions || pos_per_window)))
        return fail(PCAD_ERR_INVALID, "pcad_probs_head: bad positions (P=%d)", P);
    if (h_compact && (pos_per_window || P == 0)) return fail(PCAD_ERR_INVALID, "pcad_probs_head: h_compact needs a shared list of positions");
    ProbCols pc;
    if (int rc = probs_cols_arg("pcad_probs_head", cols, PCAD_MAX_VOCAB, &pc)) return rc;
    Positions pos;
    if (int rc = positions_arg("pcad_probs_head", pos_per_window ? nullptr : positions, pos_per_window ? 0 : P, L, &pos)) return rc;
    if (B == 0) return PCAD_OK;
    HIP_TRY(launch_probs_head({.in = head_input(h, res, norm_weight, B, L, D, eps, dtype, res_dtype, res_fragment_layout, ids, status), .emb_f32 = emb_f32,
                               .comp8 = complement, .cols = pc, .probs_out = probs_out, .logits_out = logits_out, .pos = pos, .pos_per_window = pos_per_window,
                               .Pw = pos_per_window ? P : 0, .h_compact = h_compact != 0}, (hipStream_t)stream));
    return PCAD_OK;
}

}  // extern "C"
