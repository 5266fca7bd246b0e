// The entry points of libpcad_bwd.so (include/pcad_bwd.h): argument checks + the launch.  The library links libpcad.so and reports
// through its pcad::fail, so pcad_last_error() of the calling thread carries the message.
#include "../../include/pcad_bwd.h"
#include "pcad_internal.hpp"
#include <math.h>
#include <string.h>
using namespace pcad;

extern "C" {

size_t pcad_causal_conv1d_silu_bwd_scratch_bytes(int S, int L, int E) {
    if (S <= 0 || L <= 0 || E <= 0) return 0;
    return conv_bwd_bytes(S, L, E);
}

int pcad_causal_conv1d_silu_bwd(const void* x, int64_t ldx, const float* w, const float* b, const void* dout, void* dx, float* dw, float* db,
                                void* scratch, size_t scratch_bytes, int S, int L, int E, int reverse, int dtype, pcad_stream stream) {
    const char* who = "pcad_causal_conv1d_silu_bwd";
    const struct { const void* p; const char* name; } req[] = {{x, "x"}, {w, "w"}, {b, "b"}, {dout, "dout"}, {dx, "dx"}, {dw, "dw"}, {db, "db"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    const int V = dtype == PCAD_BF16 ? 8 : 4;
    if (S < 0 || L < 0) return fail(PCAD_ERR_INVALID, "%s: S, L must be >= 0 (S=%d, L=%d)", who, S, L);
    if (E <= 0 || E % V) return fail(PCAD_ERR_INVALID, "%s: E must be a positive multiple of 16 bytes = %d elements (E=%d)", who, V, E);
    if (ldx < E) return fail(PCAD_ERR_INVALID, "%s: ldx must be >= E (ldx=%lld, E=%d)", who, (long long)ldx, E);
    if (ldx % V) return fail(PCAD_ERR_INVALID, "%s: ldx must be a multiple of 16 bytes = %d elements (ldx=%lld)", who, V, (long long)ldx);
    const struct { const void* p; const char* name; } al[] = {{x, "x"}, {dout, "dout"}, {dx, "dx"}, {w, "w"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (S == 0 || L == 0) return PCAD_OK;
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < conv_bwd_bytes(S, L, E))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_causal_conv1d_silu_bwd_scratch_bytes large", who);
    hipError_t err = launch_conv_bwd({.x = x, .ldx = ldx, .w = w, .b = b, .dout = dout, .dx = dx, .dw = dw, .db = db, .scratch = scratch,
                                      .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0},
                                     (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: S * ceil(L / 64) * E / %d lanes must fit a 32-bit grid of 256-lane blocks", who, V);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

size_t pcad_add_rmsnorm_bwd_scratch_bytes(int64_t rows, int D) {
    if (rows <= 0 || D <= 0) return 0;
    return norm_bwd_bytes(rows, D);
}

int pcad_add_rmsnorm_bwd(const void* x, const void* residual_in, const float* weight, const void* dy, const void* dresidual_out, void* dx,
                         void* dresidual_in, float* dweight, void* scratch, size_t scratch_bytes, int64_t rows, int D, float eps, int dtype,
                         int res_dtype, pcad_stream stream) {
    const char* who = "pcad_add_rmsnorm_bwd";
    const struct { const void* p; const char* name; } req[] = {{x, "x"}, {weight, "weight"}, {dy, "dy"}, {dx, "dx"}, {dweight, "dweight"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if ((residual_in != nullptr) != (dresidual_in != nullptr))
        return fail(PCAD_ERR_INVALID, "%s: dresidual_in is required exactly when residual_in is given (residual_in %s, dresidual_in %s)", who,
                    residual_in ? "given" : "NULL", dresidual_in ? "given" : "NULL");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (res_dtype != PCAD_F32 && !(res_dtype == PCAD_BF16 && dtype == PCAD_BF16))
        return fail(PCAD_ERR_INVALID, "%s: bad res_dtype %d for dtype %d (BF16 / F32, BF16 / BF16 or F32 / F32)", who, res_dtype, dtype);
    if (rows < 0) return fail(PCAD_ERR_INVALID, "%s: rows must be >= 0", who);
    if (D <= 0 || D % 8) return fail(PCAD_ERR_INVALID, "%s: D must be a positive multiple of 8 (D=%d)", who, D);
    if (D > 2048) return fail(PCAD_ERR_INVALID, "%s: D must be <= 2048 (D=%d)", who, D);
    const struct { const void* p; const char* name; } al[] = {{x, "x"}, {residual_in, "residual_in"}, {weight, "weight"}, {dy, "dy"},
                                                              {dresidual_out, "dresidual_out"}, {dx, "dx"}, {dresidual_in, "dresidual_in"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (rows == 0) return PCAD_OK;
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < norm_bwd_bytes(rows, D))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_add_rmsnorm_bwd_scratch_bytes large", who);
    hipError_t err = launch_norm_bwd({.x = x, .res_in = residual_in, .w = weight, .dy = dy, .dres_out = dresidual_out, .dx = dx,
                                      .dres_in = dresidual_in, .dw = dweight, .scratch = scratch, .rows = rows, .D = D, .eps = eps,
                                      .dt = dtype, .rdt = res_dtype},
                                     (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: rows / 64 must fit a 32-bit grid", who);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

size_t pcad_loss_head_bwd_scratch_bytes(int B, int L, int D) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    return loss_head_bwd_bytes(B, L, D);
}

int pcad_loss_head_bwd(const void* h, const void* res, const float* norm_weight, const float* emb_f32, const int32_t* complement,
                       const int32_t* labels, const float* loss_weights, int ignore_index, const float* dsum, const float* dnll, void* dh,
                       void* dres, float* dnorm_weight, float* demb, void* scratch, size_t scratch_bytes, int B, int L, int D, float eps,
                       int dtype, int res_dtype, pcad_stream stream) {
    const char* who = "pcad_loss_head_bwd";
    const struct { const void* p; const char* name; } req[] = {{h, "h"}, {res, "res"}, {norm_weight, "norm_weight"}, {emb_f32, "emb_f32"},
                                                               {complement, "complement"}, {labels, "labels"}, {dsum, "dsum"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if (!dh && !dres && !dnorm_weight && !demb)
        return fail(PCAD_ERR_INVALID, "%s: no output requested (dh, dres, dnorm_weight and demb are all NULL)", who);
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (res_dtype != PCAD_F32 && !(res_dtype == PCAD_BF16 && dtype == PCAD_BF16))
        return fail(PCAD_ERR_INVALID, "%s: bad res_dtype %d for dtype %d (BF16 / F32, BF16 / BF16 or F32 / F32)", who, res_dtype, dtype);
    if (B < 0 || L < 0) return fail(PCAD_ERR_INVALID, "%s: B, L must be >= 0 (B=%d, L=%d)", who, B, L);
    if (D <= 0 || D % 8) return fail(PCAD_ERR_INVALID, "%s: D must be a positive multiple of 8 (D=%d)", who, D);
    if (D > 2048) return fail(PCAD_ERR_INVALID, "%s: D must be <= 2048 (D=%d)", who, D);
    const struct { const void* p; const char* name; } al[] = {{h, "h"}, {res, "res"}, {norm_weight, "norm_weight"}, {emb_f32, "emb_f32"},
                                                              {dh, "dh"}, {dres, "dres"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (B == 0 || L == 0) return PCAD_OK;
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < loss_head_bwd_bytes(B, L, D))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_loss_head_bwd_scratch_bytes large", who);
    hipError_t err = launch_loss_head_bwd({.in = {.h = h, .res = res, .w = norm_weight, .B = B, .L = L, .D = D, .eps = eps, .dt = dtype, .rdt = res_dtype},
                                           .emb_f32 = emb_f32, .comp8 = complement, .labels = labels, .loss_w = loss_weights,
                                           .ignore_index = ignore_index, .dsum = dsum, .dnll = dnll, .dh = dh, .dres = dres,
                                           .dnorm_w = dnorm_weight, .demb = demb, .scratch = scratch},
                                          (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: B * ceil(L / 64) must fit a 32-bit grid", who);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

size_t pcad_pooled_head_bwd_scratch_bytes(int B, int L, int D, int pooling) {
    if (B <= 0 || L <= 0 || D <= 0) return 0;
    if (pooling != PCAD_POOL_MEAN && pooling != PCAD_POOL_FIRST && pooling != PCAD_POOL_LAST) return 0;
    return pooled_head_bwd_bytes(B, L, D, pooling);
}

int pcad_pooled_head_bwd(const void* h, const void* res, const float* norm_weight, const float* score_w, const float* pooled,
                         const float* dlogits, void* dh, void* dres, float* dnorm_weight, float* dscore_w, void* scratch, size_t scratch_bytes,
                         int B, int L, int D, int num_labels, float eps, int pooling, int dtype, int res_dtype, pcad_stream stream) {
    const char* who = "pcad_pooled_head_bwd";
    const struct { const void* p; const char* name; } req[] = {{h, "h"}, {res, "res"}, {norm_weight, "norm_weight"}, {score_w, "score_w"},
                                                               {pooled, "pooled"}, {dlogits, "dlogits"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if (!dh && !dres && !dnorm_weight && !dscore_w)
        return fail(PCAD_ERR_INVALID, "%s: no output requested (dh, dres, dnorm_weight and dscore_w are all NULL)", who);
    if (pooling == PCAD_POOL_MAX)
        return fail(PCAD_ERR_INVALID, "%s: pooling PCAD_POOL_MAX has no backward (its gradient needs a tie rule among rows that are equal "
                                      "after rounding to the model dtype)", who);
    if (pooling != PCAD_POOL_MEAN && pooling != PCAD_POOL_FIRST && pooling != PCAD_POOL_LAST)
        return fail(PCAD_ERR_INVALID, "%s: bad pooling %d", who, pooling);
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (res_dtype != PCAD_F32 && !(res_dtype == PCAD_BF16 && dtype == PCAD_BF16))
        return fail(PCAD_ERR_INVALID, "%s: bad res_dtype %d for dtype %d (BF16 / F32, BF16 / BF16 or F32 / F32)", who, res_dtype, dtype);
    if (B < 0 || L < 0) return fail(PCAD_ERR_INVALID, "%s: B, L must be >= 0 (B=%d, L=%d)", who, B, L);
    if (D <= 0 || D % 8) return fail(PCAD_ERR_INVALID, "%s: D must be a positive multiple of 8 (D=%d)", who, D);
    if (D > 2048) return fail(PCAD_ERR_INVALID, "%s: D must be <= 2048 (D=%d)", who, D);
    if (num_labels < 1 || num_labels > PCAD_MAX_LABELS)
        return fail(PCAD_ERR_INVALID, "%s: num_labels must be in [1, %d] (num_labels=%d)", who, PCAD_MAX_LABELS, num_labels);
    const struct { const void* p; const char* name; } al[] = {{h, "h"}, {res, "res"}, {norm_weight, "norm_weight"}, {dh, "dh"}, {dres, "dres"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (B == 0) return PCAD_OK;
    if (L == 0) return fail(PCAD_ERR_INVALID, "%s: L must be >= 1 (a strand without rows has nothing to pool)", who);
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < pooled_head_bwd_bytes(B, L, D, pooling))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_pooled_head_bwd_scratch_bytes large", who);
    hipError_t err = launch_pooled_head_bwd({.in = {.h = h, .res = res, .w = norm_weight, .B = B, .L = L, .D = D, .eps = eps, .dt = dtype, .rdt = res_dtype},
                                             .score_w = score_w, .NL = num_labels, .pooled = pooled, .dlogits = dlogits, .pooling = pooling, .dh = dh,
                                             .dres = dres, .dnorm_w = dnorm_weight, .dscore_w = dscore_w, .scratch = scratch},
                                            (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: 2 B * ceil(L / 64) must fit a 32-bit grid", who);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// ---- the score head on cached pooled vectors (csrc/pool_feat.hip) ----
// what pcad_pooled_logits and pcad_pooled_logits_bwd refuse in (B, D, num_labels)
static int pooled_logits_shape_check(const char* who, int B, int D, int num_labels) {
    if (B < 0) return fail(PCAD_ERR_INVALID, "%s: B must be >= 0 (B=%d)", who, B);
    if (D <= 0 || D % 8) return fail(PCAD_ERR_INVALID, "%s: D must be a positive multiple of 8 (D=%d)", who, D);
    if (D > 2048) return fail(PCAD_ERR_INVALID, "%s: D must be <= 2048 (D=%d)", who, D);
    if (num_labels < 1 || num_labels > PCAD_MAX_LABELS)
        return fail(PCAD_ERR_INVALID, "%s: num_labels must be in [1, %d] (num_labels=%d)", who, PCAD_MAX_LABELS, num_labels);
    return PCAD_OK;
}

int pcad_pooled_logits(const float* pooled, const float* score_w, float* logits, int B, int D, int num_labels, int dtype, pcad_stream stream) {
    const char* who = "pcad_pooled_logits";
    const struct { const void* p; const char* name; } req[] = {{score_w, "score_w"}, {pooled, "pooled"}, {logits, "logits"}};
    for (const auto& r : req)
        if (!r.p && (B != 0 || r.p == score_w)) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);      // no windows: pooled and logits are not touched and may be NULL
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (int rc = pooled_logits_shape_check(who, B, D, num_labels)) return rc;
    const struct { const void* p; const char* name; } al[] = {{pooled, "pooled"}, {score_w, "score_w"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (((uintptr_t)logits) % 4) return fail(PCAD_ERR_INVALID, "%s: logits must be 4-byte aligned", who);
    if (B == 0) return PCAD_OK;
    hipError_t err = launch_pooled_logits({.pooled = pooled, .score_w = score_w, .logits = logits, .B = B, .D = D, .NL = num_labels, .dt = dtype},
                                          (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_pooled_logits_bwd(const float* pooled, const float* score_w, const float* dlogits, float* dscore_w, float* dpooled, int B, int D,
                           int num_labels, pcad_stream stream) {
    const char* who = "pcad_pooled_logits_bwd";
    const struct { const void* p; const char* name; } req[] = {{score_w, "score_w"}, {pooled, "pooled"}, {dlogits, "dlogits"}};
    for (const auto& r : req)
        if (!r.p && (B != 0 || r.p == score_w)) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);      // no windows: pooled and dlogits are not read and may be NULL
    if (!dscore_w && !dpooled) return fail(PCAD_ERR_INVALID, "%s: no output requested (dscore_w and dpooled are both NULL)", who);
    if (int rc = pooled_logits_shape_check(who, B, D, num_labels)) return rc;
    const struct { const void* p; const char* name; } al[] = {{pooled, "pooled"}, {score_w, "score_w"}, {dscore_w, "dscore_w"}, {dpooled, "dpooled"}};
    for (const auto& r : al)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    if (((uintptr_t)dlogits) % 4) return fail(PCAD_ERR_INVALID, "%s: dlogits must be 4-byte aligned", who);
    if (B == 0) return PCAD_OK;
    if ((int64_t)B + num_labels > 0x7fffffff) return fail(PCAD_ERR_INVALID, "%s: B + num_labels must fit a 32-bit grid (B=%d)", who, B);
    hipError_t err = launch_pooled_logits_bwd({.pooled = pooled, .score_w = score_w, .dlogits = dlogits, .dscore_w = dscore_w, .dpooled = dpooled,
                                               .B = B, .D = D, .NL = num_labels},
                                              (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// what pcad_optim_plan and pcad_grads_flat_plan refuse in record i; *chunks_out: the record's chunk count (0 for n == 0)
static int optim_record_check(const char* who, const pcad_optim_tensor& t, int64_t i, int64_t* chunks_out) {
    *chunks_out = 0;
    if (t.n < 0) return fail(PCAD_ERR_INVALID, "%s: table[%lld].n must be >= 0 (n=%lld)", who, (long long)i, (long long)t.n);
    if (t.param_dtype != PCAD_F32 && t.param_dtype != PCAD_BF16)
        return fail(PCAD_ERR_INVALID, "%s: table[%lld].param_dtype: bad dtype %d", who, (long long)i, t.param_dtype);
    if (t.grad_dtype != PCAD_F32 && t.grad_dtype != PCAD_BF16)
        return fail(PCAD_ERR_INVALID, "%s: table[%lld].grad_dtype: bad dtype %d", who, (long long)i, t.grad_dtype);
    if (t.flags & ~PCAD_OPTIM_DECAY) return fail(PCAD_ERR_INVALID, "%s: table[%lld].flags: unknown bits 0x%x", who, (long long)i, t.flags);
    if (t.n == 0) return PCAD_OK;
    const struct { const void* p; const char* name; bool required; } ptr[] = {
        {t.param, "param", true}, {t.grad, "grad", true}, {t.master, "master", t.param_dtype == PCAD_BF16},
        {t.exp_avg, "exp_avg", true}, {t.exp_avg_sq, "exp_avg_sq", true}};
    for (const auto& r : ptr) {
        if (!r.p && r.required)
            return fail(PCAD_ERR_INVALID, "%s: table[%lld].%s is null%s", who, (long long)i, r.name,
                        strcmp(r.name, "master") == 0 ? " (a bf16 param needs an fp32 master)" : "");
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: table[%lld].%s must be 16-byte aligned", who, (long long)i, r.name);
    }
    *chunks_out = (t.n - 1) / PCAD_OPTIM_CHUNK + 1;
    return PCAD_OK;
}

int pcad_optim_plan(const pcad_optim_tensor* table, int64_t count, int32_t* chunk_map, int64_t chunk_capacity, int64_t* chunks_out) {
    const char* who = "pcad_optim_plan";
    if (count < 0) return fail(PCAD_ERR_INVALID, "%s: count must be >= 0", who);
    if (!table && count > 0) return fail(PCAD_ERR_INVALID, "%s: null table", who);
    if (!chunks_out) return fail(PCAD_ERR_INVALID, "%s: null chunks_out", who);
    if (chunk_map && chunk_capacity < 0) return fail(PCAD_ERR_INVALID, "%s: chunk_capacity must be >= 0", who);
    int64_t chunks = 0;
    for (int64_t i = 0; i < count; ++i) {
        int64_t nc = 0;
        if (int rc = optim_record_check(who, table[i], i, &nc)) return rc;
        if (nc == 0) continue;
        if (nc > PCAD_OPTIM_MAX_CHUNKS - chunks) return fail(PCAD_ERR_INVALID, "%s: the table has more than 2^24 - 1 chunks (at table[%lld])", who, (long long)i);
        if (chunk_map) {
            if (chunks + nc > chunk_capacity)
                return fail(PCAD_ERR_INVALID, "%s: chunk_capacity %lld is too small (at table[%lld])", who, (long long)chunk_capacity, (long long)i);
            for (int64_t c = 0; c < nc; ++c) {
                chunk_map[2 * (chunks + c)] = (int32_t)i;
                chunk_map[2 * (chunks + c) + 1] = (int32_t)c;
            }
        }
        chunks += nc;
    }
    *chunks_out = chunks;
    return PCAD_OK;
}

int pcad_grads_flat_plan(const pcad_optim_tensor* table, int64_t count, int64_t* offsets_out, int64_t* total_out) {
    const char* who = "pcad_grads_flat_plan";
    if (count < 0) return fail(PCAD_ERR_INVALID, "%s: count must be >= 0", who);
    if (!table && count > 0) return fail(PCAD_ERR_INVALID, "%s: null table", who);
    if (!offsets_out && count > 0) return fail(PCAD_ERR_INVALID, "%s: null offsets_out", who);
    if (!total_out) return fail(PCAD_ERR_INVALID, "%s: null total_out", who);
    int64_t chunks = 0, total = 0;
    for (int64_t i = 0; i < count; ++i) {
        int64_t nc = 0;
        if (int rc = optim_record_check(who, table[i], i, &nc)) return rc;
        if (nc > PCAD_OPTIM_MAX_CHUNKS - chunks) return fail(PCAD_ERR_INVALID, "%s: the table has more than 2^24 - 1 chunks (at table[%lld])", who, (long long)i);
        chunks += nc;
        offsets_out[i] = total;
        total += (table[i].n + 3) / 4 * 4;              // below 2^24 chunks of 4096: far from 2^63
    }
    *total_out = total;
    return PCAD_OK;
}

size_t pcad_adamw_step_scratch_bytes(int64_t chunks) { return optim_scratch_bytes(chunks); }

static int optim_table_check(const char* who, const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks) {
    if (count < 0 || chunks < 0) return fail(PCAD_ERR_INVALID, "%s: count, chunks must be >= 0 (count=%lld, chunks=%lld)", who, (long long)count, (long long)chunks);
    if (chunks > PCAD_OPTIM_MAX_CHUNKS) return fail(PCAD_ERR_INVALID, "%s: chunks must be <= 2^24 - 1, a grid of 256-lane blocks below 2^32 lanes (chunks=%lld)", who, (long long)chunks);
    if (count > 0x7fffffff) return fail(PCAD_ERR_INVALID, "%s: count must fit the chunk map's 32-bit index (count=%lld)", who, (long long)count);
    if (chunks > 0) {
        if (!table || count == 0) return fail(PCAD_ERR_INVALID, "%s: null table", who);
        if (!chunk_map) return fail(PCAD_ERR_INVALID, "%s: null chunk_map", who);
        if (((uintptr_t)table) % 16) return fail(PCAD_ERR_INVALID, "%s: table must be 16-byte aligned", who);
        if (((uintptr_t)chunk_map) % 8) return fail(PCAD_ERR_INVALID, "%s: chunk_map must be 8-byte aligned", who);
    }
    return PCAD_OK;
}

int pcad_adamw_step(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, void* state, void* scratch, size_t scratch_bytes,
                    double lr, double beta1, double beta2, double eps, double weight_decay, double bc1, double bc2, double max_norm,
                    double grad_scale, pcad_stream stream) {
    const char* who = "pcad_adamw_step";
    if (int rc = optim_table_check(who, table, chunk_map, count, chunks)) return rc;
    if (!state) return fail(PCAD_ERR_INVALID, "%s: null state", who);
    if (((uintptr_t)state) % 16) return fail(PCAD_ERR_INVALID, "%s: state must be 16-byte aligned", who);
    const struct { double v; const char* name; } sc[] = {{lr, "lr"}, {beta1, "beta1"}, {beta2, "beta2"}, {eps, "eps"}, {weight_decay, "weight_decay"},
                                                         {bc1, "bc1"}, {bc2, "bc2"}, {max_norm, "max_norm"}, {grad_scale, "grad_scale"}};
    for (const auto& r : sc)
        if (!(r.v - r.v == 0.0)) return fail(PCAD_ERR_INVALID, "%s: %s must be finite", who, r.name);
    if (!(bc1 > 0.0 && bc1 <= 1.0)) return fail(PCAD_ERR_INVALID, "%s: bc1 = 1 - beta1^t must be in (0, 1] (bc1=%g)", who, bc1);
    if (!(bc2 > 0.0 && bc2 <= 1.0)) return fail(PCAD_ERR_INVALID, "%s: bc2 = 1 - beta2^t must be in (0, 1] (bc2=%g)", who, bc2);
    if (chunks > 0 && (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < optim_scratch_bytes(chunks)))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_adamw_step_scratch_bytes large", who);
    hipError_t err = launch_adamw_step({.table = table, .map = chunk_map, .chunks = chunks, .state = state, .part = (float*)scratch,
                                        .max_norm = (float)max_norm, .grad_scale = (float)grad_scale, .decay = (float)(1.0 - lr * weight_decay),
                                        .b1 = (float)beta1, .omb1 = (float)(1.0 - beta1), .b2 = (float)beta2, .omb2 = (float)(1.0 - beta2),
                                        .step_size = (float)(lr / bc1), .bc2_sqrt = (float)sqrt(bc2), .eps = (float)eps},
                                       (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_zero_grads(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, pcad_stream stream) {
    const char* who = "pcad_zero_grads";
    if (int rc = optim_table_check(who, table, chunk_map, count, chunks)) return rc;
    hipError_t err = launch_zero_grads(table, chunk_map, chunks, (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

int pcad_grads_gather(const void* table, const int32_t* chunk_map, int64_t count, int64_t chunks, const int64_t* offsets, float* flat,
                      int64_t flat_elems, pcad_stream stream) {
    const char* who = "pcad_grads_gather";
    if (int rc = optim_table_check(who, table, chunk_map, count, chunks)) return rc;
    if (flat_elems < 0) return fail(PCAD_ERR_INVALID, "%s: flat_elems must be >= 0 (flat_elems=%lld)", who, (long long)flat_elems);
    if (chunks > 0) {
        if (!offsets) return fail(PCAD_ERR_INVALID, "%s: null offsets", who);
        if (((uintptr_t)offsets) % 8) return fail(PCAD_ERR_INVALID, "%s: offsets must be 8-byte aligned", who);
        if (!flat) return fail(PCAD_ERR_INVALID, "%s: null flat", who);
        if (((uintptr_t)flat) % 16) return fail(PCAD_ERR_INVALID, "%s: flat must be 16-byte aligned", who);
    }
    hipError_t err = launch_grads_gather(table, chunk_map, chunks, offsets, flat, flat_elems, (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// what the three pcad_linear_wgrad* entries refuse in (M, N, K)
static int wgrad_shape_check(const char* who, int64_t M, int N, int K) {
    if (M < 0) return fail(PCAD_ERR_INVALID, "%s: M must be >= 0 (M=%lld)", who, (long long)M);
    if (N < 8 || N > 8192 || N % 8) return fail(PCAD_ERR_INVALID, "%s: N must be a multiple of 8 in [8, 8192] (N=%d)", who, N);
    if (K < 8 || K > 8192 || K % 8) return fail(PCAD_ERR_INVALID, "%s: K must be a multiple of 8 in [8, 8192] (K=%d)", who, K);
    return PCAD_OK;
}

int64_t pcad_linear_wgrad_slabs(int64_t M, int N, int K, int64_t* rows_per_slab_out) {
    int64_t rows = 0;
    if (rows_per_slab_out) *rows_per_slab_out = 0;
    if (wgrad_shape_check("pcad_linear_wgrad_slabs", M, N, K)) return -1;
    const int64_t slabs = wgrad_slabs(M, N, K, &rows);
    if (rows_per_slab_out) *rows_per_slab_out = rows;
    return slabs;
}

size_t pcad_linear_wgrad_scratch_bytes(int64_t M, int N, int K) {
    if (M < 0 || N < 8 || N > 8192 || N % 8 || K < 8 || K > 8192 || K % 8) return 0;
    return wgrad_bytes(M, N, K);
}

int pcad_linear_wgrad(const void* dy, int64_t lddy, const void* x, int64_t ldx, float* dw, int64_t lddw, int64_t M, int N, int K,
                      int accumulate, void* scratch, size_t scratch_bytes, pcad_stream stream) {
    const char* who = "pcad_linear_wgrad";
    const struct { const void* p; const char* name; } req[] = {{dy, "dy"}, {x, "x"}, {dw, "dw"}};
    if (!dw) return fail(PCAD_ERR_INVALID, "%s: null dw", who);
    for (const auto& r : req)
        if (!r.p && M != 0) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);      // no rows: dy and x are not read and may be NULL
    if (int rc = wgrad_shape_check(who, M, N, K)) return rc;
    if (lddy < N || lddy % 8) return fail(PCAD_ERR_INVALID, "%s: lddy must be a multiple of 8 and >= N (lddy=%lld, N=%d)", who, (long long)lddy, N);
    if (ldx < K || ldx % 8) return fail(PCAD_ERR_INVALID, "%s: ldx must be a multiple of 8 and >= K (ldx=%lld, K=%d)", who, (long long)ldx, K);
    if (lddw < K || lddw % 4) return fail(PCAD_ERR_INVALID, "%s: lddw must be a multiple of 4 and >= K (lddw=%lld, K=%d)", who, (long long)lddw, K);
    for (const auto& r : req)
        if (((uintptr_t)r.p) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, r.name);
    const size_t need = wgrad_bytes(M, N, K);
    if (need > 0 && (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < need))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_linear_wgrad_scratch_bytes large", who);
    hipError_t err = launch_linear_wgrad({.dy = dy, .lddy = lddy, .x = x, .ldx = ldx, .dw = dw, .lddw = lddw, .M = M, .N = N, .K = K,
                                          .accumulate = accumulate != 0, .scratch = scratch},
                                         (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// ---- the dropout-masked down-projection of a LoRA branch (csrc/lora.hip) ----
static int lora_p_check(const char* who, double p) {
    const int64_t T = lora_threshold(p);
    if (T < 0 || T > 65535)
        return fail(PCAD_ERR_INVALID, "%s: p must be in [0, 1) with floor(p 65536 + 0.5) <= 65535 (p=%g)", who, p);
    return PCAD_OK;
}

static int lora_shape_check(const char* who, int64_t M, int K, int r, bool with_r) {
    if (M < 0 || M >= ((int64_t)1 << 32)) return fail(PCAD_ERR_INVALID, "%s: M must be in [0, 2^32) (M=%lld)", who, (long long)M);
    if (K < 8 || K > LORA_MAX_K || K % 8) return fail(PCAD_ERR_INVALID, "%s: K must be a multiple of 8 in [8, %d] (K=%d)", who, LORA_MAX_K, K);
    if (with_r && r != 4 && r != 8 && r != 16) return fail(PCAD_ERR_INVALID, "%s: r must be 4, 8 or 16 (r=%d)", who, r);
    return PCAD_OK;
}

int pcad_lora_dropout_mask(uint8_t* keep_u8, int64_t M, int K, int64_t ldk, double p, uint64_t seed, uint64_t stream_id, pcad_stream stream) {
    const char* who = "pcad_lora_dropout_mask";
    if (int rc = lora_shape_check(who, M, K, 0, false)) return rc;
    if (ldk < K) return fail(PCAD_ERR_INVALID, "%s: ldk must be >= K (ldk=%lld, K=%d)", who, (long long)ldk, K);
    if (int rc = lora_p_check(who, p)) return rc;
    if (!keep_u8 && M != 0) return fail(PCAD_ERR_INVALID, "%s: null keep_u8", who);
    hipError_t err = launch_lora_dropout_mask(keep_u8, M, K, ldk, lora_mask(p, seed, stream_id), (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// what pcad_lora_down and pcad_lora_down_bwd ask of a [M, K] operand in the model dtype
static int lora_rows_check(const char* who, const char* name, const char* ldname, const void* ptr, int64_t ld, int K) {
    if (ld < K || ld % 8) return fail(PCAD_ERR_INVALID, "%s: %s must be a multiple of 8 and >= K (%s=%lld, K=%d)", who, ldname, ldname, (long long)ld, K);
    if (((uintptr_t)ptr) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, name);
    return PCAD_OK;
}

int pcad_lora_down(const void* x, int64_t ldx, const float* A, float* t, int64_t M, int K, int r, double p, uint64_t seed, uint64_t stream_id,
                   int dtype, pcad_stream stream) {
    const char* who = "pcad_lora_down";
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (int rc = lora_shape_check(who, M, K, r, true)) return rc;
    if (int rc = lora_p_check(who, p)) return rc;
    if (!A) return fail(PCAD_ERR_INVALID, "%s: null A", who);
    if (M != 0 && !x) return fail(PCAD_ERR_INVALID, "%s: null x", who);
    if (M != 0 && !t) return fail(PCAD_ERR_INVALID, "%s: null t", who);
    if (int rc = lora_rows_check(who, "x", "ldx", x, ldx, K)) return rc;
    if (((uintptr_t)A) % 16) return fail(PCAD_ERR_INVALID, "%s: A must be 16-byte aligned", who);
    if (((uintptr_t)t) % 16) return fail(PCAD_ERR_INVALID, "%s: t must be 16-byte aligned", who);
    hipError_t err = launch_lora_down({.x = x, .ldx = ldx, .A = A, .t = t, .M = M, .K = K, .r = r, .mask = lora_mask(p, seed, stream_id), .dt = dtype},
                                      (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

int64_t pcad_lora_down_bwd_slabs(int64_t M, int K, int r, int64_t* rows_per_slab_out) {
    int64_t rows = 0;
    if (rows_per_slab_out) *rows_per_slab_out = 0;
    if (lora_shape_check("pcad_lora_down_bwd_slabs", M, K, r, true)) return -1;
    const int64_t slabs = lora_down_bwd_slabs(M, K, &rows);
    if (rows_per_slab_out) *rows_per_slab_out = rows;
    return slabs;
}

size_t pcad_lora_down_bwd_scratch_bytes(int64_t M, int K, int r) {
    if (M < 0 || M >= ((int64_t)1 << 32) || K < 8 || K > LORA_MAX_K || K % 8 || (r != 4 && r != 8 && r != 16)) return 0;
    return lora_down_bwd_bytes(M, K, r);
}

int pcad_lora_down_bwd(const void* x, int64_t ldx, const float* A, const float* u, void* dx, int64_t lddx, float* dA, void* scratch,
                       size_t scratch_bytes, int64_t M, int K, int r, double p, uint64_t seed, uint64_t stream_id, int dtype, pcad_stream stream) {
    const char* who = "pcad_lora_down_bwd";
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (int rc = lora_shape_check(who, M, K, r, true)) return rc;
    if (int rc = lora_p_check(who, p)) return rc;
    if (!dx && !dA) return fail(PCAD_ERR_INVALID, "%s: no output requested (dx and dA are both NULL)", who);
    if (!A) return fail(PCAD_ERR_INVALID, "%s: null A", who);
    if (M != 0 && !x) return fail(PCAD_ERR_INVALID, "%s: null x", who);
    if (M != 0 && !u) return fail(PCAD_ERR_INVALID, "%s: null u", who);
    if (int rc = lora_rows_check(who, "x", "ldx", x, ldx, K)) return rc;
    if (dx)
        if (int rc = lora_rows_check(who, "dx", "lddx", dx, lddx, K)) return rc;
    const struct { const void* ptr; const char* name; } al[] = {{A, "A"}, {u, "u"}, {dA, "dA"}};
    for (const auto& q : al)
        if (((uintptr_t)q.ptr) % 16) return fail(PCAD_ERR_INVALID, "%s: %s must be 16-byte aligned", who, q.name);
    const size_t need = dA ? lora_down_bwd_bytes(M, K, r) : 0;
    if (need > 0 && (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < need))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_lora_down_bwd_scratch_bytes large", who);
    hipError_t err = launch_lora_down_bwd({.x = x, .ldx = ldx, .A = A, .u = u, .dx = dx, .lddx = lddx, .dA = dA, .scratch = scratch, .M = M,
                                           .K = K, .r = r, .mask = lora_mask(p, seed, stream_id), .dt = dtype},
                                          (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// ---- the segmented backward of the selective scan (csrc/scan_bwd_seg.hip) ----
int pcad_selective_scan_bwd_seg_steps(int L, int segments) { return scan_bwd_seg_steps(L, segments); }

size_t pcad_selective_scan_bwd_seg_scratch_bytes(int S, int L, int E, int segments) {
    if (S <= 0 || L <= 0 || E <= 0 || E % 64 || segments < 1 || segments > SCAN_BWD_MAX_SEGMENTS) return 0;
    return scan_bwd_seg_bytes(S, L, E, segments);
}

int pcad_selective_scan_bwd_seg(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc, const float* A,
                                const float* Dskip, const float* delta_bias, const void* dout, void* du, void* ddelta, void* dz, float* dbc,
                                float* dA, float* dD, float* ddelta_bias, void* scratch, size_t scratch_bytes, int S, int L, int E,
                                int reverse, int dtype, int segments, pcad_stream stream) {
    const char* who = "pcad_selective_scan_bwd_seg";
    const struct { const void* p; const char* name; } req[] = {
        {u, "u"}, {delta, "delta"}, {bc, "bc"}, {A, "A"}, {Dskip, "Dskip"}, {delta_bias, "delta_bias"}, {dout, "dout"}, {du, "du"},
        {ddelta, "ddelta"}, {dbc, "dbc"}, {dA, "dA"}, {dD, "dD"}, {ddelta_bias, "ddelta_bias"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if ((z != nullptr) != (dz != nullptr))
        return fail(PCAD_ERR_INVALID, "%s: dz is required exactly when z is given (z %s, dz %s)", who, z ? "given" : "NULL", dz ? "given" : "NULL");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (S < 0 || L < 0 || E <= 0 || E % 64) return fail(PCAD_ERR_INVALID, "%s: E must be a multiple of 64 (E=%d); S, L >= 0", who, E);
    if (segments < 1 || segments > SCAN_BWD_MAX_SEGMENTS)
        return fail(PCAD_ERR_INVALID, "%s: segments must be in [1, %d] (segments=%d)", who, SCAN_BWD_MAX_SEGMENTS, segments);
    if (z && ldz < E) return fail(PCAD_ERR_INVALID, "%s: ldz must be >= E", who);
    if (((uintptr_t)bc) % 16) return fail(PCAD_ERR_INVALID, "%s: bc must be 16-byte aligned", who);
    if (((uintptr_t)dbc) % 16) return fail(PCAD_ERR_INVALID, "%s: dbc must be 16-byte aligned", who);
    if (S == 0 || L == 0) return PCAD_OK;
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < scan_bwd_seg_bytes(S, L, E, segments))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_selective_scan_bwd_seg_scratch_bytes large", who);
    hipError_t err = launch_scan_bwd_seg({.u = u, .delta = delta, .z = z, .ldz = ldz, .bc = bc, .A = A, .Dskip = Dskip, .dbias = delta_bias, .dout = dout,
                                          .du = du, .ddelta = ddelta, .dz = dz, .dbc = dbc, .dA = dA, .dD = dD, .ddbias = ddelta_bias,
                                          .scratch = scratch, .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0},
                                         segments, (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "%s: S * segments * E / 64 and S * L * 32 / 256 must fit a 32-bit grid", who);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

// ---- the segmented training forward of the selective scan (csrc/scan_fwd_seg.hip) ----
size_t pcad_selective_scan_fwd_seg_scratch_bytes(int S, int L, int E, int segments) {
    if (S <= 0 || L <= 0 || E <= 0 || E % 64 || segments < 1 || segments > SCAN_BWD_MAX_SEGMENTS) return 0;
    return scan_fwd_seg_bytes(S, L, E, segments);
}

int pcad_selective_scan_fwd_seg(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc, const float* A,
                                const float* Dskip, const float* delta_bias, void* y, void* scratch, size_t scratch_bytes, int S, int L,
                                int E, int reverse, int dtype, int segments, pcad_stream stream) {
    const char* who = "pcad_selective_scan_fwd_seg";
    const struct { const void* p; const char* name; } req[] = {
        {u, "u"}, {delta, "delta"}, {bc, "bc"}, {A, "A"}, {Dskip, "Dskip"}, {delta_bias, "delta_bias"}, {y, "y"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "%s: null %s", who, r.name);
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "%s: bad dtype %d", who, dtype);
    if (S < 0 || L < 0 || E <= 0 || E % 64) return fail(PCAD_ERR_INVALID, "%s: E must be a multiple of 64 (E=%d); S, L >= 0", who, E);
    if (segments < 1 || segments > SCAN_BWD_MAX_SEGMENTS)
        return fail(PCAD_ERR_INVALID, "%s: segments must be in [1, %d] (segments=%d)", who, SCAN_BWD_MAX_SEGMENTS, segments);
    if (z && ldz < E) return fail(PCAD_ERR_INVALID, "%s: ldz must be >= E", who);
    if (((uintptr_t)bc) % 16) return fail(PCAD_ERR_INVALID, "%s: bc must be 16-byte aligned", who);
    if (S == 0 || L == 0) return PCAD_OK;
    if (!scan_fwd_seg_grid_ok(S, L, E, segments))
        return fail(PCAD_ERR_INVALID, "%s: S * segments * E / 64 and S * 16 * E / 256 must fit a 32-bit grid", who);
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < scan_fwd_seg_bytes(S, L, E, segments))
        return fail(PCAD_ERR_WORKSPACE, "%s: scratch must be 256-byte aligned and pcad_selective_scan_fwd_seg_scratch_bytes large", who);
    hipError_t err = launch_scan_fwd_seg({.u = u, .delta = delta, .z = z, .ldz = ldz, .bc = bc, .A = A, .Dskip = Dskip, .dbias = delta_bias, .y = y,
                                          .scratch = scratch, .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0},
                                         segments, (hipStream_t)stream);
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "%s: %s", who, hipGetErrorString(err));
    return PCAD_OK;
}

}  // extern "C"
