// The entry points of libpcad_train.so (include/pcad_train.h): argument checks + the launch.  The library links libpcad.so and reports
// through its pcad::fail, so pcad_last_error() of the calling thread carries the message.
#include "../../include/pcad_train.h"
#include "pcad_internal.hpp"
using namespace pcad;

extern "C" {

size_t pcad_selective_scan_bwd_scratch_bytes(int S, int L, int E) {
    if (S <= 0 || L <= 0 || E <= 0 || E % 64) return 0;
    return scan_bwd_bytes(S, L, E);
}

int pcad_selective_scan_bwd(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc, const float* A,
                            const float* Dskip, const float* delta_bias, const void* dout, void* du, void* ddelta, void* dz, float* dbc,
                            float* dA, float* dD, float* ddelta_bias, void* scratch, size_t scratch_bytes, int S, int L, int E,
                            int reverse, int dtype, pcad_stream stream) {
    const struct { const void* p; const char* name; } req[] = {
        {u, "u"}, {delta, "delta"}, {bc, "bc"}, {A, "A"}, {Dskip, "Dskip"}, {delta_bias, "delta_bias"}, {dout, "dout"}, {du, "du"},
        {ddelta, "ddelta"}, {dbc, "dbc"}, {dA, "dA"}, {dD, "dD"}, {ddelta_bias, "ddelta_bias"}};
    for (const auto& r : req)
        if (!r.p) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: null %s", r.name);
    if ((z != nullptr) != (dz != nullptr))
        return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: dz is required exactly when z is given (z %s, dz %s)", z ? "given" : "NULL", dz ? "given" : "NULL");
    if (dtype != PCAD_F32 && dtype != PCAD_BF16) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: bad dtype %d", dtype);
    if (S < 0 || L < 0 || E <= 0 || E % 64) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: E must be a multiple of 64 (E=%d); S, L >= 0", E);
    if (z && ldz < E) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: ldz must be >= E");
    if (((uintptr_t)bc) % 16) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: bc must be 16-byte aligned");
    if (((uintptr_t)dbc) % 16) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: dbc must be 16-byte aligned");
    if (S == 0 || L == 0) return PCAD_OK;
    if (!scratch || ((uintptr_t)scratch) % 256 || scratch_bytes < scan_bwd_bytes(S, L, E))
        return fail(PCAD_ERR_WORKSPACE, "pcad_selective_scan_bwd: scratch must be 256-byte aligned and pcad_selective_scan_bwd_scratch_bytes large");
    hipError_t err = launch_scan_bwd({.u = u, .delta = delta, .z = z, .ldz = ldz, .bc = bc, .A = A, .Dskip = Dskip, .dbias = delta_bias, .dout = dout,
                                      .du = du, .ddelta = ddelta, .dz = dz, .dbc = dbc, .dA = dA, .dD = dD, .ddbias = ddelta_bias, .scratch = scratch,
                                      .S = S, .L = L, .E = E, .dt = dtype, .reverse = reverse != 0},
                                     (hipStream_t)stream);
    if (err == hipErrorInvalidValue) return fail(PCAD_ERR_INVALID, "pcad_selective_scan_bwd: S * E / 64 and S * L * 32 / 256 must fit a 32-bit grid");
    if (err != hipSuccess) return fail(PCAD_ERR_HIP, "pcad_selective_scan_bwd: %s", hipGetErrorString(err));
    return PCAD_OK;
}

}  // extern "C"
