// Backward of the selective scan (include/pcad_train.h pcad_selective_scan_bwd, libpcad_train.so), one direction, plain token-major layout:
// the scratch layout and the launch of the unsegmented form.  The kernels, with the formulas and the two passes, are in scan_bwd_kernel.hpp.
#include "scan_bwd_kernel.hpp"

namespace pcad {

namespace {
constexpr size_t sb_align(size_t v) { return (v + 255) / 256 * 256; }
int sb_chunks(int L) { return (L + SBT - 1) / SBT; }
// scratch sections, each 256-byte aligned: checkpoints [S][chunks][16][E], dbc partials [S L][E/64][32], dA [S][E][16], dD [S][E], dbias [S][E]
struct ScanBwdCarve { size_t ckpt, part, pA, pD, pbias, total; };
ScanBwdCarve sb_carve(int S, int L, int E) {
    ScanBwdCarve c;
    const size_t f = sizeof(float), s = (size_t)S, e = (size_t)E;
    c.ckpt = 0;
    c.part = c.ckpt + sb_align(s * sb_chunks(L) * 16 * e * f);
    c.pA = c.part + sb_align(s * (size_t)L * (e / 64) * 32 * f);
    c.pD = c.pA + sb_align(s * e * 16 * f);
    c.pbias = c.pD + sb_align(s * e * f);
    c.total = c.pbias + sb_align(s * e * f);
    return c;
}
}  // namespace

size_t scan_bwd_bytes(int S, int L, int E) { return sb_carve(S, L, E).total; }

template <typename T>
static hipError_t launch_scan_bwd_t(const ScanBwdLaunch& a, hipStream_t s) {
    const ScanBwdCarve cv = sb_carve(a.S, a.L, a.E);
    char* base = (char*)a.scratch;
    float *ckpt = (float*)(base + cv.ckpt), *part = (float*)(base + cv.part), *pA = (float*)(base + cv.pA), *pD = (float*)(base + cv.pD),
          *pbias = (float*)(base + cv.pbias);
    const dim3 grid((unsigned)((int64_t)a.S * (a.E / 64))), blk(64);
#define PCAD_SCAN_BWD(G)                                                                                                             \
    hipLaunchKernelGGL((scan_bwd_kernel<T, G, false>), grid, blk, 0, s, (const T*)a.u, (const T*)a.delta, (const T*)a.z, a.ldz, a.bc, a.A, \
                       a.Dskip, a.dbias, (const T*)a.dout, (T*)a.du, (T*)a.ddelta, (T*)a.dz, ckpt, part, pA, pD, pbias, a.L, a.E,   \
                       a.reverse ? 1 : 0, ScanBwdSegArgs{})
    if (a.z != nullptr) PCAD_SCAN_BWD(true);
    else PCAD_SCAN_BWD(false);
#undef PCAD_SCAN_BWD
    if (hipError_t e = hipGetLastError()) return e;
    const int64_t rows = (int64_t)a.S * a.L, n = rows * 32 + (int64_t)a.E * 18;
    hipLaunchKernelGGL(scan_bwd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)part, (const float*)pA,
                       (const float*)pD, (const float*)pbias, a.dbc, a.dA, a.dD, a.ddbias, rows, a.S, a.E);
    return hipGetLastError();
}

hipError_t launch_scan_bwd(const ScanBwdLaunch& a, hipStream_t s) {
    if (a.S <= 0 || a.L <= 0 || a.E <= 0 || a.E % 64 || a.scratch == nullptr || (a.z != nullptr) != (a.dz != nullptr)) return hipErrorInvalidValue;
    // one wave per (strand, 64 channels) and one reduce thread per output element, both as 32-bit grids
    if ((int64_t)a.S * (a.E / 64) > 0x7fffffff || ((int64_t)a.S * a.L * 32 + (int64_t)a.E * 18 + 255) / 256 > 0x7fffffff) return hipErrorInvalidValue;
    if (a.dt == BF16) return launch_scan_bwd_t<bf16_t>(a, s);
    if (a.dt == F32) return launch_scan_bwd_t<float>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace pcad
