// Segmented backward of the selective scan (include/pcad_bwd.h pcad_selective_scan_bwd_seg, libpcad_bwd.so): the strand's L walk
// steps are cut into G segments of `steps` steps (a multiple of SCAN_BWD_CHUNK; the last one may be shorter) and one wave owns 64
// channels of one segment, so that a call of few strands fills G times as many wave slots.
//
// Both recurrences of the backward are linear in what they carry, with the same coefficients a_s[n] = exp(d_s A[c,n]):
//   h_s = a_s h_{s-1} + d_s u_s B_s                 (the state, walked up)
//   kc_{s-1} = a_s (dy_s C_s + kc_s)                (kc_s = a_{s+1} k_{s+1}: the adjoint handed down; scan_bwd_kernel's `kc`)
// so a segment's effect on either is (carried value) x P_g + (what the segment yields from a zero start), P_g[n] = prod_s a_s[n] =
// exp(A[c,n] sum_s d_s):
//   phase 1  scan_bwd_seg_local_kernel, one wave per (strand, segment, 64 channels): from h = 0 up the segment -> e_g[n] and
//            Dsum_g = sum d_s (segments g < G - 1); from kc = 0 down the segment -> kappa_g[n] (segments g > 0; needs dy, C and d only)
//   phase 2  scan_bwd_seg_combine_kernel, one thread per (strand, n, channel), serial over the segments in a fixed order:
//            H_0 = 0, H_{g+1} = P_g H_g + e_g ascending, H_g stored to the checkpoint slot segment g's first chunk starts from;
//            K_{G-1} = 0, K_{g-1} = P_g K_g + kappa_g descending, K_{g-1} stored over kappa_g (slot g: what segment g - 1 reads)
//   phase 3  scan_bwd_kernel<.., SEG>: pass A from H_g, pass B from K_g, dA / dD / dbias partials per (strand, segment), which
//            scan_bwd_reduce_kernel adds in index order as S G "strands".
// No floating-point atomics; every sum has a fixed order, so a call is bit-reproducible for a given G.  A call with one segment
// (segments == 1, or L <= steps) launches the unsegmented kernel: the bits of pcad_selective_scan_bwd.  All in-tensor offsets are 64-bit.
#include "scan_bwd_kernel.hpp"

namespace pcad {

namespace {
constexpr size_t sbs_align(size_t v) { return (v + 255) / 256 * 256; }
// scratch sections, each 256-byte aligned: the unsegmented call's (checkpoints [S][chunks][16][E], dbc partials [S L][E/64][32]) with the
// dA [S G][E][16], dD [S G][E], dbias [S G][E] partials per (strand, segment), then e [S][G][16][E], kappa / K [S][G][16][E], Dsum [S][G][E]
struct ScanBwdSegCarve { size_t ckpt, part, pA, pD, pbias, e, kap, dsum, total; };
ScanBwdSegCarve sbs_carve(int S, int L, int E, int G) {
    ScanBwdSegCarve c;
    const size_t f = sizeof(float), sg = (size_t)S * G, e = (size_t)E;
    c.ckpt = 0;
    c.part = c.ckpt + sbs_align((size_t)S * ((L + SBT - 1) / SBT) * 16 * e * f);
    c.pA = c.part + sbs_align((size_t)S * L * (e / 64) * 32 * f);
    c.pD = c.pA + sbs_align(sg * e * 16 * f);
    c.pbias = c.pD + sbs_align(sg * e * f);
    c.e = c.pbias + sbs_align(sg * e * f);
    const size_t carry = G > 1 ? sg : 0;                 // one segment: no phases 1 and 2
    c.kap = c.e + sbs_align(carry * 16 * e * f);
    c.dsum = c.kap + sbs_align(carry * 16 * e * f);
    c.total = c.dsum + sbs_align(carry * e * f);
    return c;
}
}  // namespace

int scan_bwd_seg_steps(int L, int segments) {
    if (L < 1 || segments < 1 || segments > SCAN_BWD_MAX_SEGMENTS) return 0;
    const int per = (L + segments - 1) / segments;
    return SBT * ((per + SBT - 1) / SBT);
}

size_t scan_bwd_seg_bytes(int S, int L, int E, int segments) {
    const int steps = scan_bwd_seg_steps(L, segments);
    if (steps == 0) return 0;
    return sbs_carve(S, L, E, (L + steps - 1) / steps).total;
}

// Phase 1.  Grid: (strand G + g) (E / 64) + wave; lane = channel; the loads of scan_bwd_kernel's pass A.
template <typename T, bool GATED>
__global__ __launch_bounds__(64) void scan_bwd_seg_local_kernel(const T* __restrict__ u, const T* __restrict__ delta, const T* __restrict__ z, int64_t ldz,
                                                                const float* __restrict__ bc, const float* __restrict__ A,
                                                                const float* __restrict__ dbias, const T* __restrict__ dout,
                                                                float* __restrict__ eo, float* __restrict__ kap, float* __restrict__ dsum,
                                                                int L, int E, int reverse, int steps, int G) {
    const int lane = threadIdx.x;
    const int nw = E >> 6;
    const int w = blockIdx.x % nw;
    const int64_t unit = blockIdx.x / nw;                   // strand * G + g
    const int g = (int)(unit % G);
    const int64_t strand = unit / G;
    const int c = (w << 6) + lane;                          // < E: E is a multiple of 64
    const int64_t row0 = strand * L;
    const int s0 = g * steps, s1 = min(L, s0 + steps);      // s0 < L: G = ceil(L / steps)
    float Ac[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) Ac[n] = A[(int64_t)c * 16 + n];
    const float bias = dbias[c];
    const int64_t slot = (unit * 16) * (int64_t)E + c;      // + n * E

    if (g + 1 < G) {                                         // a whole segment: steps / SBT whole chunks, all below L
        float h[16], ds = 0.f;
#pragma unroll
        for (int n = 0; n < 16; ++n) h[n] = 0.f;
        for (int sb = s0; sb < s1; sb += SBT) {
            float uu[SBT], dd[SBT];
#pragma unroll
            for (int i = 0; i < SBT; ++i) {
                const int s = sb + i;
                const int64_t at = (row0 + (reverse ? L - 1 - s : s)) * E + c;
                uu[i] = Elem<T>::load(u + at);
                dd[i] = softplus(Elem<T>::load(delta + at) + bias);
            }
#pragma unroll
            for (int i = 0; i < SBT; ++i) {
                const int s = sb + i;
                const float* bcr = bc + (row0 + (reverse ? L - 1 - s : s)) * 32;
                const float d2 = dd[i] * kLog2e, du_ = dd[i] * uu[i];
                ds += dd[i];
#pragma unroll
                for (int n = 0; n < 16; ++n) h[n] = fast_exp2(d2 * Ac[n]) * h[n] + du_ * bcr[n];
            }
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) eo[slot + (int64_t)n * E] = h[n];
        dsum[unit * E + c] = ds;
    }

    if (g > 0) {                                             // the last segment may end inside a chunk
        float kc[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) kc[n] = 0.f;
        const int nch = (s1 - s0 + SBT - 1) / SBT;
        for (int j = nch - 1; j >= 0; --j) {
            const int sb = s0 + j * SBT, len = min(SBT, s1 - sb);
            float dd[SBT], dy[SBT];
#pragma unroll
            for (int i = 0; i < SBT; ++i) {
                if (i < len) {
                    const int s = sb + i;
                    const int64_t row = row0 + (reverse ? L - 1 - s : s);
                    const int64_t at = row * E + c;
                    dd[i] = softplus(Elem<T>::load(delta + at) + bias);
                    const float gv = Elem<T>::load(dout + at);
                    if (GATED) {
                        const float zv = Elem<T>::load(z + row * ldz + c);
                        dy[i] = gv * (zv * sigmoid_f(zv));
                    } else {
                        dy[i] = gv;
                    }
                }
            }
#pragma unroll
            for (int i = SBT - 1; i >= 0; --i) {
                if (i < len) {
                    const int s = sb + i;
                    const float* bcr = bc + (row0 + (reverse ? L - 1 - s : s)) * 32;
                    const float d2 = dd[i] * kLog2e;
#pragma unroll
                    for (int n = 0; n < 16; ++n) kc[n] = fast_exp2(d2 * Ac[n]) * (dy[i] * bcr[16 + n] + kc[n]);
                }
            }
        }
#pragma unroll
        for (int n = 0; n < 16; ++n) kap[slot + (int64_t)n * E] = kc[n];
    }
}

// Phase 2.  One thread per (strand, n, channel), the channel fastest; the G segments in index order, ascending for H and descending for K.
__global__ __launch_bounds__(256) void scan_bwd_seg_combine_kernel(const float* __restrict__ A, const float* __restrict__ eo, float* __restrict__ kap,
                                                                   const float* __restrict__ dsum, float* __restrict__ ckpt, int64_t total,
                                                                   int L, int E, int steps, int G) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                  // total = S * 16 * E
    const int c = (int)(i % E), n = (int)((i / E) % 16);
    const int64_t strand = i / ((int64_t)E * 16);
    const int nck = (L + SBT - 1) / SBT, cps = steps / SBT;
    const float An = A[(int64_t)c * 16 + n];
    const float* ds = dsum + strand * G * (int64_t)E + c;                     // + g * E
    const int64_t carry = (strand * G * 16 + n) * (int64_t)E + c;             // + g * 16 * E
    float* ck = ckpt + (strand * nck * 16 + n) * (int64_t)E + c;              // + chunk * 16 * E
    float H = 0.f;
    for (int g = 0; g + 1 < G; ++g) {
        const float P = fast_exp2(ds[(int64_t)g * E] * kLog2e * An);
        H = P * H + eo[carry + (int64_t)g * 16 * E];
        ck[(int64_t)(g + 1) * cps * 16 * E] = H;             // chunk (g + 1) cps < nck: segment g + 1 exists
    }
    float K = 0.f;
    for (int g = G - 1; g >= 1; --g) {
        const int64_t at = carry + (int64_t)g * 16 * E;
        // the last segment's Dsum is not stored (it may be a part segment, and P_{G-1} multiplies K_{G-1} = 0)
        const float P = g + 1 < G ? fast_exp2(ds[(int64_t)g * E] * kLog2e * An) : 0.f;
        K = P * K + kap[at];
        kap[at] = K;                                         // K_{g-1}: the adjoint segment g - 1 starts from
    }
}

template <typename T>
static hipError_t launch_scan_bwd_seg_t(const ScanBwdLaunch& a, int steps, int G, hipStream_t s) {
    const ScanBwdSegCarve cv = sbs_carve(a.S, a.L, a.E, G);
    char* base = (char*)a.scratch;
    float *ckpt = (float*)(base + cv.ckpt), *part = (float*)(base + cv.part), *pA = (float*)(base + cv.pA), *pD = (float*)(base + cv.pD),
          *pbias = (float*)(base + cv.pbias), *eo = (float*)(base + cv.e), *kap = (float*)(base + cv.kap), *dsum = (float*)(base + cv.dsum);
    const dim3 grid((unsigned)((int64_t)a.S * G * (a.E / 64))), blk(64);
    const int rev = a.reverse ? 1 : 0;
    if (G > 1) {
#define PCAD_SCAN_BWD_LOCAL(GATED)                                                                                                          \
    hipLaunchKernelGGL((scan_bwd_seg_local_kernel<T, GATED>), grid, blk, 0, s, (const T*)a.u, (const T*)a.delta, (const T*)a.z, a.ldz, a.bc, \
                       a.A, a.dbias, (const T*)a.dout, eo, kap, dsum, a.L, a.E, rev, steps, G)
        if (a.z != nullptr) PCAD_SCAN_BWD_LOCAL(true);
        else PCAD_SCAN_BWD_LOCAL(false);
#undef PCAD_SCAN_BWD_LOCAL
        if (hipError_t e = hipGetLastError()) return e;
        const int64_t total = (int64_t)a.S * 16 * a.E;
        hipLaunchKernelGGL(scan_bwd_seg_combine_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.A, (const float*)eo, kap,
                           (const float*)dsum, ckpt, total, a.L, a.E, steps, G);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const ScanBwdSegArgs sa{.K = kap, .steps = steps, .G = G};
#define PCAD_SCAN_BWD(GATED, SEG)                                                                                                             \
    hipLaunchKernelGGL((scan_bwd_kernel<T, GATED, SEG>), grid, blk, 0, s, (const T*)a.u, (const T*)a.delta, (const T*)a.z, a.ldz, a.bc, a.A, \
                       a.Dskip, a.dbias, (const T*)a.dout, (T*)a.du, (T*)a.ddelta, (T*)a.dz, ckpt, part, pA, pD, pbias, a.L, a.E, rev, sa)
    if (G > 1) {
        if (a.z != nullptr) PCAD_SCAN_BWD(true, true);
        else PCAD_SCAN_BWD(false, true);
    } else {                                                 // one segment: the unsegmented kernel, the bits of launch_scan_bwd
        if (a.z != nullptr) PCAD_SCAN_BWD(true, false);
        else PCAD_SCAN_BWD(false, false);
    }
#undef PCAD_SCAN_BWD
    if (hipError_t e = hipGetLastError()) return e;
    const int64_t rows = (int64_t)a.S * a.L, n = rows * 32 + (int64_t)a.E * 18;
    hipLaunchKernelGGL(scan_bwd_reduce_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, (const float*)part, (const float*)pA,
                       (const float*)pD, (const float*)pbias, a.dbc, a.dA, a.dD, a.ddbias, rows, a.S * G, a.E);
    return hipGetLastError();
}

hipError_t launch_scan_bwd_seg(const ScanBwdLaunch& a, int segments, hipStream_t s) {
    if (a.S <= 0 || a.L <= 0 || a.E <= 0 || a.E % 64 || a.scratch == nullptr || (a.z != nullptr) != (a.dz != nullptr)) return hipErrorInvalidValue;
    const int steps = scan_bwd_seg_steps(a.L, segments);
    if (steps == 0) return hipErrorInvalidValue;
    const int G = (a.L + steps - 1) / steps;                 // <= segments
    // one wave per (strand, segment, 64 channels) and one reduce / combine thread per element, all as 32-bit grids
    if ((int64_t)a.S * G * (a.E / 64) > 0x7fffffff || ((int64_t)a.S * a.L * 32 + (int64_t)a.E * 18 + 255) / 256 > 0x7fffffff ||
        ((int64_t)a.S * 16 * a.E + 255) / 256 > 0x7fffffff)
        return hipErrorInvalidValue;
    if (a.dt == BF16) return launch_scan_bwd_seg_t<bf16_t>(a, steps, G, s);
    if (a.dt == F32) return launch_scan_bwd_seg_t<float>(a, steps, G, s);
    return hipErrorInvalidValue;
}

}  // namespace pcad
