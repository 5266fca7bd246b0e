// Segmented forward of the selective scan on plain rows (include/pcad_bwd.h pcad_selective_scan_fwd_seg, libpcad_bwd.so):
// the training forward's call (pcad_selective_scan with an explicit delta) with every strand's L walk steps cut into G segments of
// `steps` = scan_bwd_seg_steps(L, segments) steps - the backward's rule, so the cuts fall on its checkpoint boundaries; the last
// segment may be shorter - and one wave owning 64 channels of one (strand, segment): lane = channel, the 16 states in registers, the
// B_t | C_t rows fetched as uniform data.  A call of few strands then fills G times as many wave slots.
//
// The recurrence h_s = a_s h_{s-1} + d_s u_s B_s, a_s[n] = exp(d_s A[c,n]), d = softplus(delta + bias), is linear in what it carries,
// so a segment maps the state it starts from to (that state) x P_g + (what it reaches from zero), P_g[n] = exp(A[c,n] sum_s d_s):
//   phase 1  scan_fwd_seg_local_kernel, one wave per (strand, segment g < G - 1, 64 channels): from h = 0 up the segment -> e_g[n] and
//            Dsum_g = sum d_s (the arithmetic of scan_bwd_seg_local_kernel's first half)
//   phase 2  scan_fwd_seg_carry_kernel, one thread per (strand, n, channel), serial over g ascending: H_0 = 0,
//            H_{g+1} = exp2(A log2e Dsum_g) H_g + e_g; H_g stored over e_g (slot g: what segment g starts from), for every segment
//   phase 3  scan_fwd_seg_walk_kernel, one wave per (strand, segment, 64 channels): from H_g, y_s = sum_n h_s[n] C_s[n] + D u_s, times
//            silu(z_s) when gated, rounded once to the dtype and stored once
// delta and u are read in the model dtype, everything in between is fp32 (the rounding points of the plain call).  No floating-point
// atomics; every sum has a fixed order, so a call is bit-reproducible for a given G.  A call with one segment (segments == 1, or
// L <= steps) runs phase 3 alone from a zero state.  All in-tensor offsets are 64-bit.
#include "scan_bwd_kernel.hpp"

namespace pcad {

namespace {
constexpr size_t sfs_align(size_t v) { return (v + 255) / 256 * 256; }
// scratch sections, each 256-byte aligned: e / H [S][G][16][E], Dsum [S][G][E] (one segment: sized the same way and not touched)
struct ScanFwdSegCarve { size_t eh, dsum, total; };
ScanFwdSegCarve sfs_carve(int S, int E, int G) {
    ScanFwdSegCarve c;
    const size_t f = sizeof(float), sg = (size_t)S * G, e = (size_t)E;
    c.eh = 0;
    c.dsum = c.eh + sfs_align(sg * 16 * e * f);
    c.total = c.dsum + sfs_align(sg * e * f);
    return c;
}
}  // namespace

size_t scan_fwd_seg_bytes(int S, int L, int E, int segments) {
    const int steps = scan_bwd_seg_steps(L, segments);
    if (steps == 0) return 0;
    return sfs_carve(S, E, (L + steps - 1) / steps).total;
}

// Phase 1.  Grid: (strand (G - 1) + g) (E / 64) + wave, g < G - 1: whole segments, steps / SBT whole chunks, all below L.
template <typename T>
__global__ __launch_bounds__(64) void scan_fwd_seg_local_kernel(const T* __restrict__ u, const T* __restrict__ delta, const float* __restrict__ bc,
                                                                const float* __restrict__ A, const float* __restrict__ dbias,
                                                                float* __restrict__ eo, float* __restrict__ dsum, int L, int E, int reverse,
                                                                int steps, int G) {
    const int lane = threadIdx.x;
    const int nw = E >> 6;
    const int w = blockIdx.x % nw;
    const int64_t item = blockIdx.x / nw;                   // strand * (G - 1) + g
    const int g = (int)(item % (G - 1));
    const int64_t strand = item / (G - 1);
    const int64_t unit = strand * G + g;
    const int c = (w << 6) + lane;                          // < E: E is a multiple of 64
    const int64_t row0 = strand * L;
    const int s0 = g * steps, s1 = s0 + steps;              // s1 < L: a later segment exists
    float Ac[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) Ac[n] = A[(int64_t)c * 16 + n];
    const float bias = dbias[c];
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
    const int64_t slot = (unit * 16) * (int64_t)E + c;      // + n * E
#pragma unroll
    for (int n = 0; n < 16; ++n) eo[slot + (int64_t)n * E] = h[n];
    dsum[unit * E + c] = ds;
}

// Phase 2.  One thread per (strand, n, channel), the channel fastest; the G segments in index order.  Slot g: e_g in, H_g out (the last
// segment's slot and Dsum are never read: nothing follows it).
__global__ __launch_bounds__(256) void scan_fwd_seg_carry_kernel(const float* __restrict__ A, float* __restrict__ eh, const float* __restrict__ dsum,
                                                                 int64_t total, int E, int G) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;                                  // total = S * 16 * E
    const int c = (int)(i % E), n = (int)((i / E) % 16);
    const int64_t strand = i / ((int64_t)E * 16);
    const float An = A[(int64_t)c * 16 + n];
    const float* ds = dsum + strand * G * (int64_t)E + c;                     // + g * E
    const int64_t carry = (strand * G * 16 + n) * (int64_t)E + c;             // + g * 16 * E
    float H = 0.f;
    for (int g = 0; g < G; ++g) {
        const int64_t at = carry + (int64_t)g * 16 * E;
        float e = 0.f, P = 0.f;
        if (g + 1 < G) {
            e = eh[at];
            P = fast_exp2(ds[(int64_t)g * E] * kLog2e * An);
        }
        eh[at] = H;                                          // H_g: the state segment g starts from
        H = P * H + e;
    }
}

// Phase 3.  Grid: (strand G + g) (E / 64) + wave.  Hs == nullptr (one segment): from a zero state.
template <typename T, bool GATED>
__global__ __launch_bounds__(64) void scan_fwd_seg_walk_kernel(const T* __restrict__ u, const T* __restrict__ delta, const T* __restrict__ z, int64_t ldz,
                                                               const float* __restrict__ bc, const float* __restrict__ A,
                                                               const float* __restrict__ Dskip, const float* __restrict__ dbias,
                                                               const float* __restrict__ Hs, T* __restrict__ y, int L, int E, int reverse,
                                                               int steps, int G) {
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
    const float bias = dbias[c], Dc = Dskip[c];
    float h[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) h[n] = 0.f;
    if (Hs != nullptr) {
        const float* src = Hs + (unit * 16) * (int64_t)E + c;
#pragma unroll
        for (int n = 0; n < 16; ++n) h[n] = src[(int64_t)n * E];
    }
    for (int sb = s0; sb < s1; sb += SBT) {                  // the strand's last segment may end inside a chunk
        const int len = min(SBT, s1 - sb);
        float uu[SBT], dd[SBT], gate[SBT];
#pragma unroll
        for (int i = 0; i < SBT; ++i) {
            if (i < len) {
                const int s = sb + i;
                const int64_t row = row0 + (reverse ? L - 1 - s : s);
                const int64_t at = row * E + c;
                uu[i] = Elem<T>::load(u + at);
                dd[i] = softplus(Elem<T>::load(delta + at) + bias);
                if (GATED) gate[i] = silu(Elem<T>::load(z + row * ldz + c));
            }
        }
#pragma unroll
        for (int i = 0; i < SBT; ++i) {
            if (i < len) {
                const int s = sb + i;
                const int64_t row = row0 + (reverse ? L - 1 - s : s);
                const float* bcr = bc + row * 32;
                const float d2 = dd[i] * kLog2e, du_ = dd[i] * uu[i];
                float yv = Dc * uu[i];
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    h[n] = fast_exp2(d2 * Ac[n]) * h[n] + du_ * bcr[n];
                    yv += h[n] * bcr[16 + n];
                }
                if (GATED) yv *= gate[i];
                Elem<T>::store(y + row * E + c, yv);
            }
        }
    }
}

template <typename T>
static hipError_t launch_scan_fwd_seg_t(const ScanFwdSegLaunch& a, int steps, int G, hipStream_t s) {
    const ScanFwdSegCarve cv = sfs_carve(a.S, a.E, G);
    char* base = (char*)a.scratch;
    float *eh = G > 1 ? (float*)(base + cv.eh) : nullptr, *dsum = G > 1 ? (float*)(base + cv.dsum) : nullptr;
    const int nw = a.E / 64, rev = a.reverse ? 1 : 0;
    const dim3 blk(64);
    if (G > 1) {
        hipLaunchKernelGGL((scan_fwd_seg_local_kernel<T>), dim3((unsigned)((int64_t)a.S * (G - 1) * nw)), blk, 0, s, (const T*)a.u,
                           (const T*)a.delta, a.bc, a.A, a.dbias, eh, dsum, a.L, a.E, rev, steps, G);
        if (hipError_t e = hipGetLastError()) return e;
        const int64_t total = (int64_t)a.S * 16 * a.E;
        hipLaunchKernelGGL(scan_fwd_seg_carry_kernel, dim3((unsigned)((total + 255) / 256)), dim3(256), 0, s, a.A, eh, (const float*)dsum, total,
                           a.E, G);
        if (hipError_t e = hipGetLastError()) return e;
    }
    const dim3 grid((unsigned)((int64_t)a.S * G * nw));
#define PCAD_SCAN_FWD_WALK(GATED)                                                                                                          \
    hipLaunchKernelGGL((scan_fwd_seg_walk_kernel<T, GATED>), grid, blk, 0, s, (const T*)a.u, (const T*)a.delta, (const T*)a.z, a.ldz, a.bc, \
                       a.A, a.Dskip, a.dbias, (const float*)eh, (T*)a.y, a.L, a.E, rev, steps, G)
    if (a.z != nullptr) PCAD_SCAN_FWD_WALK(true);
    else PCAD_SCAN_FWD_WALK(false);
#undef PCAD_SCAN_FWD_WALK
    return hipGetLastError();
}

bool scan_fwd_seg_grid_ok(int S, int L, int E, int segments) {
    const int steps = scan_bwd_seg_steps(L, segments);
    if (steps == 0 || S <= 0 || E <= 0 || E % 64) return false;
    const int G = (L + steps - 1) / steps;
    // one wave per (strand, segment, 64 channels) and one carry thread per (strand, n, channel), both as 32-bit grids
    return (int64_t)S * G * (E / 64) <= 0x7fffffff && ((int64_t)S * 16 * E + 255) / 256 <= 0x7fffffff;
}

hipError_t launch_scan_fwd_seg(const ScanFwdSegLaunch& a, int segments, hipStream_t s) {
    if (a.S <= 0 || a.L <= 0 || !scan_fwd_seg_grid_ok(a.S, a.L, a.E, segments)) return hipErrorInvalidValue;
    const int steps = scan_bwd_seg_steps(a.L, segments);
    const int G = (a.L + steps - 1) / steps;                 // <= segments
    if (a.scratch == nullptr) return hipErrorInvalidValue;
    if (a.dt == BF16) return launch_scan_fwd_seg_t<bf16_t>(a, steps, G, s);
    if (a.dt == F32) return launch_scan_fwd_seg_t<float>(a, steps, G, s);
    return hipErrorInvalidValue;
}

}  // namespace pcad
