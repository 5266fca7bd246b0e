// The selective scan's backward kernel, shared by scan_bwd.hip (libpcad_train.so: the unsegmented form) and
// scan_bwd_seg.hip (libpcad_bwd.so: the segmented form, and the unsegmented one for a call that has one segment).
//
// Walk step s = 0..L-1 visits row t = s (forward) or L-1-s (reverse); per strand and channel c, state n < 16:
//   d_t    = softplus(delta_t + bias_c)                          a_s[n] = exp(d_t A[c,n])
//   h_s[n] = a_s[n] h_{s-1}[n] + d_t u_t B_t[n]                  y_t    = sum_n h_s[n] C_t[n] + D_c u_t
// and, with g = dL/dout (out = y silu(z), or y when z is not given):
//   dy_t   = g_t silu(z_t)                                       dz_t   = g_t y_t sig(z_t) (1 + z_t (1 - sig(z_t)))
//   k_s[n] = dy_t C_t[n] + a_{s+1}[n] k_{s+1}[n]                 (walked from s = L-1 down to 0, k_L = 0)
//   dC_t[n] = sum_c dy_t h_s[n]                                  dB_t[n] = sum_c k_s[n] d_t u_t
//   du_t   = dy_t D_c + d_t sum_n k_s[n] B_t[n]
//   dd_t   = sum_n k_s[n] (A[c,n] a_s[n] h_{s-1}[n] + u_t B_t[n])          ddelta_t = dd_t sig(delta_t + bias_c)
//   dA[c,n] = sum_{strand,s} k_s[n] d_t a_s[n] h_{s-1}[n]        dD_c = sum dy_t u_t        dbias_c = sum ddelta_t
// Everything is fp32; the only roundings are the stores of du, ddelta and dz in the model dtype.
//
// The forward keeps no states, so they are recomputed.  One wave owns 64 channels of one strand (lane = channel, as scan.hip) and
//   pass A  walks the strand once and stores h every SCAN_BWD_CHUNK steps (the state each chunk starts from) to the caller's scratch;
//   pass B  takes the chunks last to first: re-runs a chunk from its checkpoint keeping h_{s-1} of its steps in registers (the
//           chunk loops are unrolled, so the [step][n] array is never indexed at run time), which also gives y_t and dz_t, then
//           walks the chunk backwards.  The adjoint a_{s+1} k_{s+1} is carried across chunks in registers.
// No floating-point atomics: dB_t | dC_t are summed over the wave's 64 channels by a transposed butterfly (32 values per lane ->
// one per lane pair in 32 exchanges, a fixed tree) and stored as per-wave partials [S L, E / 64, 32]; dA, dD and dbias are summed
// over time in registers and stored as per-strand partials; scan_bwd_reduce_kernel adds each family in index order (the
// convention of loss.hip and convx.hip).  Results are bit-reproducible.  All in-tensor offsets are 64-bit.
//
// SEG (scan_bwd_seg.hip): one wave owns 64 channels of one SEGMENT of a strand - the walk steps [g steps, min(L, (g + 1) steps)),
// `steps` a multiple of SCAN_BWD_CHUNK, so that checkpoint slot j keeps its meaning.  Pass A starts from the state in the slot of
// the segment's first chunk (written by the combine kernel; segment 0 starts from zero), pass B from the adjoint the combine kernel
// left for it (the last segment from zero), and dA, dD and dbias are stored as per-(strand, segment) partials.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int SBT = SCAN_BWD_CHUNK;

// sig(x) = 1 / (1 + exp(-x)), formed from e = exp(-|x|) so that small values keep their relative accuracy
__device__ __forceinline__ float sigmoid_f(float x) {
    const float e = fast_exp2(-__builtin_fabsf(x) * kLog2e);
    const float r = fast_rcp(1.0f + e);
    return x >= 0.0f ? r : e * r;
}

// v[0..31] of every lane -> the sum over the 64 lanes of v[j], j = lane >> 1 (both lanes of a pair hold the same bits).
// Stage with lane bit m: a lane keeps the half of its values whose index has that bit's value and receives the partner's.
__device__ __forceinline__ float wave_sum32(float (&v)[32], int lane) {
#pragma unroll
    for (int st = 0; st < 5; ++st) {
        const int half = 16 >> st, m = 32 >> st;          // compile-time after unrolling: v[] is never indexed at run time
        const bool up = (lane & m) != 0;
#pragma unroll
        for (int i = 0; i < half; ++i) {
            const float lo = v[i], hi = v[i + half];      // values first: a conditional between two array elements selects an address
            const float keep = up ? hi : lo;
            const float send = up ? lo : hi;
            v[i] = keep + __shfl_xor(send, m, 64);
        }
    }
    return v[0] + __shfl_xor(v[0], 1, 64);
}

// what the segmented form takes besides the unsegmented form's arguments (unread without SEG)
struct ScanBwdSegArgs {
    const float* K = nullptr;     // [S][G][16][E]: slot g + 1 holds the adjoint segment g starts pass B from (g < G - 1)
    int steps = 0;                // walk steps per segment, a multiple of SCAN_BWD_CHUNK
    int G = 1;                    // segments per strand = ceil(L / steps)
};

// Two waves per SIMD: the chunk's states alone are 128 registers per lane, and 256 registers with ~80 values spilled measured 1.5x faster
// than one wave per SIMD without spills (profiles/scan_bwd_timing.txt).
template <typename T, bool GATED, bool SEG>
__global__ __launch_bounds__(64) __attribute__((amdgpu_waves_per_eu(2, 2))) void scan_bwd_kernel(const T* __restrict__ u, const T* __restrict__ delta, const T* __restrict__ z, int64_t ldz,
                                                      const float* __restrict__ bc, const float* __restrict__ A,
                                                      const float* __restrict__ Dskip, const float* __restrict__ dbias,
                                                      const T* __restrict__ dout, T* __restrict__ du, T* __restrict__ ddelta,
                                                      T* __restrict__ dz, float* __restrict__ ckpt, float* __restrict__ part,
                                                      float* __restrict__ pA, float* __restrict__ pD, float* __restrict__ pbias,
                                                      int L, int E, int reverse, ScanBwdSegArgs sa) {
    const int lane = threadIdx.x;
    const int nw = E >> 6;
    const int w = blockIdx.x % nw;
    const int64_t unit = blockIdx.x / nw;                   // SEG: strand * G + segment
    const int seg = SEG ? (int)(unit % sa.G) : 0;
    const int64_t strand = SEG ? unit / sa.G : unit;
    const int c = (w << 6) + lane;                          // < E: E is a multiple of 64
    const int nck = (L + SBT - 1) / SBT;
    // the chunks [jlo, jhi) this wave walks
    const int jlo = SEG ? seg * (sa.steps / SBT) : 0;
    const int jhi = SEG ? min(nck, jlo + sa.steps / SBT) : nck;
    const int64_t row0 = strand * L;
    float Ac[16];
#pragma unroll
    for (int n = 0; n < 16; ++n) Ac[n] = A[(int64_t)c * 16 + n];
    const float bias = dbias[c], Dc = Dskip[c];
    float* ck = ckpt + strand * nck * 16 * (int64_t)E + c;    // + (chunk * 16 + n) * E

    // ---- pass A: the state every chunk but the first starts from -------------------------------------------------------------
    {
        float h[16];
#pragma unroll
        for (int n = 0; n < 16; ++n) h[n] = 0.f;
        if (SEG && jlo > 0) {                                // the state the strand reaches before this segment
            const float* src = ck + (int64_t)jlo * 16 * E;
#pragma unroll
            for (int n = 0; n < 16; ++n) h[n] = src[(int64_t)n * E];
        }
        for (int j = jlo; j + 1 < jhi; ++j) {                // whole chunks only: the last chunk's end state is not needed
            float uu[SBT], dd[SBT];
#pragma unroll
            for (int i = 0; i < SBT; ++i) {
                const int s = j * SBT + i;
                const int64_t at = (row0 + (reverse ? L - 1 - s : s)) * E + c;
                uu[i] = Elem<T>::load(u + at);
                dd[i] = softplus(Elem<T>::load(delta + at) + bias);
            }
#pragma unroll
            for (int i = 0; i < SBT; ++i) {
                const int s = j * SBT + i;
                const float* bcr = bc + (row0 + (reverse ? L - 1 - s : s)) * 32;
                const float d2 = dd[i] * kLog2e, du_ = dd[i] * uu[i];
#pragma unroll
                for (int n = 0; n < 16; ++n) h[n] = fast_exp2(d2 * Ac[n]) * h[n] + du_ * bcr[n];
            }
            float* dst = ck + (int64_t)(j + 1) * 16 * E;
#pragma unroll
            for (int n = 0; n < 16; ++n) dst[(int64_t)n * E] = h[n];
        }
    }

    // ---- pass B: chunks last to first ------------------------------------------------------------------------------------------
    float kc[16], dAc[16];          // kc = a_{s+1} k_{s+1}: the adjoint handed to the step before
#pragma unroll
    for (int n = 0; n < 16; ++n) { kc[n] = 0.f; dAc[n] = 0.f; }
    if (SEG && seg + 1 < sa.G) {                             // the adjoint the later segments hand down
        const float* src = sa.K + ((strand * sa.G + seg + 1) * 16) * (int64_t)E + c;
#pragma unroll
        for (int n = 0; n < 16; ++n) kc[n] = src[(int64_t)n * E];
    }
    float dDc = 0.f, dbc_ = 0.f;
    for (int j = jhi - 1; j >= jlo; --j) {
        const int len = min(SBT, L - j * SBT);
        float h[16], hp[SBT][16];
        if (j > 0) {
            const float* src = ck + (int64_t)j * 16 * E;
#pragma unroll
            for (int n = 0; n < 16; ++n) h[n] = src[(int64_t)n * E];
        } else {
#pragma unroll
            for (int n = 0; n < 16; ++n) h[n] = 0.f;
        }
        float uu[SBT], dd[SBT], xs[SBT], dy[SBT];           // xs = delta + bias
        // re-run the chunk: h_{s-1} of every step, y_t, dz_t
#pragma unroll
        for (int i = 0; i < SBT; ++i) {
            if (i < len) {
                const int s = j * SBT + i;
                const int64_t row = row0 + (reverse ? L - 1 - s : s);
                const int64_t at = row * E + c;
                uu[i] = Elem<T>::load(u + at);
                xs[i] = Elem<T>::load(delta + at) + bias;
                dd[i] = softplus(xs[i]);
                const float g = Elem<T>::load(dout + at);
                const float* bcr = bc + row * 32;
                const float d2 = dd[i] * kLog2e, du_ = dd[i] * uu[i];
                float y = Dc * uu[i];
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    hp[i][n] = h[n];
                    h[n] = fast_exp2(d2 * Ac[n]) * h[n] + du_ * bcr[n];
                    y += h[n] * bcr[16 + n];
                }
                if (GATED) {
                    const float zv = Elem<T>::load(z + row * ldz + c);
                    const float sg = sigmoid_f(zv);
                    dy[i] = g * (zv * sg);
                    Elem<T>::store(dz + at, g * y * (sg * (1.0f + zv * (1.0f - sg))));
                } else {
                    dy[i] = g;
                }
            }
        }
        // walk the chunk backwards
#pragma unroll
        for (int i = SBT - 1; i >= 0; --i) {
            if (i < len) {
                const int s = j * SBT + i;
                const int64_t row = row0 + (reverse ? L - 1 - s : s);
                const int64_t at = row * E + c;
                const float* bcr = bc + row * 32;
                const float d2 = dd[i] * kLog2e, du_ = dd[i] * uu[i];
                float v[32];                                 // this lane's terms of dB_t (0..15) | dC_t (16..31)
                float sB = 0.f, sD = 0.f;
#pragma unroll
                for (int n = 0; n < 16; ++n) {
                    const float Bn = bcr[n], Cn = bcr[16 + n];
                    const float an = fast_exp2(d2 * Ac[n]);
                    const float ah = an * hp[i][n];                           // a_s h_{s-1}
                    const float hs = ah + du_ * Bn;                           // h_s, the bits of the re-run
                    const float k = dy[i] * Cn + kc[n];
                    v[16 + n] = dy[i] * hs;
                    v[n] = k * du_;
                    sB += k * Bn;
                    sD += k * (Ac[n] * ah + uu[i] * Bn);
                    dAc[n] += k * (dd[i] * ah);
                    kc[n] = an * k;
                }
                const float dd_in = sD * (xs[i] > 20.0f ? 1.0f : sigmoid_f(xs[i]));
                Elem<T>::store(du + at, dy[i] * Dc + dd[i] * sB);
                Elem<T>::store(ddelta + at, dd_in);
                dDc += dy[i] * uu[i];
                dbc_ += dd_in;
                const float tot = wave_sum32(v, lane);
                if ((lane & 1) == 0) part[(row * nw + w) * 32 + (lane >> 1)] = tot;
            }
        }
    }
    const int64_t sc = unit * E + c;                         // one row of partials per strand (SEG: per strand and segment)
#pragma unroll
    for (int n = 0; n < 16; ++n) pA[sc * 16 + n] = dAc[n];
    pD[sc] = dDc;
    pbias[sc] = dbc_;
}

// one thread per output element of dbc [rows, 32] | dA [E, 16] | dD [E] | dbias [E]: its partials added in index order
// (S: the rows of pA / pD / pbias, one per strand - per strand and segment in the segmented form)
static __global__ __launch_bounds__(256) void scan_bwd_reduce_kernel(const float* __restrict__ part, const float* __restrict__ pA,
                                                              const float* __restrict__ pD, const float* __restrict__ pbias,
                                                              float* __restrict__ dbc, float* __restrict__ dA, float* __restrict__ dD,
                                                              float* __restrict__ dbias, int64_t rows, int S, int E) {
    const int64_t nbc = rows * 32, nA = (int64_t)E * 16;
    int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < nbc) {
        const int nw = E >> 6;
        const float* p = part + (i >> 5) * nw * 32 + (i & 31);
        float a = p[0];
        for (int w = 1; w < nw; ++w) a += p[(int64_t)w * 32];
        dbc[i] = a;
        return;
    }
    i -= nbc;
    const float* p;
    float* out;
    int64_t stride;
    if (i < nA) { p = pA + i; out = dA + i; stride = nA; }
    else if (i < nA + E) { p = pD + (i - nA); out = dD + (i - nA); stride = E; }
    else if (i < nA + 2 * (int64_t)E) { p = pbias + (i - nA - E); out = dbias + (i - nA - E); stride = E; }
    else return;
    float a = p[0];
    for (int s = 1; s < S; ++s) a += p[(int64_t)s * stride];
    *out = a;
}

}  // namespace pcad
