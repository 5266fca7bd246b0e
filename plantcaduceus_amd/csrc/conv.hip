// Depth-wise conv1d (width 4) + bias + SiLU, causal AND anti-causal in one pass, token-major.
//
// Replaces causal_conv1d.causal_conv1d_fn(x, weight, bias, activation="silu") (causal-conv1d 1.4.0;
// SURVEY.md §2b K2).  The reference calls it 4x per layer on channels-first (B,E,L) tensors and feeds the
// reverse Mamba a flipped COPY of the sequence; here the reverse direction is the anti-causal conv
//   y_rev[t] = silu(b + sum_k w[k] * x[t + 3 - k])
// on the same rows, so one read of x produces both directions (HBM-bound: 1 read + 2 writes of S*L*E).
//
// A thread owns 8 channels (16-byte vectors; a wave covers 1 KiB of a row) and slides a 7-row window
// x[t-3 .. t+3] along SEG consecutive timesteps: the 2 x (4 taps + bias) x 8 channel weights are loaded once
// per thread instead of once per output, every x row is read once (+6 halo rows per segment), and the rows
// of the next 4-step group are in flight while the current group is computed.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int CONV_SEG = 64;   // timesteps per thread
constexpr int CONV_UN = 4;     // timesteps per unrolled group

template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> { typedef u32x4 type; };
template <> struct Raw8<float> { struct type { f32x4 a, b; }; };

template <typename T> __device__ __forceinline__ typename Raw8<T>::type raw_load8(const T* p);
template <> __device__ __forceinline__ u32x4 raw_load8<bf16_t>(const bf16_t* p) { return *reinterpret_cast<const u32x4*>(p); }
template <> __device__ __forceinline__ Raw8<float>::type raw_load8<float>(const float* p) {
    Raw8<float>::type r;
    r.a = *reinterpret_cast<const f32x4*>(p);
    r.b = *reinterpret_cast<const f32x4*>(p + 4);
    return r;
}
__device__ __forceinline__ void raw_unpack(const u32x4& r, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[2 * i] = bf16lo_to_f32(r[i]); v[2 * i + 1] = bf16hi_to_f32(r[i]); }
}
__device__ __forceinline__ void raw_unpack(const Raw8<float>::type& r, float (&v)[8]) {
#pragma unroll
    for (int i = 0; i < 4; ++i) { v[i] = r.a[i]; v[4 + i] = r.b[i]; }
}
template <typename R> __device__ __forceinline__ R raw_zero();
template <> __device__ __forceinline__ u32x4 raw_zero<u32x4>() { return u32x4{0u, 0u, 0u, 0u}; }
template <> __device__ __forceinline__ Raw8<float>::type raw_zero<Raw8<float>::type>() {
    Raw8<float>::type r;
    r.a = f32x4{0.f, 0.f, 0.f, 0.f};
    r.b = r.a;
    return r;
}

template <typename T>
__global__ __launch_bounds__(256) void conv_bidir_kernel(const T* __restrict__ x, int64_t ldx,
                                                         const float* __restrict__ wf, const float* __restrict__ bfw,
                                                         const float* __restrict__ wr, const float* __restrict__ brw,
                                                         T* __restrict__ yf, T* __restrict__ yr, int S, int L, int E,
                                                         int out_blocked, int in_blocked) {
    typedef typename Raw8<T>::type raw_t;
    const int nchunk = E >> 3;
    const int nseg = (L + CONV_SEG - 1) / CONV_SEG;
    const int64_t total = (int64_t)S * nseg * nchunk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % nchunk) * 8;
    const int64_t rb = i / nchunk;
    const int s = (int)(rb / nseg);
    const int t0 = (int)(rb - (int64_t)s * nseg) * CONV_SEG;
    const int t1 = min(L, t0 + CONV_SEG);
    const T* xs = x + (int64_t)s * L * ldx + c;
    const int64_t pieces = ((int64_t)E * sizeof(T)) >> 7;

    float wfv[8][4], wrv[8][4], bfv[8], brv[8];
#pragma unroll
    for (int e = 0; e < 8; ++e) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(wf + (int64_t)(c + e) * 4);
        const f32x4 b = *reinterpret_cast<const f32x4*>(wr + (int64_t)(c + e) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) { wfv[e][k] = a[k]; wrv[e][k] = b[k]; }
    }
    load8<float>(bfw + c, bfv);
    load8<float>(brw + c, brv);

    auto row = [&](int t) -> raw_t {
        if (t < 0 || t >= L) return raw_zero<raw_t>();
        if (in_blocked) return raw_load8<T>(x + blocked_off((int64_t)s * L + t, (int64_t)c * sizeof(T), pieces) / (int64_t)sizeof(T));
        return raw_load8<T>(xs + (int64_t)t * ldx);
    };

    // ext[j] = x[t - 3 + j], j = 0..10 for the group starting at t; ext[0..6] carried, ext[7..10] prefetched
    float ext[7 + CONV_UN][8];
#pragma unroll
    for (int j = 0; j < 7; ++j) raw_unpack(row(t0 - 3 + j), ext[j]);
    raw_t nxt[CONV_UN];
#pragma unroll
    for (int j = 0; j < CONV_UN; ++j) nxt[j] = row(t0 + 4 + j);

    for (int t = t0; t < t1; t += CONV_UN) {
#pragma unroll
        for (int j = 0; j < CONV_UN; ++j) raw_unpack(nxt[j], ext[7 + j]);
#pragma unroll
        for (int j = 0; j < CONV_UN; ++j) nxt[j] = row(t + CONV_UN + 4 + j);     // rows of the NEXT group, in flight
#pragma unroll
        for (int k = 0; k < CONV_UN; ++k) {
            if (t + k < t1) {
                float of[8], orv[8];
#pragma unroll
                for (int e = 0; e < 8; ++e) {
                    float af = bfv[e], ar = brv[e];
#pragma unroll
                    for (int q = 0; q < 4; ++q) {
                        af += wfv[e][q] * ext[k + q][e];          // x[t+k - 3 + q]
                        ar += wrv[e][q] * ext[k + 6 - q][e];      // x[t+k + 3 - q]
                    }
                    of[e] = silu(af);
                    orv[e] = silu(ar);
                }
                const int64_t orow = (int64_t)s * L + t + k;
                const int64_t o = out_blocked ? blocked_off(orow, (int64_t)c * sizeof(T), ((int64_t)E * sizeof(T)) >> 7) / (int64_t)sizeof(T)
                                              : orow * E + c;
                if (yf != nullptr) store8<T>(yf + o, of);
                if (yr != nullptr) store8<T>(yr + o, orv);
            }
        }
#pragma unroll
        for (int j = 0; j < 7; ++j)
#pragma unroll
            for (int e = 0; e < 8; ++e) ext[j][e] = ext[j + CONV_UN][e];
    }
}

template <typename T>
static void launch_conv_bidir_t(const ConvLaunch& c, unsigned nb, hipStream_t s) {
    hipLaunchKernelGGL(conv_bidir_kernel<T>, dim3(nb), dim3(256), 0, s, (const T*)c.x, c.ldx, c.fwd.w, c.fwd.b, c.rev.w, c.rev.b, (T*)c.fwd.y, (T*)c.rev.y,
                       c.S, c.L, c.E, (int)c.out_blocked, (int)c.in_blocked);
}

hipError_t launch_conv_bidir(const ConvLaunch& c, hipStream_t s) {
    const int S = c.S, L = c.L, E = c.E;
    if (S <= 0 || L <= 0) return hipSuccess;
    if (E % 8) return hipErrorInvalidValue;
    if (c.out_blocked && (E * (c.dt == BF16 ? 2 : 4)) % 128) return hipErrorInvalidValue;
    const int64_t total = (int64_t)S * ((L + CONV_SEG - 1) / CONV_SEG) * (E >> 3);
    const int64_t nb = (total + 255) / 256;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    if (c.dt == BF16) launch_conv_bidir_t<bf16_t>(c, (unsigned)nb, s);
    else launch_conv_bidir_t<float>(c, (unsigned)nb, s);
    return hipGetLastError();
}

// ---- one direction ---------------------------------------------------------------------------------------------------
// The untied-directions form (api.hip "untied_directions") gives each direction its own in_proj, hence its own x: one read of x can no
// longer feed both convolutions, so this kernel reads ONE x and writes ONE xc, causal (REV = false) or anti-causal (REV = true).
// HBM-bound at 2 E s bytes per row (one read, one write).  A lane owns 16 bytes of a row (8 bf16 / 4 fp32 channels), so 8 consecutive
// lanes move one 128-byte piece - one piece of the blocked layout, or 128 contiguous bytes of a plain row - per access, and slides a
// 4-row window along CONV_SEG consecutive timesteps of its direction: every row is read once (+ the 3-row halo per segment, straight
// from L2: no LDS), the taps are loaded once per thread, and the rows of the next 4-step group are in flight while the current one is
// computed.  Per output the products are accumulated in conv_bidir_kernel's order (bias, then taps 0..3), so with the same taps and
// the same x the values are conv_bidir_kernel's, bit for bit.
template <typename T> struct Raw16;
template <> struct Raw16<bf16_t> {
    typedef u32x4 type; enum { N = 8 };
    static __device__ __forceinline__ void unpack(const u32x4& r, float (&v)[8]) { raw_unpack(r, v); }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) { store8<bf16_t>(p, v); }
};
template <> struct Raw16<float> {
    typedef f32x4 type; enum { N = 4 };
    static __device__ __forceinline__ void unpack(const f32x4& r, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = r[i];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};

template <typename T, bool REV>
__global__ __launch_bounds__(256) void conv_dir_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                       const float* __restrict__ bw, T* __restrict__ y, int64_t ldy, int S, int L, int E,
                                                       int out_blocked, int in_blocked) {
    typedef typename Raw16<T>::type raw_t;
    constexpr int V = Raw16<T>::N;
    const int nchunk = E / V;
    const int nseg = (L + CONV_SEG - 1) / CONV_SEG;
    const int64_t total = (int64_t)S * nseg * nchunk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % nchunk) * V;
    const int64_t rb = i / nchunk;
    const int s = (int)(rb / nseg);
    const int t0 = (int)(rb - (int64_t)s * nseg) * CONV_SEG;
    const int t1 = min(L, t0 + CONV_SEG);
    const int64_t pieces = ((int64_t)E * sizeof(T)) >> 7;

    float wv[V][4], bv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(w + (int64_t)(c + e) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[e][k] = a[k];
        bv[e] = bw[c + e];
    }

    auto row = [&](int t) -> raw_t {                  // rows outside the strand are the conv's zero padding: never another strand's
        if (t < 0 || t >= L) return raw_t{0, 0, 0, 0};
        if (in_blocked) return *reinterpret_cast<const raw_t*>(x + blocked_off((int64_t)s * L + t, (int64_t)c * sizeof(T), pieces) / (int64_t)sizeof(T));
        return *reinterpret_cast<const raw_t*>(x + ((int64_t)s * L + t) * ldx + c);
    };

    // ext[j] = x[t + sh + j], j = 0 .. 3 + CONV_UN - 1, for the group starting at t; sh = -3 (causal: x[t-3 .. t]) or 0 (anti-causal:
    // x[t .. t+3]); ext[0..2] carried from the previous group, ext[3..] prefetched
    constexpr int sh = REV ? 0 : -3;
    float ext[3 + CONV_UN][V];
#pragma unroll
    for (int j = 0; j < 3; ++j) Raw16<T>::unpack(row(t0 + sh + j), ext[j]);
    raw_t nxt[CONV_UN];
#pragma unroll
    for (int j = 0; j < CONV_UN; ++j) nxt[j] = row(t0 + sh + 3 + j);

    for (int t = t0; t < t1; t += CONV_UN) {
#pragma unroll
        for (int j = 0; j < CONV_UN; ++j) Raw16<T>::unpack(nxt[j], ext[3 + j]);
#pragma unroll
        for (int j = 0; j < CONV_UN; ++j) nxt[j] = row(t + CONV_UN + sh + 3 + j);     // rows of the NEXT group, in flight
#pragma unroll
        for (int k = 0; k < CONV_UN; ++k) {
            if (t + k < t1) {
                float o[V];
#pragma unroll
                for (int e = 0; e < V; ++e) {
                    float a = bv[e];
#pragma unroll
                    for (int q = 0; q < 4; ++q) a += wv[e][q] * ext[REV ? k + 3 - q : k + q][e];      // x[t+k + 3 - q] / x[t+k - 3 + q]
                    o[e] = silu(a);
                }
                const int64_t orow = (int64_t)s * L + t + k;
                const int64_t off = out_blocked ? blocked_off(orow, (int64_t)c * sizeof(T), pieces) / (int64_t)sizeof(T) : orow * ldy + c;
                Raw16<T>::store(y + off, o);
            }
        }
#pragma unroll
        for (int j = 0; j < 3; ++j)
#pragma unroll
            for (int e = 0; e < V; ++e) ext[j][e] = ext[j + CONV_UN][e];
    }
}

template <typename T>
static void launch_conv_dir_t(const ConvLaunch& c, bool reverse, unsigned nb, hipStream_t s) {
    const ConvDirection& d = reverse ? c.rev : c.fwd;
    const auto kernel = reverse ? conv_dir_kernel<T, true> : conv_dir_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, s, (const T*)c.x, c.ldx, d.w, d.b, (T*)d.y, c.ldy, c.S, c.L, c.E, (int)c.out_blocked, (int)c.in_blocked);
}

hipError_t launch_conv_dir(const ConvLaunch& c, bool reverse, hipStream_t s) {
    const int S = c.S, L = c.L, E = c.E;
    if (S <= 0 || L <= 0) return hipSuccess;
    const int esz = c.dt == BF16 ? 2 : 4, V = 16 / esz;
    const ConvDirection& d = reverse ? c.rev : c.fwd;
    if (!d.w || !d.b || !d.y) return hipErrorInvalidValue;       // the side that `reverse` names was not filled in
    if (E <= 0 || E % V || (!c.in_blocked && (c.ldx < E || c.ldx % V)) || (!c.out_blocked && (c.ldy < E || c.ldy % V))) return hipErrorInvalidValue;
    if ((c.out_blocked || c.in_blocked) && (E * esz) % 128) return hipErrorInvalidValue;
    const int64_t total = (int64_t)S * ((L + CONV_SEG - 1) / CONV_SEG) * (E / V);
    const int64_t nb = (total + 255) / 256;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    if (c.dt == BF16) launch_conv_dir_t<bf16_t>(c, reverse, (unsigned)nb, s);
    else launch_conv_dir_t<float>(c, reverse, (unsigned)nb, s);
    return hipGetLastError();
}

}  // namespace pcad
