// Backward of the one-direction conv1d (width 4) + bias + SiLU (include/pcad_bwd.h pcad_causal_conv1d_silu_bwd, libpcad_bwd.so; DESIGN.md
// §4m), plain token-major rows.  Replaces the backward of causal_conv1d.causal_conv1d_fn(x, weight, bias, activation="silu").
//
// Per strand and channel, rows outside [0, L) contributing zero, g = dL/dout:
//   causal:       a_t = b + sum_k w[k] x[t-3+k]     dx_t = sum_k w[k] da_{t+3-k}     dw[k] = sum_{s,t} da_t x[t-3+k]
//   anti-causal:  a_t = b + sum_k w[k] x[t+3-k]     dx_t = sum_k w[k] da_{t-3+k}     dw[k] = sum_{s,t} da_t x[t+3-k]
//   da_t = g_t sig(a_t) (1 + a_t (1 - sig(a_t)))    db = sum_{s,t} da_t
// The anti-causal conv is the causal one on the rows taken last to first, so the kernel walks steps j = 0..L-1 over row t = j (causal)
// or t = L-1-j (anti-causal) and both directions are the first line in walk space.
//
// The forward saves nothing and its rounded output cannot be inverted, so a_j is recomputed from x in fp32 in conv_dir_kernel's
// accumulation order (bias, then taps 0..3).  As there, a lane owns 16 bytes of a row (8 bf16 / 4 fp32 channels) and CONV_BWD_SEG
// consecutive walk steps; it slides the x and da windows, so every row of x and dout is read once plus the halo of its segment (3 rows
// of x behind; 3 rows of x and dout ahead, whose da the lane recomputes for its own last dx rows instead of exchanging them - the
// neighbouring segment forms the same bits), keeps the taps and its dw (V x 4) and db (V) partials in registers and stores them once
// per (strand, segment) to the caller's scratch; launch_sum_partials adds the rows in a fixed order.  No floating-point atomics.
// All products and sums are fp32; the only rounding is the store of dx in the model dtype.  All in-tensor offsets are 64-bit.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

namespace {
constexpr int CBS = CONV_BWD_SEG;
constexpr int CBU = 2;              // walk steps per unrolled group: the rows of the next group are in flight while this one is computed (4: 256 registers in bf16, one wave per SIMD)

template <typename T> struct Vec16;
template <> struct Vec16<bf16_t> {
    typedef u32x4 type; enum { N = 8 };
    static __device__ __forceinline__ void unpack(const u32x4& r, float (&v)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = bf16lo_to_f32(r[i]); v[2 * i + 1] = bf16hi_to_f32(r[i]); }
    }
    static __device__ __forceinline__ void store(bf16_t* p, const float (&v)[8]) { store8<bf16_t>(p, v); }
};
template <> struct Vec16<float> {
    typedef f32x4 type; enum { N = 4 };
    static __device__ __forceinline__ void unpack(const f32x4& r, float (&v)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) v[i] = r[i];
    }
    static __device__ __forceinline__ void store(float* p, const float (&v)[4]) { *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]}; }
};

// sig(x) = 1 / (1 + exp(-x)), formed from e = exp(-|x|) so that small values keep their relative accuracy (as scan_bwd.hip)
__device__ __forceinline__ float sigmoid_acc(float x) {
    const float e = fast_exp2(-__builtin_fabsf(x) * kLog2e);
    const float r = fast_rcp(1.0f + e);
    return x >= 0.0f ? r : e * r;
}
}  // namespace

size_t conv_bwd_bytes(int S, int L, int E) {
    const size_t P = (size_t)S * (size_t)((L + CBS - 1) / CBS);
    return (P * 5 * (size_t)E * sizeof(float) + 255) / 256 * 256;
}

template <typename T, bool REV>
__global__ __launch_bounds__(256) void conv_bwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ w,
                                                       const float* __restrict__ bw, const T* __restrict__ dout, T* __restrict__ dx,
                                                       float* __restrict__ part, int S, int L, int E) {
    typedef typename Vec16<T>::type raw_t;
    constexpr int V = Vec16<T>::N;
    const int nchunk = E / V;
    const int nseg = (L + CBS - 1) / CBS;
    const int64_t total = (int64_t)S * nseg * nchunk;
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % nchunk) * V;
    const int64_t rb = i / nchunk;                    // = strand * nseg + segment: the row of this lane's partials
    const int s = (int)(rb / nseg);
    const int j0 = (int)(rb - (int64_t)s * nseg) * CBS;
    const int j1 = min(L, j0 + CBS);
    const int jend = min(L, j1 + 3);                  // walk steps [j1, jend): the halo ahead, whose da only this segment's last dx rows need

    float wv[V][4], bv[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        const f32x4 a = *reinterpret_cast<const f32x4*>(w + (int64_t)(c + e) * 4);
#pragma unroll
        for (int k = 0; k < 4; ++k) wv[e][k] = a[k];
        bv[e] = bw[c + e];
    }

    // walk step j -> row of the strand; steps outside [0, jend) are the conv's zero padding or not this lane's to read: never another strand's
    auto xrow = [&](int j) -> raw_t {
        if (j < 0 || j >= jend) return raw_t{0, 0, 0, 0};
        return *reinterpret_cast<const raw_t*>(x + ((int64_t)s * L + (REV ? L - 1 - j : j)) * ldx + c);
    };
    auto grow = [&](int j) -> raw_t {
        if (j >= jend) return raw_t{0, 0, 0, 0};
        return *reinterpret_cast<const raw_t*>(dout + ((int64_t)s * L + (REV ? L - 1 - j : j)) * E + c);
    };

    // for the group starting at step j: ext[q] = x_{j-3+q}, dae[q] = da_{j-3+q}, q = 0 .. 3 + CBU - 1; [0..2] carried from the previous
    // group (da before the segment is never used: the first dx row this lane stores is j0, which needs da_{j0} .. da_{j0+3})
    float ext[3 + CBU][V], dae[3 + CBU][V];
#pragma unroll
    for (int q = 0; q < 3; ++q) {
        Vec16<T>::unpack(xrow(j0 - 3 + q), ext[q]);
#pragma unroll
        for (int e = 0; e < V; ++e) dae[q][e] = 0.f;
    }
    raw_t nx[CBU], ng[CBU];
#pragma unroll
    for (int k = 0; k < CBU; ++k) { nx[k] = xrow(j0 + k); ng[k] = grow(j0 + k); }

    float dwp[V][4], dbp[V];
#pragma unroll
    for (int e = 0; e < V; ++e) {
        dbp[e] = 0.f;
#pragma unroll
        for (int k = 0; k < 4; ++k) dwp[e][k] = 0.f;
    }

    for (int j = j0; j < j1 + 3; j += CBU) {
        raw_t cg[CBU];
#pragma unroll
        for (int k = 0; k < CBU; ++k) { Vec16<T>::unpack(nx[k], ext[3 + k]); cg[k] = ng[k]; }
#pragma unroll
        for (int k = 0; k < CBU; ++k) { nx[k] = xrow(j + CBU + k); ng[k] = grow(j + CBU + k); }      // rows of the NEXT group, in flight
#pragma unroll
        for (int k = 0; k < CBU; ++k) {
            const int jj = j + k;
            float g[V];
            Vec16<T>::unpack(cg[k], g);                       // zero from step jend on: da = 0 there
            const bool own = jj < j1;                         // the halo's da belongs to the next segment's dw and db
#pragma unroll
            for (int e = 0; e < V; ++e) {
                float a = bv[e];
#pragma unroll
                for (int q = 0; q < 4; ++q) a += wv[e][q] * ext[k + q][e];           // x_{jj-3+q}
                const float sg = sigmoid_acc(a);
                const float da = g[e] * (sg * (1.0f + a * (1.0f - sg)));
                dae[3 + k][e] = da;
                const float mine = own ? da : 0.f;
#pragma unroll
                for (int q = 0; q < 4; ++q) dwp[e][q] += mine * ext[k + q][e];
                dbp[e] += mine;
            }
            if (jj >= j0 + 3 && jj < j1 + 3) {                // dx_{jj-3} = w[0] da_jj + w[1] da_{jj-1} + w[2] da_{jj-2} + w[3] da_{jj-3}
                float o[V];
#pragma unroll
                for (int e = 0; e < V; ++e)
                    o[e] = wv[e][0] * dae[3 + k][e] + wv[e][1] * dae[2 + k][e] + wv[e][2] * dae[1 + k][e] + wv[e][3] * dae[k][e];
                const int jo = jj - 3;                        // in [j0, j1): inside the strand
                Vec16<T>::store(dx + ((int64_t)s * L + (REV ? L - 1 - jo : jo)) * E + c, o);
            }
        }
#pragma unroll
        for (int q = 0; q < 3; ++q)
#pragma unroll
            for (int e = 0; e < V; ++e) { ext[q][e] = ext[q + CBU][e]; dae[q][e] = dae[q + CBU][e]; }
    }

    float* pr = part + rb * 5 * (int64_t)E;                   // [dw: E x 4 | db: E]
#pragma unroll
    for (int e = 0; e < V; ++e) *reinterpret_cast<f32x4*>(pr + (int64_t)(c + e) * 4) = f32x4{dwp[e][0], dwp[e][1], dwp[e][2], dwp[e][3]};
#pragma unroll
    for (int e = 0; e < V; e += 4) *reinterpret_cast<f32x4*>(pr + 4 * (int64_t)E + c + e) = f32x4{dbp[e], dbp[e + 1], dbp[e + 2], dbp[e + 3]};
}

// ---- the partial rows of conv_bwd_kernel and norm_bwd_kernel added in a fixed order -------------------------------------------------
// A block owns 32 consecutive outputs (128 contiguous bytes of every row); its SP_SLICES groups of 32 threads each add the rows of one
// slice of P (ceil(P / SP_SLICES) consecutive rows) in index order, and the first group adds the slice sums in index order.  The order
// depends on P alone.  (Eight slices left a thread 1024 dependent adds at the norm's 8192 slabs and the kernel on 32 blocks.)
constexpr int SP_SLICES = 32;
__global__ __launch_bounds__(32 * SP_SLICES) void sum_partials_kernel(const float* __restrict__ part, int64_t P, int n, float* __restrict__ out0,
                                                                      int n0, float* __restrict__ out1) {
    __shared__ float sl[SP_SLICES][32];
    const int o = threadIdx.x & 31, q = threadIdx.x >> 5;
    const int i = blockIdx.x * 32 + o;
    const int64_t per = (P + SP_SLICES - 1) / SP_SLICES;
    const int64_t p0 = q * per, p1 = min(P, p0 + per);
    float acc = 0.f;
    if (i < n)
        for (int64_t p = p0; p < p1; ++p) acc += part[p * n + i];
    sl[q][o] = acc;
    __syncthreads();
    if (q == 0 && i < n) {
        float a = sl[0][o];
#pragma unroll
        for (int k = 1; k < SP_SLICES; ++k) a += sl[k][o];
        if (i < n0) out0[i] = a;
        else out1[i - n0] = a;
    }
}

hipError_t launch_sum_partials(const float* part, int64_t P, float* out0, int n0, float* out1, int n1, hipStream_t s) {
    const int n = n0 + n1;
    if (P <= 0 || n0 <= 0 || n1 < 0 || !part || !out0 || (n1 > 0 && !out1)) return hipErrorInvalidValue;
    hipLaunchKernelGGL(sum_partials_kernel, dim3((unsigned)((n + 31) / 32)), dim3(32 * SP_SLICES), 0, s, part, P, n, out0, n0, out1);
    return hipGetLastError();
}

template <typename T>
static hipError_t launch_conv_bwd_t(const ConvBwdLaunch& a, unsigned nb, hipStream_t s) {
    const auto kernel = a.reverse ? conv_bwd_kernel<T, true> : conv_bwd_kernel<T, false>;
    hipLaunchKernelGGL(kernel, dim3(nb), dim3(256), 0, s, (const T*)a.x, a.ldx, a.w, a.b, (const T*)a.dout, (T*)a.dx, (float*)a.scratch, a.S, a.L, a.E);
    if (hipError_t e = hipGetLastError()) return e;
    return launch_sum_partials((const float*)a.scratch, (int64_t)a.S * ((a.L + CBS - 1) / CBS), a.dw, 4 * a.E, a.db, a.E, s);
}

hipError_t launch_conv_bwd(const ConvBwdLaunch& a, hipStream_t s) {
    if (a.dt != BF16 && a.dt != F32) return hipErrorInvalidValue;
    const int V = a.dt == BF16 ? 8 : 4;
    if (a.S <= 0 || a.L <= 0 || a.E <= 0 || a.E % V || a.ldx < a.E || a.ldx % V) return hipErrorInvalidValue;
    if (!a.x || !a.w || !a.b || !a.dout || !a.dx || !a.dw || !a.db || !a.scratch) return hipErrorInvalidValue;
    if ((int64_t)a.E * 5 > 0x7fffffff) return hipErrorInvalidValue;
    const int64_t total = (int64_t)a.S * ((a.L + CBS - 1) / CBS) * (a.E / V);
    const int64_t nb = (total + 255) / 256;
    if (nb > 0x7fffffff) return hipErrorInvalidValue;
    if (a.dt == BF16) return launch_conv_bwd_t<bf16_t>(a, (unsigned)nb, s);
    return launch_conv_bwd_t<float>(a, (unsigned)nb, s);
}

}  // namespace pcad
