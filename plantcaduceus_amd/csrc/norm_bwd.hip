// Backward of the fused residual-add + RMSNorm (include/pcad_bwd.h pcad_add_rmsnorm_bwd, libpcad_bwd.so).  Replaces the
// backward of mamba_ssm.ops.triton.layer_norm.rms_norm_fn for the forms Caduceus uses: no bias, with or without a residual, with or
// without the prenorm output.
//
// Per row, everything in fp32:
//   r = x + residual_in  (unrounded, as add_rmsnorm_kernel forms it; no residual_in: x)     rstd = rsqrt(mean(r^2) + eps)     rh = r rstd
//   dr_i = dresidual_out_i + rstd (w_i dy_i - rh_i (1/D) sum_j w_j dy_j rh_j)               (no dresidual_out: 0)
//   dx = round(dr) in the model dtype     dresidual_in = round(dr) in the residual dtype     dweight_i = sum_rows dy_i rh_i
// The forward saves nothing: r and rstd are recomputed from the forward's own inputs.
//
// One wave per row with 16-byte accesses, as add_rmsnorm_kernel; a wave walks a slab of NORM_BWD_ROWS consecutive rows, keeps the norm
// weight and its dweight partial in registers and stores one partial row per slab to the caller's scratch; launch_sum_partials adds
// the slabs in a fixed order.  No floating-point atomics.  The only roundings are the two stores.  All in-tensor offsets are 64-bit.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

namespace {
int64_t nb_slabs(int64_t rows) { return (rows + NORM_BWD_ROWS - 1) / NORM_BWD_ROWS; }
}  // namespace

size_t norm_bwd_bytes(int64_t rows, int D) { return ((size_t)nb_slabs(rows) * (size_t)D * sizeof(float) + 255) / 256 * 256; }

// 8 consecutive elements as they come from memory: a load is issued here and waited for only where the values are unpacked
template <typename T> struct Raw8;
template <> struct Raw8<bf16_t> {
    u32x4 r;
    __device__ __forceinline__ void load(const bf16_t* p) { r = *reinterpret_cast<const u32x4*>(p); }
    __device__ __forceinline__ void zero() { r = u32x4{0u, 0u, 0u, 0u}; }
    __device__ __forceinline__ void unpack(float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[2 * i] = bf16lo_to_f32(r[i]); v[2 * i + 1] = bf16hi_to_f32(r[i]); }
    }
};
template <> struct Raw8<float> {
    f32x4 a, b;
    __device__ __forceinline__ void load(const float* p) { a = *reinterpret_cast<const f32x4*>(p); b = *reinterpret_cast<const f32x4*>(p + 4); }
    __device__ __forceinline__ void zero() { a = f32x4{0.f, 0.f, 0.f, 0.f}; b = a; }
    __device__ __forceinline__ void unpack(float (&v)[8]) const {
#pragma unroll
        for (int i = 0; i < 4; ++i) { v[i] = a[i]; v[4 + i] = b[i]; }
    }
};

// One row's four operands, all issued together (the forward's x and residual_in, then dy and dresidual_out).  AHEAD (D <= 1024): the
// next row's loads are issued before this row's two wave reductions, so a wave always has a row in flight; at D = 2048 the second
// set of registers would halve the occupancy and the loads are issued after the row's stores instead.
template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(256) void norm_bwd_kernel(const T* __restrict__ x, const RT* __restrict__ res_in, const float* __restrict__ w,
                                                       const T* __restrict__ dy, const RT* __restrict__ dres_out, T* __restrict__ dx,
                                                       RT* __restrict__ dres_in, float* __restrict__ part, int64_t rows, int D, float eps) {
    constexpr bool AHEAD = MAXC <= 2;
    const int lane = threadIdx.x & 63;
    const int64_t slab = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t r0 = slab * NORM_BWD_ROWS;
    if (r0 >= rows) return;
    const int64_t r1 = min(rows, r0 + NORM_BWD_ROWS);
    const int nchunk = D >> 3;
    const float inv_d = 1.0f / (float)D;

    float wv[MAXC][8], dwp[MAXC][8];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
#pragma unroll
        for (int i = 0; i < 8; ++i) { wv[j][i] = 0.f; dwp[j][i] = 0.f; }
        if (c < nchunk) load8<float>(w + c * 8, wv[j]);
    }

    struct RowRaw { Raw8<T> x[MAXC], g[MAXC]; Raw8<RT> r[MAXC], d[MAXC]; };
    auto load_row = [&](int64_t row, RowRaw& q) {             // row >= r1 (wave-uniform): nothing is read
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            q.x[j].zero(); q.g[j].zero(); q.r[j].zero(); q.d[j].zero();
            if (row < r1 && c < nchunk) {
                const int64_t at = row * D + c * 8;
                q.x[j].load(x + at);
                q.g[j].load(dy + at);
                if (res_in != nullptr) q.r[j].load(res_in + at);
                if (dres_out != nullptr) q.d[j].load(dres_out + at);
            }
        }
    };

    RowRaw cur;
    load_row(r0, cur);
    for (int64_t row = r0; row < r1; ++row) {
        RowRaw nxt;
        if (AHEAD) load_row(row + 1, nxt);
        float v[MAXC][8], g[MAXC][8], dr[MAXC][8];            // chunks beyond the row are zeros throughout
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            float r[8];
            cur.x[j].unpack(v[j]);
            cur.r[j].unpack(r);
            cur.g[j].unpack(g[j]);
            cur.d[j].unpack(dr[j]);
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[j][i] += r[i];                              // zero without a residual: x + 0 = x, exactly
                ss += v[j][i] * v[j][i];
            }
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss * inv_d + eps);
        float dot = 0.f;                                      // sum_j w_j dy_j rh_j
#pragma unroll
        for (int j = 0; j < MAXC; ++j)
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[j][i] *= rstd;                              // rh
                dwp[j][i] += g[j][i] * v[j][i];
                g[j][i] *= wv[j][i];                          // w dy
                dot += g[j][i] * v[j][i];
            }
        dot = wave_sum(dot) * inv_d;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
                float o[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) o[i] = dr[j][i] + rstd * (g[j][i] - v[j][i] * dot);      // dr: zero without dresidual_out
                store8<T>(dx + row * D + c * 8, o);
                if (dres_in != nullptr) store8<RT>(dres_in + row * D + c * 8, o);
            }
        }
        if (AHEAD) cur = nxt;
        else load_row(row + 1, cur);
    }
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) store8<float>(part + slab * D + c * 8, dwp[j]);
    }
}

template <typename T, typename RT>
static hipError_t launch_norm_bwd_t(const NormBwdLaunch& a, hipStream_t s) {
    const int64_t slabs = nb_slabs(a.rows);
    const dim3 grid((unsigned)((slabs + 3) / 4)), block(256);
#define PCAD_NORM_BWD(MC)                                                                                                             \
    hipLaunchKernelGGL((norm_bwd_kernel<T, RT, MC>), grid, block, 0, s, (const T*)a.x, (const RT*)a.res_in, a.w, (const T*)a.dy,     \
                       (const RT*)a.dres_out, (T*)a.dx, (RT*)a.dres_in, (float*)a.scratch, a.rows, a.D, a.eps)
    if (a.D <= 512) PCAD_NORM_BWD(1);
    else if (a.D <= 1024) PCAD_NORM_BWD(2);
    else PCAD_NORM_BWD(4);
#undef PCAD_NORM_BWD
    if (hipError_t e = hipGetLastError()) return e;
    return launch_sum_partials((const float*)a.scratch, slabs, a.dw, a.D, nullptr, 0, s);
}

hipError_t launch_norm_bwd(const NormBwdLaunch& a, hipStream_t s) {
    if (a.rows <= 0 || a.D <= 0 || a.D % 8 || a.D > 2048) return hipErrorInvalidValue;
    if (!a.x || !a.w || !a.dy || !a.dx || !a.dw || !a.scratch || (a.res_in != nullptr) != (a.dres_in != nullptr)) return hipErrorInvalidValue;
    if ((nb_slabs(a.rows) + 3) / 4 > 0x7fffffff) return hipErrorInvalidValue;
    if (a.dt == BF16 && a.rdt == F32) return launch_norm_bwd_t<bf16_t, float>(a, s);
    if (a.dt == BF16 && a.rdt == BF16) return launch_norm_bwd_t<bf16_t, bf16_t>(a, s);
    if (a.dt == F32 && a.rdt == F32) return launch_norm_bwd_t<float, float>(a, s);
    return hipErrorInvalidValue;
}

}  // namespace pcad
