// The dropout-masked down-projection of a LoRA branch and its backward (include/pcad_bwd.h pcad_lora_down, pcad_lora_down_bwd,
// pcad_lora_dropout_mask; libpcad_bwd.so):
//   t[m, j]  = c sum_k keep(m, k) x[m, k] A[j, k]                                   forward, fp32 [M, r]
//   dA[j, k] = c sum_m keep(m, k) u[m, j] x[m, k]                                   backward, fp32 [r, K]
//   dx[m, k] = round(dx0[m, k] + c keep(m, k) sum_j u[m, j] A[j, k])                backward, IN PLACE on dx0
// keep is regenerated from (seed, stream, m, k) by lora_mask.hpp: no mask tensor and no dropped copy of x exist anywhere.
//
// A lane owns 8 consecutive columns: one 16-byte bf16 load (two for fp32) and one Philox call serve the same 8 elements.  A wave
// owns LORA_CHUNK = 512 columns.  Columns past K are padded, not masked: their lanes load nothing, hold zeros and run the same
// instruction stream, so every loop bound and every branch around a barrier is wave-uniform.
//   forward   a wave walks LORA_FWD_ROWS rows through the row's chunks in index order (A's slice of a chunk is loaded once for the
//             4 rows), then adds each of the 4 r sums over the lanes by the xor butterfly and scales by c once.
//   backward  grid (chunk, row slab).  A lane keeps A's slice [r][8] (for dx) and 8 r dA sums in registers; wave w of the block
//             takes rows w, w + 4, ... of the slab, the next row's x and dx0 are loaded before this row's arithmetic.  The waves'
//             sums are added in wave order through LDS, the block's partial goes to scratch [slab][r][K] and lora_dA_reduce_kernel
//             adds the slabs in index order, times c once.  No floating-point atomics; the order depends on (M, K) and
//             kernels.hpp's constants only.
// The products are fp32 x fp32 (A, u are fp32 by contract), so the 8 r FMAs per element go to the vector ALU: the bf16 MFMA cannot
// take an fp32 operand without rounding it, and the fp32 MFMA runs at the vector rate with 16 - r of its 16 columns padded.
#include "common.hpp"
#include "kernels.hpp"
#include "lora_mask.hpp"

namespace pcad {

int64_t lora_threshold(double p) {
    if (!(p >= 0.0) || !(p - p == 0.0)) return -1;
    const double t = p * 65536.0 + 0.5;
    return t >= 4294967296.0 ? (int64_t)4294967296 : (int64_t)t;       // floor: t >= 0
}

LoraMask lora_mask(double p, uint64_t seed, uint64_t stream_id) {
    const uint32_t T = (uint32_t)lora_threshold(p);
    return {T, 65536.0f / (float)(65536u - T), (uint32_t)seed, (uint32_t)(seed >> 32), (uint32_t)stream_id, (uint32_t)(stream_id >> 32)};
}

int64_t lora_down_bwd_slabs(int64_t M, int K, int64_t* rows_per_slab) {
    if (M <= 0) { *rows_per_slab = 0; return 0; }
    const int64_t chunks = (K + LORA_CHUNK - 1) / LORA_CHUNK;
    int64_t want = LORA_TARGET_BLOCKS / chunks;
    want = want < 1 ? 1 : want > LORA_MAX_SLABS ? LORA_MAX_SLABS : want;
    int64_t rows = (M + want - 1) / want;
    rows = (rows + LORA_SLAB_ROWS - 1) / LORA_SLAB_ROWS * LORA_SLAB_ROWS;
    *rows_per_slab = rows;
    return (M + rows - 1) / rows;
}

size_t lora_down_bwd_bytes(int64_t M, int K, int r) {
    int64_t rows;
    const int64_t slabs = lora_down_bwd_slabs(M, K, &rows);
    return ((size_t)slabs * (size_t)r * (size_t)K * sizeof(float) + 255) / 256 * 256;
}

namespace {

__device__ __forceinline__ uint32_t keep8(const LoraMask& mk, uint32_t m, int k) {
    return lora_keep8(mk.T, mk.seed_lo, mk.seed_hi, mk.stream_lo, mk.stream_hi, m, (uint32_t)k >> 3);
}

template <typename T> __device__ __forceinline__ void load8_or_zero(const T* p, bool live, float (&v)[8]) {
    if (live) {
        load8<T>(p, v);
    } else {
#pragma unroll
        for (int i = 0; i < 8; ++i) v[i] = 0.f;
    }
}

// keep_u8[m, k] = keep(m, k): one block per row (grid-strided), a lane per 8 columns
__global__ __launch_bounds__(256) void lora_mask_kernel(uint8_t* __restrict__ keep, int64_t M, int K, int64_t ldk, LoraMask mk) {
    for (int64_t m = blockIdx.x; m < M; m += gridDim.x)
        for (int k = (int)threadIdx.x * 8; k < K; k += 256 * 8) {
            const uint32_t bits = keep8(mk, (uint32_t)m, k);
#pragma unroll
            for (int i = 0; i < 8; ++i) keep[m * ldk + k + i] = (uint8_t)((bits >> i) & 1u);
        }
}

template <typename T, int R>
__global__ __launch_bounds__(256) void lora_down_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ A, float* __restrict__ t,
                                                        int64_t M, int K, LoraMask mk) {
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int64_t m0 = ((int64_t)blockIdx.x * 4 + wv) * LORA_FWD_ROWS;
    if (m0 >= M) return;                                               // wave-uniform; the kernel has no barrier
    float acc[LORA_FWD_ROWS][R];
#pragma unroll
    for (int q = 0; q < LORA_FWD_ROWS; ++q)
#pragma unroll
        for (int j = 0; j < R; ++j) acc[q][j] = 0.f;

    for (int k0 = 0; k0 < K; k0 += LORA_CHUNK) {
        const int k = k0 + lane * 8;
        const bool in = k < K;
        float xm[LORA_FWD_ROWS][8];
#pragma unroll
        for (int q = 0; q < LORA_FWD_ROWS; ++q) {
            const int64_t m = m0 + q;
            load8_or_zero<T>(x + m * ldx + k, in && m < M, xm[q]);
            const uint32_t bits = keep8(mk, (uint32_t)m, k);
#pragma unroll
            for (int i = 0; i < 8; ++i) xm[q][i] = (bits >> i) & 1u ? xm[q][i] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < R; ++j) {
            float a[8];
            load8_or_zero<float>(A + (int64_t)j * K + k, in, a);
#pragma unroll
            for (int q = 0; q < LORA_FWD_ROWS; ++q)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[q][j] = __builtin_fmaf(xm[q][i], a[i], acc[q][j]);
        }
    }
#pragma unroll
    for (int q = 0; q < LORA_FWD_ROWS; ++q) {
        float mine = 0.f;
#pragma unroll
        for (int j = 0; j < R; ++j) {
            const float s = wave_sum(acc[q][j]);
            mine = lane == j ? s : mine;
        }
        const int64_t m = m0 + q;
        if (lane < R && m < M) t[m * R + lane] = mk.c * mine;
    }
}

// grid (chunks, slabs).  part: scratch [slabs][R][K] or nullptr (dA not wanted); dx may be nullptr
template <typename T, int R>
__global__ __launch_bounds__(256) void lora_down_bwd_kernel(const T* __restrict__ x, int64_t ldx, const float* __restrict__ A,
                                                            const float* __restrict__ u, T* __restrict__ dx, int64_t lddx,
                                                            float* __restrict__ part, int64_t M, int K, int64_t rows_per_slab, LoraMask mk) {
    __shared__ float comb[R * 8 * 64];
    const int lane = threadIdx.x & 63;
    const int wv = __builtin_amdgcn_readfirstlane((int)threadIdx.x >> 6);
    const int k = (int)blockIdx.x * LORA_CHUNK + lane * 8;
    const bool in = k < K;
    const int64_t m_begin = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t m_end = m_begin + rows_per_slab < M ? m_begin + rows_per_slab : M;

    float a[R][8], acc[R][8];
#pragma unroll
    for (int j = 0; j < R; ++j) {
        load8_or_zero<float>(A + (int64_t)j * K + k, in && dx != nullptr, a[j]);
#pragma unroll
        for (int i = 0; i < 8; ++i) acc[j][i] = 0.f;
    }

    float xn[8], dn[8];
    int64_t m = m_begin + wv;
    if (m < m_end) {
        load8_or_zero<T>(x + m * ldx + k, in, xn);
        load8_or_zero<T>(dx + m * lddx + k, in && dx != nullptr, dn);
    }
    for (; m < m_end; m += 4) {                                        // wave-uniform bounds
        float xv[8], d[8];
#pragma unroll
        for (int i = 0; i < 8; ++i) { xv[i] = xn[i]; d[i] = dn[i]; }
        if (m + 4 < m_end) {
            load8_or_zero<T>(x + (m + 4) * ldx + k, in, xn);
            load8_or_zero<T>(dx + (m + 4) * lddx + k, in && dx != nullptr, dn);
        }
        const uint32_t bits = keep8(mk, (uint32_t)m, k);
        float uu[R];
#pragma unroll
        for (int j = 0; j < R; ++j) uu[j] = u[m * R + j];              // one address per wave
        if (part) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                const float xm = (bits >> i) & 1u ? xv[i] : 0.f;
#pragma unroll
                for (int j = 0; j < R; ++j) acc[j][i] = __builtin_fmaf(uu[j], xm, acc[j][i]);
            }
        }
        if (dx) {
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                float s = 0.f;
#pragma unroll
                for (int j = 0; j < R; ++j) s = __builtin_fmaf(uu[j], a[j][i], s);
                d[i] = (bits >> i) & 1u ? d[i] + mk.c * s : d[i];      // a dropped element is stored back as it was read
            }
            if (in) store8<T>(dx + m * lddx + k, d);
        }
    }

    if (!part) return;                                                 // block-uniform
    for (int w = 1; w < 4; ++w) {                                      // ((w0 + w1) + w2) + w3
        if (wv == w) {
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) comb[(j * 8 + i) * 64 + lane] = acc[j][i];
        }
        __syncthreads();
        if (wv == 0) {
#pragma unroll
            for (int j = 0; j < R; ++j)
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[j][i] += comb[(j * 8 + i) * 64 + lane];
        }
        __syncthreads();
    }
    if (wv == 0 && in) {
        float* const dst = part + (int64_t)blockIdx.y * R * K + k;
#pragma unroll
        for (int j = 0; j < R; ++j) store8<float>(dst + (int64_t)j * K, acc[j]);
    }
}

// dA[j, k..k+3] = c ((part[0] + part[1]) + ... + part[slabs - 1]); slabs == 0: zeros
__global__ __launch_bounds__(256) void lora_dA_reduce_kernel(const float* __restrict__ part, int slabs, float* __restrict__ dA, int n4, float c) {
    const int idx = (int)blockIdx.x * 256 + (int)threadIdx.x;
    if (idx >= n4) return;
    const int64_t off = (int64_t)idx * 4, stride = (int64_t)n4 * 4;
    f32x4 s = {0.f, 0.f, 0.f, 0.f};
    if (slabs > 0) s = *(const f32x4*)(part + off);
    for (int i = 1; i < slabs; ++i) s += *(const f32x4*)(part + i * stride + off);
    *(f32x4*)(dA + off) = s * c;
}

template <typename T, int R> hipError_t run_down(const LoraDownLaunch& a, hipStream_t s) {
    const int64_t blocks = (a.M + 4 * LORA_FWD_ROWS - 1) / (4 * LORA_FWD_ROWS);
    hipLaunchKernelGGL((lora_down_kernel<T, R>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)a.x, a.ldx, a.A, a.t, a.M, a.K, a.mask);
    return hipGetLastError();
}

template <typename T, int R> hipError_t run_down_bwd(const LoraDownBwdLaunch& a, int64_t slabs, int64_t rows, hipStream_t s) {
    const dim3 grid((unsigned)((a.K + LORA_CHUNK - 1) / LORA_CHUNK), (unsigned)slabs);
    hipLaunchKernelGGL((lora_down_bwd_kernel<T, R>), grid, dim3(256), 0, s, (const T*)a.x, a.ldx, a.A, a.u, (T*)a.dx, a.lddx,
                       a.dA ? (float*)a.scratch : nullptr, a.M, a.K, rows, a.mask);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_lora_dropout_mask(uint8_t* keep, int64_t M, int K, int64_t ldk, const LoraMask& mask, hipStream_t s) {
    if (M <= 0) return hipSuccess;
    const int64_t blocks = M < 65536 ? M : 65536;
    hipLaunchKernelGGL(lora_mask_kernel, dim3((unsigned)blocks), dim3(256), 0, s, keep, M, K, ldk, mask);
    return hipGetLastError();
}

#define PCAD_LORA_DISPATCH(fn, ...)                                                                         \
    do {                                                                                                    \
        const bool f32 = a.dt != BF16;                                                                  \
        switch (a.r) {                                                                                      \
            case 4: return f32 ? fn<float, 4>(__VA_ARGS__) : fn<bf16_t, 4>(__VA_ARGS__);                    \
            case 8: return f32 ? fn<float, 8>(__VA_ARGS__) : fn<bf16_t, 8>(__VA_ARGS__);                    \
            case 16: return f32 ? fn<float, 16>(__VA_ARGS__) : fn<bf16_t, 16>(__VA_ARGS__);                 \
            default: return hipErrorInvalidValue;                                                           \
        }                                                                                                   \
    } while (0)

hipError_t launch_lora_down(const LoraDownLaunch& a, hipStream_t s) {
    if (a.M <= 0) return hipSuccess;
    PCAD_LORA_DISPATCH(run_down, a, s);
}

hipError_t launch_lora_down_bwd(const LoraDownBwdLaunch& a, hipStream_t s) {
    int64_t rows = 0;
    const int64_t slabs = lora_down_bwd_slabs(a.M, a.K, &rows);
    if (slabs > 0) {
        hipError_t e = [&]() -> hipError_t { PCAD_LORA_DISPATCH(run_down_bwd, a, slabs, rows, s); }();
        if (e != hipSuccess) return e;
    }
    if (a.dA) {
        const int n4 = a.r * a.K / 4;
        hipLaunchKernelGGL(lora_dA_reduce_kernel, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, (const float*)a.scratch, (int)slabs, a.dA, n4,
                           a.mask.c);
        return hipGetLastError();
    }
    return hipSuccess;
}

}  // namespace pcad
