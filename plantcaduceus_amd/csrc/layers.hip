// Per-layer hidden states at the evaluated positions: the rows of one level of the reference's `hidden_states`
// tuple that a caller reads, gathered from the 2B-strand activation tensor right after the level is produced.
//
//   source        plain rows [2B * L, D]: the mixer output h of a layer, or the RCPS embedding (level 0);
//                 or (assembled) rows [.., 2D] that final_head_kernel already wrote in the reference's layout (the last level);
//                 or (compact) the [2B, P, D] plain rows that launch_gather_rows + the small out_proj leave of a shortened block:
//                 strand b slot q = row p_q, strand B + b slot q = row L - 1 - p_q (the last executed block of a truncated walk)
//   rows read     (window b, slot q, position p): strand b row p ("fwd") and strand B + b row L - 1 - p ("rc")
//   plain form    model dtype [B, P, 2D]: [0, D) = fwd, [D, 2D) = rc with channels reversed - assemble_hidden_kernel's row (b, p), bit for bit
//   averaged form fp32 [B, P, D]: (float(fwd[c]) + float(rc[c])) * 0.5f - one fp32 add and one exact multiply: the value
//                 embeddings.extract_embeddings forms with torch from the plain row ((e[:D] + flip(e[D:])) / 2 on fp32), bit for bit
//
// Positions: a shared by-value list, or a device list per window (pos_per_window [B, P]; a value outside [0, L) is clamped and
// reported).  One WAVE per (window, slot): it reads both rows itself in 16-byte pieces and stores every output element once in
// 16-byte pieces - no hand-over between waves, no atomics on data, so a window's rows depend on that window only.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int LAYERS_STATUS_BAD_POSITION_BIT = 2;     // = pcad.h PCAD_STATUS_BAD_POSITION
constexpr int LAYERS_WAVES = 4;                       // (window, slot) items per block

// one 16-byte piece = EPV elements of T, as raw bits (a copy never passes through a float conversion)
template <typename T> struct Piece;
template <> struct Piece<float> {
    static constexpr int EPV = 4;
    static __device__ __forceinline__ u32x4 reversed(u32x4 v) { return u32x4{v[3], v[2], v[1], v[0]}; }
    static __device__ __forceinline__ void to_f32(u32x4 v, float (&f)[4]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) f[i] = __uint_as_float(v[i]);
    }
};
template <> struct Piece<bf16_t> {
    static constexpr int EPV = 8;
    static __device__ __forceinline__ u32x4 reversed(u32x4 v) {
        u32x4 r;
#pragma unroll
        for (int i = 0; i < 4; ++i) r[i] = (v[3 - i] >> 16) | (v[3 - i] << 16);
        return r;
    }
    static __device__ __forceinline__ void to_f32(u32x4 v, float (&f)[8]) {
#pragma unroll
        for (int i = 0; i < 4; ++i) { f[2 * i] = bf16lo_to_f32(v[i]); f[2 * i + 1] = bf16hi_to_f32(v[i]); }
    }
};

// ASM: src holds assembled rows of 2D elements, row of (b, q) at index b * sb + q * sq; CMP (never with ASM): compact plain rows
// [2B, P, D], the two rows of (b, q) at indices b * P + q and (B + b) * P + q; else plain rows [2B * L, D]
template <typename T, bool AVG, bool ASM, bool CMP>
__global__ __launch_bounds__(64 * LAYERS_WAVES) void layer_rows_kernel(const T* __restrict__ src, void* __restrict__ out, int B, int L, int D,
                                                                       Positions pos, const int32_t* __restrict__ pos_per_window, int P,
                                                                       int64_t sb, int64_t sq, int32_t* __restrict__ status) {
    constexpr int EPV = Piece<T>::EPV;
    const int lane = threadIdx.x & 63;
    const int64_t item = (int64_t)blockIdx.x * LAYERS_WAVES + (threadIdx.x >> 6);      // = b * P + q, wave-uniform
    if (item >= (int64_t)B * P) return;
    const int b = (int)(item / P), q = (int)(item - (int64_t)b * P);
    const T *fwd, *rc;
    if constexpr (ASM) {
        fwd = src + (b * sb + q * sq) * 2 * D;
        rc = fwd + D;
    } else if constexpr (CMP) {
        fwd = src + item * D;                            // launch_gather_rows' order: (strand * P + q), the same slot in both strands
        rc = src + ((int64_t)B * P + item) * D;
    } else {
        int p = 0;
        if (pos_per_window) {
            const int raw = pos_per_window[item];
            if (status != nullptr && lane == 0 && (unsigned)raw >= (unsigned)L) atomicOr(status, LAYERS_STATUS_BAD_POSITION_BIT);
            p = min(max(raw, 0), L - 1);         // clamped: nothing is read out of bounds
        } else {
            // uniform select from the by-value array (avoids runtime-indexed kernarg scratch)
#pragma unroll
            for (int i = 0; i < 16; ++i)
                if (i == q) p = pos.p[i];
        }
        fwd = src + ((int64_t)b * L + p) * D;
        rc = src + ((int64_t)(B + b) * L + (L - 1 - p)) * D;
    }
    const int npiece = D / EPV;
    if constexpr (!AVG) {
        T* o = (T*)out + item * 2 * D;
        for (int c = lane; c < npiece; c += 64) {
            const u32x4 f = *reinterpret_cast<const u32x4*>(fwd + c * EPV);
            const u32x4 r = *reinterpret_cast<const u32x4*>(rc + c * EPV);
            *reinterpret_cast<u32x4*>(o + c * EPV) = f;
            if constexpr (ASM) *reinterpret_cast<u32x4*>(o + D + c * EPV) = r;        // already channel-reversed
            else *reinterpret_cast<u32x4*>(o + D + (npiece - 1 - c) * EPV) = Piece<T>::reversed(r);
        }
    } else {
        float* o = (float*)out + item * D;
        for (int c = lane; c < npiece; c += 64) {
            const u32x4 f = *reinterpret_cast<const u32x4*>(fwd + c * EPV);
            // the rc strand's channels c * EPV ..: straight in the plain rows, mirrored (and reversed) in an assembled row
            u32x4 r = *reinterpret_cast<const u32x4*>(rc + (ASM ? npiece - 1 - c : c) * EPV);
            if constexpr (ASM) r = Piece<T>::reversed(r);
            float a[EPV], m[EPV];
            Piece<T>::to_f32(f, a);
            Piece<T>::to_f32(r, m);
#pragma unroll
            for (int k = 0; k < EPV; k += 4)
                *reinterpret_cast<f32x4*>(o + c * EPV + k) = f32x4{(a[k] + m[k]) * 0.5f, (a[k + 1] + m[k + 1]) * 0.5f,
                                                                    (a[k + 2] + m[k + 2]) * 0.5f, (a[k + 3] + m[k + 3]) * 0.5f};
        }
    }
}

template <typename T>
static hipError_t launch_layer_rows_t(const LayerRowsLaunch& a, hipStream_t s) {
    // the six instantiations, by [average][source: plain / assembled / compact]
    static constexpr decltype(&layer_rows_kernel<T, false, false, false>) kernels[2][3] = {
        {layer_rows_kernel<T, false, false, false>, layer_rows_kernel<T, false, true, false>, layer_rows_kernel<T, false, false, true>},
        {layer_rows_kernel<T, true, false, false>, layer_rows_kernel<T, true, true, false>, layer_rows_kernel<T, true, false, true>}};
    const int64_t blocks = ((int64_t)a.B * a.P + LAYERS_WAVES - 1) / LAYERS_WAVES;
    hipLaunchKernelGGL(kernels[a.average ? 1 : 0][a.assembled ? 1 : a.compact ? 2 : 0], dim3((unsigned)blocks), dim3(64 * LAYERS_WAVES), 0, s, (const T*)a.src, a.out,
                       a.B, a.L, a.D, a.pos, a.pos_per_window, a.P, a.sb, a.sq, a.status);
    return hipGetLastError();
}

hipError_t launch_layer_rows(const LayerRowsLaunch& a, hipStream_t s) {
    const bool shared = !a.assembled && !a.pos_per_window;
    if (a.compact && !shared) return hipErrorInvalidValue;        // the gathered rows exist for a shared list only
    if (a.D <= 0 || a.D % 8 || a.L <= 0 || a.P < 1 || a.P > 16) return hipErrorInvalidValue;
    if (shared && a.pos.n != a.P) return hipErrorInvalidValue;
    if (shared)
        for (int i = 0; i < a.P; ++i)
            if (a.pos.p[i] < 0 || a.pos.p[i] >= a.L) return hipErrorInvalidValue;
    if (((uintptr_t)a.src) % 16 || ((uintptr_t)a.out) % 16) return hipErrorInvalidValue;      // 16-byte pieces
    if (a.B <= 0) return hipSuccess;
    if (((int64_t)a.B * a.P + LAYERS_WAVES - 1) / LAYERS_WAVES > 0x7fffffff) return hipErrorInvalidValue;
    if (a.dt == BF16) return launch_layer_rows_t<bf16_t>(a, s);
    if (a.dt == F32) return launch_layer_rows_t<float>(a, s);
    return hipErrorInvalidValue;
}

// dst [P, B] = transpose of src [B, P]: one contiguous per-window position list per slot, the form final_head_kernel reads
__global__ __launch_bounds__(256) void position_columns_kernel(const int32_t* __restrict__ src, int32_t* __restrict__ dst, int B, int P) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= (int64_t)B * P) return;
    const int b = (int)(i / P), q = (int)(i - (int64_t)b * P);
    dst[(int64_t)q * B + b] = src[i];
}

hipError_t launch_position_columns(const int32_t* src, int32_t* dst, int B, int P, hipStream_t s) {
    if (B <= 0 || P <= 0) return hipSuccess;
    const int64_t n = (int64_t)B * P;
    hipLaunchKernelGGL(position_columns_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, src, dst, B, P);
    return hipGetLastError();
}

// Token-id validation of a truncated walk (pcad_forward_layers whose highest level lies below n_layer: no head runs, and the head is
// what reports ids outside [0, 8) otherwise).  n ids from `ids`, which need not be 16-byte aligned (a chunk starts at window b0, i.e.
// b0 * L ids in): `head` ids up to the first aligned one and the n - head - 4 nv behind the last whole piece are read singly by the
// first lanes of the grid, the nv pieces between them as 16-byte loads in a grid-stride loop.  A wave that saw a bad id issues ONE
// atomicOr; nothing else is written.
constexpr int IDS_STATUS_BAD_TOKEN_BIT = 1;          // = pcad.h PCAD_STATUS_BAD_TOKEN
__global__ __launch_bounds__(256) void ids_check_kernel(const int32_t* __restrict__ ids, int64_t n, int head, int64_t nv, int32_t* __restrict__ status) {
    const int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, stride = (int64_t)gridDim.x * blockDim.x;
    const int tail = (int)(n - head - 4 * nv);       // < 4
    bool bad = false;
    if (g < head) bad |= (unsigned)ids[g] > 7u;
    if (g < tail) bad |= (unsigned)ids[head + 4 * nv + g] > 7u;
    const u32x4* v = reinterpret_cast<const u32x4*>(ids + head);
    for (int64_t i = g; i < nv; i += stride) {
        const u32x4 t = v[i];
        bad |= (t[0] | t[1] | t[2] | t[3]) > 7u;     // unsigned: a negative id has its top bit set
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) atomicOr(status, IDS_STATUS_BAD_TOKEN_BIT);
}

hipError_t launch_ids_check(const int32_t* ids, int64_t n, int32_t* status, hipStream_t s) {
    if (!status || n <= 0) return hipSuccess;        // no status word bound: nothing to report to
    if (((uintptr_t)ids) % 4) return hipErrorInvalidValue;
    int64_t head = (int64_t)(((16 - ((uintptr_t)ids & 15)) & 15) / 4);
    if (head > n) head = n;
    const int64_t nv = (n - head) / 4;
    int64_t blocks = (nv + 255) / 256;
    blocks = blocks < 1 ? 1 : blocks > 1024 ? 1024 : blocks;
    hipLaunchKernelGGL(ids_check_kernel, dim3((unsigned)blocks), dim3(256), 0, s, ids, n, (int)head, nv, status);
    return hipGetLastError();
}

}  // namespace pcad
