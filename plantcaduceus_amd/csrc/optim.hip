// One AdamW step with global-norm gradient clipping over a whole parameter set, the zeroing of its gradients, and their gathering into
// one fp32 buffer for a collective (include/pcad_bwd.h pcad_adamw_step / pcad_zero_grads / pcad_grads_gather, libpcad_bwd.so).  Replaces torch.nn.utils.clip_grad_norm_ + torch.optim.AdamW.step
// (and zero_grad) with a fixed number of launches however many tensors the set has.
//
// The set is a table of pcad_optim_tensor records in device memory and a chunk map beside it (pcad_optim_plan): chunk c is elements
// [OPTIM_CHUNK * map[2c+1], ... + OPTIM_CHUNK) of tensor map[2c], cut at the tensor's end.  One block of 256 lanes per chunk, so what a
// block does is a function of the table alone - not of the grid, not of the device.
//   1. optim_sumsq_kernel    part[c] = sum over the chunk of (grad_scale g)^2: a lane adds its elements in index order (vector k of the
//                            chunk belongs to lane k % 256), the 64 lanes of a wave by the xor butterfly, the 4 waves in index order
//   2. optim_finalise_kernel one block of 1024 lanes: lane t adds part[t], part[t + 1024], ... in index order, then the same wave / block
//                            tree; lane 0 writes norm, coef, finite and bumps `skipped` in the state block (plain vector stores)
//   3. optim_update_kernel   the AdamW arithmetic per element in fp32, coef read from the state block; finite == 0: nothing is stored
// No floating-point atomics, every sum in a fixed order: two calls from equal states give equal bits.  All accesses are 16 bytes per
// lane except a tensor's last n % 4 (fp32) / n % 8 (bf16) elements, which one lane walks one by one; nothing past n is read or written.
#include "../../include/pcad_bwd.h"
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

static_assert(OPTIM_CHUNK == PCAD_OPTIM_CHUNK, "kernels.hpp and pcad_bwd.h disagree on the chunk size");
static_assert(sizeof(pcad_optim_tensor) == 64, "pcad_optim_tensor is 64 bytes");
static_assert(OPTIM_CHUNK % (256 * 8) == 0, "a chunk is a whole number of 16-byte vectors per lane in either dtype");

size_t optim_scratch_bytes(int64_t chunks) { return chunks <= 0 ? 0 : ((size_t)chunks * sizeof(float) + 255) / 256 * 256; }

namespace {

template <typename T> struct Vec;                 // the elements of one 16-byte access
template <> struct Vec<float> { static constexpr int N = 4; };
template <> struct Vec<bf16_t> { static constexpr int N = 8; };

// V consecutive elements <-> V floats: V = 8 is common.hpp's load8 / store8 (one 16-byte access in bf16, two in fp32), V = 4 one fp32 access
template <typename T, int V> __device__ __forceinline__ void loadv(const T* p, float (&v)[V]) {
    if constexpr (V == 8) {
        load8<T>(p, v);
    } else {
        static_assert(V == 4 && sizeof(T) == 4, "4 at a time: fp32 only");
        const f32x4 a = *reinterpret_cast<const f32x4*>(p);
        v[0] = a[0]; v[1] = a[1]; v[2] = a[2]; v[3] = a[3];
    }
}
template <typename T, int V> __device__ __forceinline__ void storev(T* p, const float (&v)[V]) {
    if constexpr (V == 8) {
        store8<T>(p, v);
    } else {
        static_assert(V == 4 && sizeof(T) == 4, "4 at a time: fp32 only");
        *reinterpret_cast<f32x4*>(p) = f32x4{v[0], v[1], v[2], v[3]};
    }
}

// the 256 lanes' values: the 64 of a wave by the xor butterfly, the 4 (or 16) wave sums in index order; every lane returns the total
template <int WAVES> __device__ __forceinline__ float block_sum(float v, float* lds) {
    v = wave_sum(v);
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = v;
    __syncthreads();
    float t = 0.f;
#pragma unroll
    for (int w = 0; w < WAVES; ++w) t += lds[w];
    return t;
}

struct Chunk { pcad_optim_tensor t; int64_t off; int cnt; };
__device__ __forceinline__ Chunk chunk_of(const pcad_optim_tensor* __restrict__ tab, const int32_t* __restrict__ map) {
    const int64_t c = blockIdx.x;
    Chunk k;
    k.t = tab[map[2 * c]];                                    // block-uniform
    k.off = (int64_t)map[2 * c + 1] * OPTIM_CHUNK;
    const int64_t left = k.t.n - k.off;
    k.cnt = left < OPTIM_CHUNK ? (int)(left < 0 ? 0 : left) : OPTIM_CHUNK;
    return k;
}

template <typename G> __device__ __forceinline__ float sumsq_chunk(const G* __restrict__ g, int cnt, float scale) {
    constexpr int V = Vec<G>::N, PER = OPTIM_CHUNK / (256 * V);
    float acc = 0.f;
    if (cnt == OPTIM_CHUNK) {
        float x[PER][V];
#pragma unroll
        for (int k = 0; k < PER; ++k) loadv<G, V>(g + (int64_t)(threadIdx.x + 256 * k) * V, x[k]);
#pragma unroll
        for (int k = 0; k < PER; ++k)
#pragma unroll
            for (int i = 0; i < V; ++i) { const float s = scale * x[k][i]; acc += s * s; }
        return acc;
    }
#pragma unroll 1
    for (int k = 0; k < PER; ++k) {
        const int at = (threadIdx.x + 256 * k) * V;
        if (at + V <= cnt) {
            float x[V];
            loadv<G, V>(g + at, x);
#pragma unroll
            for (int i = 0; i < V; ++i) { const float s = scale * x[i]; acc += s * s; }
        } else {
            for (int i = at; i < cnt; ++i) { const float s = scale * Elem<G>::load(g + i); acc += s * s; }
        }
    }
    return acc;
}

__global__ __launch_bounds__(256) void optim_sumsq_kernel(const pcad_optim_tensor* __restrict__ tab, const int32_t* __restrict__ map,
                                                          float* __restrict__ part, float grad_scale) {
    __shared__ float lds[4];
    const Chunk k = chunk_of(tab, map);
    float acc;
    if (k.t.grad_dtype == BF16) acc = sumsq_chunk<bf16_t>((const bf16_t*)k.t.grad + k.off, k.cnt, grad_scale);
    else acc = sumsq_chunk<float>((const float*)k.t.grad + k.off, k.cnt, grad_scale);
    acc = block_sum<4>(acc, lds);
    if (threadIdx.x == 0) part[blockIdx.x] = acc;
}

constexpr int FIN_LANES = 1024;

__global__ __launch_bounds__(FIN_LANES) void optim_finalise_kernel(const float* __restrict__ part, int64_t chunks, pcad_optim_state* state,
                                                                   float max_norm, float grad_scale) {
    __shared__ float lds[FIN_LANES / 64];
    float acc = 0.f;
    for (int64_t i = threadIdx.x; i < chunks; i += FIN_LANES) acc += part[i];
    acc = block_sum<FIN_LANES / 64>(acc, lds);
    if (threadIdx.x == 0) {
        const float norm = sqrtf(acc);
        const bool finite = norm - norm == 0.f;               // false for inf and NaN
        float clip = 1.f;
        if (max_norm > 0.f) clip = fminf(1.f, max_norm / (norm + 1e-6f));
        state->norm = norm;
        state->coef = grad_scale * clip;
        state->finite = finite ? 1 : 0;
        state->skipped += finite ? 0 : 1;
    }
}

struct AdamConsts { float decay, b1, omb1, b2, omb2, step_size, bc2_sqrt, eps; };

__device__ __forceinline__ void adam_element(float g, float& p, float& m, float& v, float coef, bool decay, const AdamConsts& a) {
    g *= coef;
    if (decay) p *= a.decay;
    m = a.b1 * m + a.omb1 * g;
    v = a.b2 * v + a.omb2 * (g * g);
    p -= a.step_size * (m / (sqrtf(v) / a.bc2_sqrt + a.eps));
}

// P: the parameter's storage type; G: the gradient's.  bf16 parameters have an fp32 master; an fp32 parameter is its own master unless
// one is given.  V = the elements per 16-byte access of the narrower of the two.
template <typename P, typename G>
__device__ __forceinline__ void update_chunk(const Chunk& k, float coef, const AdamConsts& a) {
    constexpr int V = (sizeof(P) == 2 || sizeof(G) == 2) ? 8 : 4, PER = OPTIM_CHUNK / (256 * V);
    const bool decay = (k.t.flags & PCAD_OPTIM_DECAY) != 0;
    P* __restrict__ param = (P*)k.t.param + k.off;
    const G* __restrict__ grad = (const G*)k.t.grad + k.off;
    const bool own = k.t.master == nullptr;                   // fp32 parameter without a master (the plan refuses a bf16 one)
    float* __restrict__ master = own ? (float*)param : k.t.master + k.off;
    float* __restrict__ ea = k.t.exp_avg + k.off;
    float* __restrict__ es = k.t.exp_avg_sq + k.off;
    if (k.cnt == OPTIM_CHUNK) {
        float g[PER][V], p[PER][V], m[PER][V], v[PER][V];
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int at = (threadIdx.x + 256 * j) * V;
            loadv<G, V>(grad + at, g[j]);
            loadv<float, V>(master + at, p[j]);
            loadv<float, V>(ea + at, m[j]);
            loadv<float, V>(es + at, v[j]);
        }
#pragma unroll
        for (int j = 0; j < PER; ++j) {
            const int at = (threadIdx.x + 256 * j) * V;
#pragma unroll
            for (int i = 0; i < V; ++i) adam_element(g[j][i], p[j][i], m[j][i], v[j][i], coef, decay, a);
            storev<float, V>(master + at, p[j]);
            storev<float, V>(ea + at, m[j]);
            storev<float, V>(es + at, v[j]);
            if constexpr (sizeof(P) == 2) storev<P, V>(param + at, p[j]);
            else if (!own) storev<P, V>(param + at, p[j]);
        }
        return;
    }
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int at = (threadIdx.x + 256 * j) * V;
        if (at + V <= k.cnt) {
            float g[V], p[V], m[V], v[V];
            loadv<G, V>(grad + at, g);
            loadv<float, V>(master + at, p);
            loadv<float, V>(ea + at, m);
            loadv<float, V>(es + at, v);
#pragma unroll
            for (int i = 0; i < V; ++i) adam_element(g[i], p[i], m[i], v[i], coef, decay, a);
            storev<float, V>(master + at, p);
            storev<float, V>(ea + at, m);
            storev<float, V>(es + at, v);
            if constexpr (sizeof(P) == 2) storev<P, V>(param + at, p);
            else if (!own) storev<P, V>(param + at, p);
        } else {
            for (int i = at; i < k.cnt; ++i) {                // the tensor's last n % V elements, one by one
                float p = master[i], m = ea[i], v = es[i];
                adam_element(Elem<G>::load(grad + i), p, m, v, coef, decay, a);
                master[i] = p;
                ea[i] = m;
                es[i] = v;
                if (sizeof(P) == 2 || !own) Elem<P>::store(param + i, p);
            }
        }
    }
}

__global__ __launch_bounds__(256) void optim_update_kernel(const pcad_optim_tensor* __restrict__ tab, const int32_t* __restrict__ map,
                                                           const pcad_optim_state* __restrict__ state, AdamConsts a) {
    if (state->finite == 0) return;                           // a skipped step changes nothing at all
    const float coef = state->coef;
    const Chunk k = chunk_of(tab, map);
    const bool pb = k.t.param_dtype == BF16, gb = k.t.grad_dtype == BF16;
    if (pb && gb) update_chunk<bf16_t, bf16_t>(k, coef, a);
    else if (pb) update_chunk<bf16_t, float>(k, coef, a);
    else if (gb) update_chunk<float, bf16_t>(k, coef, a);
    else update_chunk<float, float>(k, coef, a);
}

template <typename G> __device__ __forceinline__ void zero_chunk(G* __restrict__ g, int cnt) {
    constexpr int V = Vec<G>::N, PER = OPTIM_CHUNK / (256 * V);
    const float z[V] = {};
#pragma unroll
    for (int j = 0; j < PER; ++j) {
        const int at = (threadIdx.x + 256 * j) * V;
        if (at + V <= cnt) storev<G, V>(g + at, z);
        else
            for (int i = at; i < cnt; ++i) g[i] = (G)0;
    }
}

__global__ __launch_bounds__(256) void optim_zero_grads_kernel(const pcad_optim_tensor* __restrict__ tab, const int32_t* __restrict__ map) {
    const Chunk k = chunk_of(tab, map);
    if (k.t.grad_dtype == BF16) zero_chunk<bf16_t>((bf16_t*)k.t.grad + k.off, k.cnt);
    else zero_chunk<float>((float*)k.t.grad + k.off, k.cnt);
}

// pcad_grads_gather: chunk c of tensor t, widened to fp32, into its slice of one flat buffer.  A full chunk's loads are
// all issued before its stores, as in update_chunk; bf16 -> fp32 is a shift, so the copy is exact.  A slice starts at a multiple of 4
// elements of a 16-byte aligned buffer and a chunk at a multiple of OPTIM_CHUNK within it, so every vector store is 16-byte aligned.
template <typename G> __device__ __forceinline__ void gather_chunk(const G* __restrict__ g, float* __restrict__ out, int cnt) {
    constexpr int V = Vec<G>::N, PER = OPTIM_CHUNK / (256 * V);
    if (cnt == OPTIM_CHUNK) {
        float x[PER][V];
#pragma unroll
        for (int j = 0; j < PER; ++j) loadv<G, V>(g + (threadIdx.x + 256 * j) * V, x[j]);
#pragma unroll
        for (int j = 0; j < PER; ++j) storev<float, V>(out + (threadIdx.x + 256 * j) * V, x[j]);
        return;
    }
#pragma unroll 1
    for (int j = 0; j < PER; ++j) {
        const int at = (threadIdx.x + 256 * j) * V;
        if (at + V <= cnt) {
            float x[V];
            loadv<G, V>(g + at, x);
            storev<float, V>(out + at, x);
        } else {
            for (int i = at; i < cnt; ++i) out[i] = Elem<G>::load(g + i);      // the tensor's last n % V elements; the slice's padding stays
        }
    }
}

__global__ __launch_bounds__(256) void optim_grads_gather_kernel(const pcad_optim_tensor* __restrict__ tab, const int32_t* __restrict__ map,
                                                                 const int64_t* __restrict__ offsets, float* __restrict__ flat,
                                                                 int64_t flat_elems) {
    const Chunk k = chunk_of(tab, map);
    const int64_t at = offsets[map[2 * (int64_t)blockIdx.x]] + k.off;
    if (at < 0 || (at & 3) || at + k.cnt > flat_elems) return;     // offsets that are not pcad_grads_flat_plan's for this buffer: nothing is written
    float* out = flat + at;
    if (k.t.grad_dtype == BF16) gather_chunk<bf16_t>((const bf16_t*)k.t.grad + k.off, out, k.cnt);
    else gather_chunk<float>((const float*)k.t.grad + k.off, out, k.cnt);
}

}  // namespace

hipError_t launch_adamw_step(const AdamwLaunch& a, hipStream_t s) {
    if (a.chunks < 0 || a.chunks > PCAD_OPTIM_MAX_CHUNKS || !a.state) return hipErrorInvalidValue;
    if (a.chunks > 0 && (!a.table || !a.map || !a.part)) return hipErrorInvalidValue;
    const auto* tab = (const pcad_optim_tensor*)a.table;
    auto* state = (pcad_optim_state*)a.state;
    const dim3 grid((unsigned)a.chunks), block(256);
    if (a.chunks > 0) {
        hipLaunchKernelGGL(optim_sumsq_kernel, grid, block, 0, s, tab, a.map, a.part, a.grad_scale);
        if (hipError_t e = hipGetLastError()) return e;
    }
    hipLaunchKernelGGL(optim_finalise_kernel, dim3(1), dim3(FIN_LANES), 0, s, (const float*)a.part, a.chunks, state, a.max_norm, a.grad_scale);
    if (hipError_t e = hipGetLastError()) return e;
    if (a.chunks > 0) {
        const AdamConsts k = {a.decay, a.b1, a.omb1, a.b2, a.omb2, a.step_size, a.bc2_sqrt, a.eps};
        hipLaunchKernelGGL(optim_update_kernel, grid, block, 0, s, tab, a.map, (const pcad_optim_state*)state, k);
        if (hipError_t e = hipGetLastError()) return e;
    }
    return hipSuccess;
}

hipError_t launch_zero_grads(const void* table, const int32_t* map, int64_t chunks, hipStream_t s) {
    if (chunks < 0 || chunks > PCAD_OPTIM_MAX_CHUNKS) return hipErrorInvalidValue;
    if (chunks == 0) return hipSuccess;
    if (!table || !map) return hipErrorInvalidValue;
    hipLaunchKernelGGL(optim_zero_grads_kernel, dim3((unsigned)chunks), dim3(256), 0, s, (const pcad_optim_tensor*)table, map);
    return hipGetLastError();
}

hipError_t launch_grads_gather(const void* table, const int32_t* map, int64_t chunks, const int64_t* offsets, float* flat, int64_t flat_elems,
                               hipStream_t s) {
    if (chunks < 0 || chunks > PCAD_OPTIM_MAX_CHUNKS) return hipErrorInvalidValue;
    if (chunks == 0) return hipSuccess;
    if (!table || !map || !offsets || !flat) return hipErrorInvalidValue;
    hipLaunchKernelGGL(optim_grads_gather_kernel, dim3((unsigned)chunks), dim3(256), 0, s, (const pcad_optim_tensor*)table, map, offsets, flat,
                       flat_elems);
    return hipGetLastError();
}

}  // namespace pcad
