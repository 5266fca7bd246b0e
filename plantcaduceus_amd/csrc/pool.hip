// Pooled sequence-classification head (CaduceusForSequenceClassification, RCPS model).
//
//   hs[b, p, :, 0] = norm_f(h + res) of the forward strand's row p, hs[b, p, :, 1] = the same of the rc strand's own row p
//   (flip(H[..., D:], dims=[1, 2]) of the reference's stacked hidden state is simply the rc strand's row in the 2B-strand batch),
//   each rounded to the model dtype;  pooled[b, :, s] = mean / max / row 0 / row L-1 over p;
//   logits[b] = round(round(round(score(pooled[b, :, 0])) + round(score(pooled[b, :, 1]))) / 2)   (score: Linear(D, NL, bias=False)).
//
// Two launches, never a [B, L, 2D] tensor in memory:
//   stage 1  one block per (window, strand, 64-row segment): 4 waves walk the segment's rows (one row per wave at a time, like
//            final_head_kernel), norm_f each row and accumulate its rounded values per channel (fp32 sum, or max); the waves'
//            accumulators are combined in wave order and the block writes one partial row [D] fp32.
//   stage 2  one block per window: the segments' partials are reduced in segment order (mean: / L, rounded once), the two pooled
//            vectors are kept in LDS and 4 waves run the [2, D] x [NL, D]^T product (fp32 accumulation, a fixed lane order).
// The segmentation depends on L only, so a window's logits do not depend on the batch or chunk it runs in.
#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int POOL_SEG = 64;      // rows per stage-1 segment
constexpr int POOL_STATUS_BAD_TOKEN_BIT = 1;     // = pcad.h PCAD_STATUS_BAD_TOKEN

int pool_segments(int L, int pooling) {
    return (pooling == POOL_MEAN || pooling == POOL_MAX) ? (L + POOL_SEG - 1) / POOL_SEG : 1;
}

size_t pool_partial_bytes(int B, int L, int D, int pooling) {
    return (size_t)B * 2 * (size_t)pool_segments(L, pooling) * (size_t)D * 4;
}

// max that keeps a NaN (torch.max propagates it)
__device__ __forceinline__ float max_nan(float a, float x) { return (x > a || x != x) ? x : a; }

template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(256) void pool_stage1_kernel(const T* __restrict__ h, const RT* __restrict__ res,
                                                          const float* __restrict__ w, float* __restrict__ part, int B, int L,
                                                          int D, float eps, int pooling, int nseg, const int32_t* __restrict__ ids,
                                                          int32_t* __restrict__ status, int res_frag) {
    __shared__ float red[3][2048];       // waves 1..3 hand their accumulators to wave 0
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int g = blockIdx.x % nseg;
    const int sb = blockIdx.x / nseg;    // window * 2 + strand
    const int b = sb >> 1, s = sb & 1;
    // input validation as final_head_kernel does it: the first block of every window scans its ids (the embedding gather aliased
    // an id outside the vocabulary to id & 7) and sets a bit of the caller's status word
    if (status != nullptr && ids != nullptr && g == 0 && s == 0) {
        bool bad = false;
        for (int t = threadIdx.x; t < L; t += 256) bad |= (unsigned)ids[(int64_t)b * L + t] > 7u;
        if (__any(bad) && lane == 0) atomicOr(status, POOL_STATUS_BAD_TOKEN_BIT);
    }
    int t0, t1;
    if (pooling == POOL_FIRST) { t0 = 0; t1 = 1; }
    else if (pooling == POOL_LAST) { t0 = L - 1; t1 = L; }
    else { t0 = g * POOL_SEG; t1 = min(L, t0 + POOL_SEG); }
    const bool is_max = pooling == POOL_MAX;
    const int nchunk = D >> 3;
    float acc[MAXC][8], wn[MAXC][8];
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
#pragma unroll
        for (int i = 0; i < 8; ++i) { acc[j][i] = is_max ? -INFINITY : 0.f; wn[j][i] = 0.f; }
        if (c < nchunk) load8<float>(w + c * 8, wn[j]);
    }
    for (int t = t0 + wv; t < t1; t += 4) {
        const int64_t row = (int64_t)(s == 0 ? b : B + b) * L + t;
        float v[MAXC][8];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
                float r[8];
                load8<T>(h + row * D + c * 8, v[j]);
                if (res_frag) {              // norm-folded form: fp32 residual in the GEMM's fragment layout (RT == float)
                    const float* rp = reinterpret_cast<const float*>(res) + res_frag_off(row, c * 8, res_frag);
                    const f32x4 a = *reinterpret_cast<const f32x4*>(rp), q = *reinterpret_cast<const f32x4*>(rp + 256);
                    r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; r[4] = q[0]; r[5] = q[1]; r[6] = q[2]; r[7] = q[3];
                } else {
                    load8<RT>(res + row * D + c * 8, r);
                }
#pragma unroll
                for (int i = 0; i < 8; ++i) { v[j][i] += r[i]; ss += v[j][i] * v[j][i]; }
            }
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)D + eps);
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    const float o = Elem<T>::round(v[j][i] * rstd * wn[j][i]);      // hidden_states[-1] in the model dtype
                    acc[j][i] = is_max ? max_nan(acc[j][i], o) : acc[j][i] + o;
                }
            }
        }
    }
    if (wv > 0) {
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk)
#pragma unroll
                for (int i = 0; i < 8; ++i) red[wv - 1][c * 8 + i] = acc[j][i];
        }
    }
    __syncthreads();
    if (wv != 0) return;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
#pragma unroll
            for (int k = 0; k < 3; ++k)      // wave order: a fixed summation order
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[j][i] = is_max ? max_nan(acc[j][i], red[k][c * 8 + i]) : acc[j][i] + red[k][c * 8 + i];
            store8<float>(part + ((int64_t)sb * nseg + g) * D + c * 8, acc[j]);
        }
    }
}

template <typename T>
__global__ __launch_bounds__(256) void pool_stage2_kernel(const float* __restrict__ part, const float* __restrict__ score_w,
                                                          float* __restrict__ pooled_out, float* __restrict__ logits_out, int L,
                                                          int D, int NL, int pooling, int nseg) {
    __shared__ float pv[2 * 2048];
    const int b = blockIdx.x;
    const bool is_max = pooling == POOL_MAX;
    for (int idx = threadIdx.x; idx < 2 * D; idx += 256) {
        const int s = idx >= D ? 1 : 0, c = idx - s * D;
        const float* p = part + ((int64_t)(2 * b + s) * nseg) * D + c;
        float a = p[0];
        for (int g = 1; g < nseg; ++g) {     // segment order: deterministic
            const float x = p[(int64_t)g * D];
            a = is_max ? max_nan(a, x) : a + x;
        }
        if (pooling == POOL_MEAN) a = Elem<T>::round(a / (float)L);       // fp32 accumulation, rounded once to the model dtype
        pv[idx] = a;
        if (pooled_out != nullptr) pooled_out[(int64_t)b * 2 * D + idx] = a;
    }
    if (logits_out == nullptr) return;
    __syncthreads();
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    for (int n = wv; n < NL; n += 4) {
        const float* wr = score_w + (int64_t)n * D;
        float a0 = 0.f, a1 = 0.f;
        for (int c = lane; c < D; c += 64) {
            const float x = wr[c];
            a0 += pv[c] * x;
            a1 += pv[D + c] * x;
        }
        a0 = Elem<T>::round(wave_sum(a0));       // score(pooled[..., 0]) in the model dtype
        a1 = Elem<T>::round(wave_sum(a1));
        if (lane == 0) logits_out[(int64_t)b * NL + n] = Elem<T>::round(Elem<T>::round(a0 + a1) * 0.5f);
    }
}

hipError_t launch_pooled_head(const PooledHeadLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (in.L <= 0 || a.pooling < POOL_MEAN || a.pooling > POOL_LAST) return hipErrorInvalidValue;
    if (a.logits_out != nullptr && (a.score_w == nullptr || a.NL < 1 || a.NL > 256)) return hipErrorInvalidValue;
    if (in.B <= 0) return hipSuccess;
    const int nseg = pool_segments(in.L, a.pooling);
    return select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        hipLaunchKernelGGL((pool_stage1_kernel<T, RT, decltype(form)::MAXC>), dim3((unsigned)((int64_t)in.B * 2 * nseg)), dim3(256), 0, s, (const T*)in.h,
                           (const RT*)in.res, in.w, (float*)a.part, in.B, in.L, in.D, in.eps, a.pooling, nseg, in.ids, in.status, in.res_frag);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL((pool_stage2_kernel<T>), dim3((unsigned)in.B), dim3(256), 0, s, (const float*)a.part, a.score_w, a.pooled_out, a.logits_out, in.L,
                           in.D, a.NL, a.pooling, nseg);
        return hipGetLastError();
    });
}

}  // namespace pcad
