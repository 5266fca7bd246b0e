// The score head on cached pooled vectors, forward and backward (include/pcad_bwd.h pcad_pooled_logits / pcad_pooled_logits_bwd,
// libpcad_bwd.so): what is left of the pooled sequence-classification head when the trunk is frozen and a window's
// pooled vectors [2, D] - pool.hip's pooled_out - are computed once and kept.
//
//   logits[b, n]    = round_T(round_T(round_T(pooled[b, 0] . W[n]) + round_T(pooled[b, 1] . W[n])) * 0.5)
//   dscore_w[n, :]  = 1/2 sum_b dlogits[b, n] (pooled[b, 0, :] + pooled[b, 1, :])           (b in index order)
//   dpooled[b, s,:] = 1/2 sum_n dlogits[b, n] W[n, :]                                       (n in index order; the same for both strands)
//
// The forward RESTATES the logits half of pool.hip's pool_stage2_kernel - the same block shape, the same lane and wave order, the same
// expressions - because libpcad.so's exports are closed: logits from cached vectors are the bits pcad_forward_pooled would have written.
// The backward restates pool_bwd.hip's pool_bwd_prep_kernel: its label branch operation for operation (dscore_w is pcad_pooled_head_bwd's
// bit for bit), and its window branch without the / L of the mean, because the pooling lies upstream of `pooled`.  The forward's
// roundings are the identity in the derivative.  No floating-point atomics; all in-tensor offsets are 64-bit.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

// one block per window: its 2 D pooled values in LDS, then pool_stage2_kernel's product - wave wv takes labels wv, wv + 4, ...
template <typename T>
__global__ __launch_bounds__(256) void pooled_logits_kernel(const float* __restrict__ pooled, const float* __restrict__ score_w,
                                                            float* __restrict__ logits_out, int D, int NL) {
    __shared__ float pv[2 * 2048];
    const int b = blockIdx.x;
    for (int idx = threadIdx.x; idx < 2 * D; idx += 256) pv[idx] = pooled[(int64_t)b * 2 * D + idx];
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

// blocks [0, nwin): dpooled of window blockIdx.x, both strands;  blocks [nwin, nwin + NL) (dscore_w given): row blockIdx.x - nwin of dscore_w
__global__ __launch_bounds__(256) void pooled_logits_bwd_kernel(const float* __restrict__ dlogits, const float* __restrict__ score_w,
                                                                const float* __restrict__ pooled, float* __restrict__ dpooled,
                                                                float* __restrict__ dscore_w, int B, int D, int NL, int nwin) {
    if ((int)blockIdx.x < nwin) {
        __shared__ float dl[256];
        const int b = blockIdx.x;
        if ((int)threadIdx.x < NL) dl[threadIdx.x] = dlogits[(int64_t)b * NL + threadIdx.x];
        __syncthreads();
        for (int col = threadIdx.x; col < D; col += 256) {
            float a = 0.f;
            for (int n = 0; n < NL; ++n) a += dl[n] * score_w[(int64_t)n * D + col];      // label order: deterministic
            a *= 0.5f;
            dpooled[(int64_t)(2 * b) * D + col] = a;
            dpooled[(int64_t)(2 * b + 1) * D + col] = a;
        }
    } else {
        const int n = (int)blockIdx.x - nwin;
        for (int col = threadIdx.x; col < D; col += 256) {
            float a = 0.f;
            for (int b = 0; b < B; ++b)                                                    // window order: deterministic
                a += dlogits[(int64_t)b * NL + n] * (pooled[(int64_t)(2 * b) * D + col] + pooled[(int64_t)(2 * b + 1) * D + col]);
            dscore_w[(int64_t)n * D + col] = 0.5f * a;
        }
    }
}

hipError_t launch_pooled_logits(const PooledLogitsLaunch& a, hipStream_t s) {
    if (!a.pooled || !a.score_w || !a.logits) return hipErrorInvalidValue;
    if (a.D <= 0 || a.D % 8 || a.D > 2048 || a.NL < 1 || a.NL > 256 || a.B < 0) return hipErrorInvalidValue;
    if (a.dt != BF16 && a.dt != F32) return hipErrorInvalidValue;
    if (a.B == 0) return hipSuccess;
    if (a.dt == BF16)
        hipLaunchKernelGGL(pooled_logits_kernel<bf16_t>, dim3((unsigned)a.B), dim3(256), 0, s, a.pooled, a.score_w, a.logits, a.D, a.NL);
    else
        hipLaunchKernelGGL(pooled_logits_kernel<float>, dim3((unsigned)a.B), dim3(256), 0, s, a.pooled, a.score_w, a.logits, a.D, a.NL);
    return hipGetLastError();
}

hipError_t launch_pooled_logits_bwd(const PooledLogitsBwdLaunch& a, hipStream_t s) {
    if (!a.dlogits || (!a.dscore_w && !a.dpooled)) return hipErrorInvalidValue;
    if ((a.dscore_w && !a.pooled) || (a.dpooled && !a.score_w)) return hipErrorInvalidValue;
    if (a.D <= 0 || a.D % 8 || a.D > 2048 || a.NL < 1 || a.NL > 256 || a.B < 0) return hipErrorInvalidValue;
    if (a.B == 0) return hipSuccess;
    const int nwin = a.dpooled ? a.B : 0;
    hipLaunchKernelGGL(pooled_logits_bwd_kernel, dim3((unsigned)(nwin + (a.dscore_w ? a.NL : 0))), dim3(256), 0, s, a.dlogits, a.score_w,
                       a.pooled, a.dpooled, a.dscore_w, a.B, a.D, a.NL, nwin);
    return hipGetLastError();
}

}  // namespace pcad
