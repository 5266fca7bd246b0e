// Backward of the pooled sequence-classification head (include/pcad_bwd.h pcad_pooled_head_bwd, libpcad_bwd.so): norm_f ->
// per-strand pooling (mean / first / last) -> score -> (fwd + rc) / 2, the forward of pool.hip, on plain rows.
//
// Per window b (both strands s get the same cotangent, because the logits average the two strands' scores), everything in fp32:
//   dpooled[b, :]  = 1/2 sum_n dlogits[b, n] W[n, :]                                       (n in index order)
//   dscore_w[n, :] = 1/2 sum_b dlogits[b, n] (pooled[b, 0, :] + pooled[b, 1, :])           (b in index order; pooled: the forward's pooled_out)
//   do(row)        = dpooled[b] / L on every row of the strand (mean);  dpooled[b] on row 0 (first) / row L-1 (last), 0 on the others
//   v = h + res    rstd = rsqrt(mean(v^2) + eps)    vh = v rstd                            (per row, as pool_stage1_kernel forms them)
//   dv_i = rstd (w_i do_i - vh_i (1/D) sum_j w_j do_j vh_j)        dh = round_T(dv)    dres = round_RT(dv)
//   dnorm_weight_i = sum_rows do_i vh_i
// The forward's roundings (o, the mean, the strands' scores, their sum, the half) are the identity in the derivative; the only new
// roundings are the stores of dh and dres.  With first / last the rows that carry no gradient are written as zeros, without reading h.
//
// Two launches and launch_sum_partials:
//   prep  one block per window forms its do row ONCE (dlogits in LDS, the 256 lanes own the columns lane + 256 m) into the caller's
//         scratch, and one block per label forms its row of dscore_w: no row of the walk below ever touches score_w.
//   rows  pool_stage1_kernel's shape: one block per (window, strand, POOL_BWD_SEG-row segment), 4 waves, one row per wave at a time with
//         16-byte accesses; a wave keeps do and w do of its window in registers (both are the same for all of its rows), walks the rows
//         t0 + wave, t0 + wave + 4, ... and adds do vh into a register partial; the waves' partials are added in wave order through
//         LDS and the block stores one partial row, which launch_sum_partials adds in a fixed order.  Every row of dh / dres is owned by
//         exactly one wave of one block.  The segmentation depends on L only, so a window's rows do not depend on its batch.
//         first / last with neither dh nor dres asked for: only the segment that holds the pooled row is launched.
// No floating-point atomics.  All in-tensor offsets are 64-bit.
#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

namespace {
int phb_segments(int L) { return (L + POOL_BWD_SEG - 1) / POOL_BWD_SEG; }
// partial rows per (window, strand): mean - one per segment; first / last - the one segment that holds the pooled row
int phb_partials(int L, int pooling) { return pooling == POOL_MEAN ? phb_segments(L) : 1; }
size_t phb_round256(size_t n) { return (n + 255) / 256 * 256; }
size_t phb_drow_bytes(int B, int D) { return phb_round256((size_t)B * (size_t)D * sizeof(float)); }
}  // namespace

// the windows' do rows [B, D], then one partial row [D] of dnorm_weight per (window, strand, segment that carries a gradient)
size_t pooled_head_bwd_bytes(int B, int L, int D, int pooling) {
    return phb_drow_bytes(B, D) + phb_round256((size_t)B * 2 * (size_t)phb_partials(L, pooling) * (size_t)D * sizeof(float));
}

// blocks [0, nwin): the do row of window blockIdx.x;  blocks [nwin, nwin + NL) (dscore_w given): row blockIdx.x - nwin of dscore_w
__global__ __launch_bounds__(256) void pool_bwd_prep_kernel(const float* __restrict__ dlogits, const float* __restrict__ score_w,
                                                            const float* __restrict__ pooled, float* __restrict__ drow,
                                                            float* __restrict__ dscore_w, int B, int L, int D, int NL, int pooling, int nwin) {
    if ((int)blockIdx.x < nwin) {
        __shared__ float dl[256];
        const int b = blockIdx.x;
        if ((int)threadIdx.x < NL) dl[threadIdx.x] = dlogits[(int64_t)b * NL + threadIdx.x];
        __syncthreads();
        for (int col = threadIdx.x; col < D; col += 256) {
            float a = 0.f;
            for (int n = 0; n < NL; ++n) a += dl[n] * score_w[(int64_t)n * D + col];      // label order: deterministic
            a *= 0.5f;
            drow[(int64_t)b * D + col] = pooling == POOL_MEAN ? a / (float)L : a;
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

template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(256) void pool_bwd_rows_kernel(const T* __restrict__ h, const RT* __restrict__ res, const float* __restrict__ w,
                                                            const float* __restrict__ drow, T* __restrict__ dh, RT* __restrict__ dres,
                                                            float* __restrict__ part, int B, int L, int D, float eps, int pooling, int nseg, int g0) {
    __shared__ float red[3][2048];       // waves 1..3 hand their dnorm_weight partials to wave 0
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int g = g0 + blockIdx.x % nseg;   // nseg: the segments per strand this launch covers, from segment g0 on
    const int sb = blockIdx.x / nseg;    // window * 2 + strand
    const int b = sb >> 1, s = sb & 1;
    const int t0 = g * POOL_BWD_SEG, t1 = min(L, t0 + POOL_BWD_SEG);
    const bool mean = pooling == POOL_MEAN;
    const int tp = pooling == POOL_FIRST ? 0 : L - 1;                  // first / last: the one row that carries a gradient
    const bool carries = mean || (tp >= t0 && tp < t1);                // the same decision in every wave of the block
    const int64_t row0 = (int64_t)(s == 0 ? b : B + b) * L;           // each strand is pooled over its own rows: no flip
    const int nchunk = D >> 3;
    const float inv_d = 1.0f / (float)D;
    const bool rows_out = dh != nullptr || dres != nullptr;

    float dO[MAXC][8], gw[MAXC][8], acc[MAXC][8];                      // do, w do, sum over the wave's rows of do vh
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
#pragma unroll
        for (int i = 0; i < 8; ++i) { dO[j][i] = 0.f; gw[j][i] = 0.f; acc[j][i] = 0.f; }
        if (carries && c < nchunk) {
            float wn[8];
            load8<float>(w + c * 8, wn);
            load8<float>(drow + (int64_t)b * D + c * 8, dO[j]);
#pragma unroll
            for (int i = 0; i < 8; ++i) gw[j][i] = wn[i] * dO[j][i];
        }
    }

    for (int t = t0 + wv; t < t1; t += 4) {
        const int64_t row = row0 + t;
        if (!mean && t != tp) {
            // a row the pooling did not read: no gradient
            const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int j = 0; j < MAXC; ++j) {
                const int c = lane + 64 * j;
                if (c < nchunk) {
                    if (dh != nullptr) store8<T>(dh + row * D + c * 8, z);
                    if (dres != nullptr) store8<RT>(dres + row * D + c * 8, z);
                }
            }
            continue;
        }
        float v[MAXC][8];
        float ss = 0.f;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
                float r[8];
                load8<T>(h + row * D + c * 8, v[j]);
                load8<RT>(res + row * D + c * 8, r);
#pragma unroll
                for (int i = 0; i < 8; ++i) { v[j][i] += r[i]; ss += v[j][i] * v[j][i]; }
            }
        }
        ss = wave_sum(ss);
        const float rstd = rsqrtf(ss / (float)D + eps);               // pool_stage1_kernel's expression
        float dot = 0.f;                                              // sum_j w_j do_j vh_j
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
#pragma unroll
                for (int i = 0; i < 8; ++i) {
                    v[j][i] *= rstd;                                  // vh
                    acc[j][i] += dO[j][i] * v[j][i];
                    dot += gw[j][i] * v[j][i];
                }
            }
        }
        if (!rows_out) continue;
        dot = wave_sum(dot) * inv_d;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (c < nchunk) {
                float dv[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) dv[i] = rstd * (gw[j][i] - v[j][i] * dot);
                if (dh != nullptr) store8<T>(dh + row * D + c * 8, dv);
                if (dres != nullptr) store8<RT>(dres + row * D + c * 8, dv);
            }
        }
    }
    if (part == nullptr || !carries) return;                          // block-uniform: no wave waits at the barrier below
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
    float* const prow = part + ((int64_t)sb * (mean ? nseg : 1) + (mean ? g : 0)) * D;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
#pragma unroll
            for (int k = 0; k < 3; ++k)      // wave order: a fixed summation order
#pragma unroll
                for (int i = 0; i < 8; ++i) acc[j][i] += red[k][c * 8 + i];
            store8<float>(prow + c * 8, acc[j]);
        }
    }
}

hipError_t launch_pooled_head_bwd(const PooledHeadBwdLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (in.res_frag || in.D <= 0 || in.L <= 0 || a.NL < 1 || a.NL > 256) return hipErrorInvalidValue;
    if (a.pooling != POOL_MEAN && a.pooling != POOL_FIRST && a.pooling != POOL_LAST) return hipErrorInvalidValue;
    if (!a.dlogits || (!a.dh && !a.dres && !a.dnorm_w && !a.dscore_w)) return hipErrorInvalidValue;
    const bool rows = a.dh != nullptr || a.dres != nullptr || a.dnorm_w != nullptr;
    if (rows && (!in.h || !in.res || !in.w || !a.score_w || !a.scratch)) return hipErrorInvalidValue;
    if (a.dscore_w && !a.pooled) return hipErrorInvalidValue;
    if (in.B <= 0) return hipSuccess;
    // first / last with neither dh nor dres: only the segment that holds the pooled row has anything to do (dnorm_weight's partial)
    const bool one_segment = a.pooling != POOL_MEAN && !a.dh && !a.dres;
    const int nseg = one_segment ? 1 : phb_segments(in.L);
    const int g0 = one_segment && a.pooling == POOL_LAST ? (in.L - 1) / POOL_BWD_SEG : 0;
    const int64_t blocks = (int64_t)in.B * 2 * nseg;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    float* const drow = (float*)a.scratch;
    float* const part = a.dnorm_w ? (float*)((char*)a.scratch + phb_drow_bytes(in.B, in.D)) : nullptr;
    const int nwin = rows ? in.B : 0;
    hipLaunchKernelGGL(pool_bwd_prep_kernel, dim3((unsigned)(nwin + (a.dscore_w ? a.NL : 0))), dim3(256), 0, s, a.dlogits, a.score_w, a.pooled, drow,
                       a.dscore_w, in.B, in.L, in.D, a.NL, a.pooling, nwin);
    if (hipError_t e = hipGetLastError()) return e;
    if (!rows) return hipSuccess;
    hipError_t err = select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        hipLaunchKernelGGL((pool_bwd_rows_kernel<T, RT, decltype(form)::MAXC>), dim3((unsigned)blocks), dim3(256), 0, s, (const T*)in.h, (const RT*)in.res,
                           in.w, (const float*)drow, (T*)a.dh, (RT*)a.dres, part, in.B, in.L, in.D, in.eps, a.pooling, nseg, g0);
        return hipGetLastError();
    });
    if (err != hipSuccess || !a.dnorm_w) return err;
    return launch_sum_partials(part, (int64_t)in.B * 2 * phb_partials(in.L, a.pooling), a.dnorm_w, in.D, nullptr, 0, s);
}

}  // namespace pcad
