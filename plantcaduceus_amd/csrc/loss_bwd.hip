// Backward of the masked-LM loss head (include/pcad_bwd.h pcad_loss_head_bwd, libpcad_bwd.so): norm_f -> RC
// re-assembly -> tied RCPS LM head -> weighted cross entropy, differentiated at the labelled positions only.
//
// Per labelled position (b, t), rows rf = (b, t) and rr = (B + b, L-1-t), everything in fp32:
//   v = h + res    rstd = rsqrt(mean(v^2) + eps)    vh = v rstd    o = round_T(vh w)              (head_row: the forward's own row code)
//   lg = the forward's logits (bit for bit: the same head_row arithmetic)    p = softmax(lg)
//   dlg[k] = (dsum[b] wt + dnll[b, t]) (p[k] - [k == label])
//   do_i = sum_k dlg[k] Emb[k][i] (rf) / sum_k dlg[k] Emb[comp[k]][i] (rr)
//   dv_i = rstd (w_i do_i - vh_i (1/D) sum_j w_j do_j vh_j)        dh = round_T(dv)    dres = round_RT(dv)
//   demb[k] += dlg[k] o (rf)    demb[comp[k]] += dlg[k] o (rr)      dnorm_weight_i += do_i vh_i
// The forward's roundings (o, the strands' partial logits, their sum) are the identity in the derivative; the only new roundings
// are the stores of dh and dres.  Rows of unlabelled positions are written as zeros.
//
// Shape (loss.hip's): one block per (window, LOSS_SEG-position segment); the 4 waves take positions t0 + 4 i + wave in rounds
// i = 0, 1, ... and each runs BOTH strands' rows of its position, so every row of dh / dres is owned by exactly one wave of one block.
// Parameter partials: in a round, each wave leaves o and do vh of its two rows (fp32) and the 8 cotangents per row in LDS; after a
// barrier the block's 256 lanes each own the columns lane + 256 m and add the round's rows into 9 register accumulators per column
// (demb[0..7], dnorm_weight) in position order, forward strand before rc strand.  A round without a labelled position has no
// barrier.  The block stores one row of 9 D partials (demb | dnorm_weight) to the caller's scratch and launch_sum_partials adds the
// blocks' rows in a fixed order.  No floating-point atomics.  All in-tensor offsets are 64-bit.
#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

namespace {
constexpr int LHB_SLOTS = 8;        // rows staged per round: 4 waves x 2 strands
int lhb_segments(int L) { return (L + LOSS_SEG - 1) / LOSS_SEG; }
// staged rows of o and of do vh, then the rows' 8 cotangents
size_t lhb_lds_bytes(int D) { return ((size_t)2 * LHB_SLOTS * D + LHB_SLOTS * 8) * sizeof(float); }
}  // namespace

// one row of 9 D partials per block, and one more row that takes the sum of whichever of demb / dnorm_weight the caller did not ask for
size_t loss_head_bwd_bytes(int B, int L, int D) {
    return (((size_t)B * (size_t)lhb_segments(L) + 1) * 9 * (size_t)D * sizeof(float) + 255) / 256 * 256;
}

// One strand's row of a labelled position: dh / dres of the row, and (STAGE) its o, do vh and cotangents into the wave's LDS slot.
// v, rstd: head_row's, as a HeadRowKept holds them.  dl[k]: the cotangent of logit k.
template <typename T, typename RT, int MAXC>
__device__ __forceinline__ void lhb_row(float (&v)[MAXC][8], float rstd, int64_t row, int strand, const float (&dl)[8],
                                        const float* __restrict__ w, const float* __restrict__ emb, const int32_t* __restrict__ comp8,
                                        T* __restrict__ dh, RT* __restrict__ dres, float* __restrict__ so, float* __restrict__ sq,
                                        int D, int lane) {
    const int nchunk = D >> 3;
    const float inv_d = 1.0f / (float)D;
    float g[MAXC][8];               // w do
    float dot = 0.f;                // sum_j w_j do_j vh_j
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            float wv[8], dO[8], o[8], q[8];
            load8<float>(w + c * 8, wv);
#pragma unroll
            for (int i = 0; i < 8; ++i) dO[i] = 0.f;
#pragma unroll
            for (int k = 0; k < 8; ++k) {
                const int er = strand == 0 ? k : (comp8[k] & 7);
                float e[8];
                load8<float>(emb + (int64_t)er * D + c * 8, e);
#pragma unroll
                for (int i = 0; i < 8; ++i) dO[i] += dl[k] * e[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) {
                v[j][i] *= rstd;                                    // vh
                o[i] = Elem<T>::round(v[j][i] * wv[i]);             // the forward's o: (v rstd) w, rounded to the model dtype
                q[i] = dO[i] * v[j][i];
                g[j][i] = wv[i] * dO[i];
                dot += g[j][i] * v[j][i];
            }
            if (so != nullptr) {
                store8<float>(so + c * 8, o);
                store8<float>(sq + c * 8, q);
            }
        }
    }
    if (dh == nullptr && dres == nullptr) return;
    dot = wave_sum(dot) * inv_d;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            float dv[8];
#pragma unroll
            for (int i = 0; i < 8; ++i) dv[i] = rstd * (g[j][i] - v[j][i] * dot);
            if (dh != nullptr) store8<T>(dh + row * D + c * 8, dv);
            if (dres != nullptr) store8<RT>(dres + row * D + c * 8, dv);
        }
    }
}

template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(256, MAXC <= 2 ? 2 : 1) void loss_head_bwd_kernel(const T* __restrict__ h, const RT* __restrict__ res, const float* __restrict__ w,
                                                            const float* __restrict__ emb, const int32_t* __restrict__ comp8,
                                                            const int32_t* __restrict__ labels, const float* __restrict__ loss_w,
                                                            int ignore_index, const float* __restrict__ dsum,
                                                            const float* __restrict__ dnll, T* __restrict__ dh, RT* __restrict__ dres,
                                                            float* __restrict__ part, int B, int L, int D, float eps, int nseg) {
    extern __shared__ float lds[];
    constexpr int NM = 2 * MAXC;                    // columns per lane of the partial sums: D <= 256 NM
    float* const so = lds;                          // [LHB_SLOTS][D]  o
    float* const sq = lds + LHB_SLOTS * D;          // [LHB_SLOTS][D]  do vh
    float* const sd = lds + 2 * LHB_SLOTS * D;      // [LHB_SLOTS][8]  cotangent of demb row j from this row
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int g = blockIdx.x % nseg;
    const int b = blockIdx.x / nseg;
    const int nchunk = D >> 3;
    const int t0 = g * LOSS_SEG, t1 = min(L, t0 + LOSS_SEG);
    const bool stage = part != nullptr;

    float acc[8][NM], accn[NM];
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        accn[m] = 0.f;
#pragma unroll
        for (int j = 0; j < 8; ++j) acc[j][m] = 0.f;
    }

    // the segment's labels, one per lane, read once: positions beyond the window count as ignored (a negative label)
    const int seg_label = t0 + lane < t1 ? labels[(int64_t)b * L + t0 + lane] : -1;

    for (int tb = t0; tb < t1; tb += 4) {
        // the round's four labels in every lane: what the block does in this round is the same decision in all of its waves
        bool lab[4];
        int mylabel = -1;
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int label = __builtin_amdgcn_readlane(seg_label, tb - t0 + k);
            lab[k] = !(label == ignore_index || label < 0) && label < 8;          // loss_stage1_kernel's rule
            if (k == wv) mylabel = label;
        }
        const bool any = lab[0] || lab[1] || lab[2] || lab[3];
        const int t = tb + wv;
        if (t < t1) {
            const int64_t at = (int64_t)b * L + t;
            const int64_t rf = at, rr = (int64_t)(B + b) * L + (L - 1 - t);
            bool mine = false;
#pragma unroll
            for (int k = 0; k < 4; ++k) mine = (k == wv) ? lab[k] : mine;
            if (!mine) {
                // an unlabelled position: its two rows carry no gradient
                const float z[8] = {0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f, 0.f};
#pragma unroll
                for (int j = 0; j < MAXC; ++j) {
                    const int c = lane + 64 * j;
                    if (c < nchunk) {
                        if (dh != nullptr) { store8<T>(dh + rf * D + c * 8, z); store8<T>(dh + rr * D + c * 8, z); }
                        if (dres != nullptr) { store8<RT>(dres + rf * D + c * 8, z); store8<RT>(dres + rr * D + c * 8, z); }
                    }
                }
            } else {
                HeadRowKept<MAXC> kf, kr;
                float af[8], ar[8];
                head_row<T, RT, MAXC>(h + rf * D, res, rf, w, emb, comp8, D, eps, 0, 0, lane, nullptr, true, af, kf);
                head_row<T, RT, MAXC>(h + rr * D, res, rr, w, emb, comp8, D, eps, 0, 1, lane, nullptr, true, ar, kr);
                float lg[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) lg[k] = Elem<T>::round(af[k] + ar[k]);
                float mx = lg[0];
#pragma unroll
                for (int k = 1; k < 8; ++k) mx = fmaxf(mx, lg[k]);
                float ex[8], se = 0.f;
#pragma unroll
                for (int k = 0; k < 8; ++k) { ex[k] = expf(lg[k] - mx); se += ex[k]; }
                const float wt = loss_w != nullptr ? loss_w[at] : 1.0f;
                const float up = dsum[b] * wt + (dnll != nullptr ? dnll[at] : 0.f);
                float dl[8];
#pragma unroll
                for (int k = 0; k < 8; ++k) dl[k] = up * (ex[k] / se - (k == mylabel ? 1.0f : 0.f));
                float* const sof = stage ? so + (2 * wv) * D : nullptr;
                float* const sor = stage ? so + (2 * wv + 1) * D : nullptr;
                lhb_row<T, RT, MAXC>(kf.v, kf.rstd, rf, 0, dl, w, emb, comp8, dh, dres, sof, sq + (2 * wv) * D, D, lane);
                lhb_row<T, RT, MAXC>(kr.v, kr.rstd, rr, 1, dl, w, emb, comp8, dh, dres, sor, sq + (2 * wv + 1) * D, D, lane);
                if (stage && lane < 8) {
                    // what this position adds to demb row `lane`: dl[lane] o (forward strand), sum over comp[k] == lane of dl[k] o (rc strand)
                    float df = 0.f, dr = 0.f;
#pragma unroll
                    for (int k = 0; k < 8; ++k) {
                        df = (k == lane) ? dl[k] : df;
                        dr += ((comp8[k] & 7) == lane) ? dl[k] : 0.f;
                    }
                    sd[(2 * wv) * 8 + lane] = df;
                    sd[(2 * wv + 1) * 8 + lane] = dr;
                }
            }
        }
        if (!stage || !any) continue;               // the same decision in every wave of the block
        __syncthreads();
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            if (!lab[k]) continue;
#pragma unroll
            for (int s = 0; s < 2; ++s) {
                const int slot = 2 * k + s;
                float d[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) d[j] = sd[slot * 8 + j];
#pragma unroll
                for (int m = 0; m < NM; ++m) {
                    const int col = (int)threadIdx.x + 256 * m;
                    if (col < D) {
                        const float o = so[slot * D + col];
                        accn[m] += sq[slot * D + col];
#pragma unroll
                        for (int j = 0; j < 8; ++j) acc[j][m] += d[j] * o;
                    }
                }
            }
        }
        __syncthreads();                            // the next round writes the slots again
    }
    if (!stage) return;
    float* const prow = part + (int64_t)blockIdx.x * 9 * D;
#pragma unroll
    for (int m = 0; m < NM; ++m) {
        const int col = (int)threadIdx.x + 256 * m;
        if (col < D) {
#pragma unroll
            for (int j = 0; j < 8; ++j) prow[(int64_t)j * D + col] = acc[j][m];
            prow[(int64_t)8 * D + col] = accn[m];
        }
    }
}

hipError_t launch_loss_head_bwd(const LossHeadBwdLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (in.res_frag || in.D <= 0 || in.L <= 0 || !in.h || !in.res || !in.w || !a.emb_f32 || !a.comp8 || !a.labels || !a.dsum)
        return hipErrorInvalidValue;
    if (!a.dh && !a.dres && !a.dnorm_w && !a.demb) return hipErrorInvalidValue;
    if (in.B <= 0) return hipSuccess;
    const bool params = a.dnorm_w != nullptr || a.demb != nullptr;
    if (params && !a.scratch) return hipErrorInvalidValue;
    const int nseg = lhb_segments(in.L);
    const int64_t blocks = (int64_t)in.B * nseg;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    float* const part = params ? (float*)a.scratch : nullptr;
    const int lds = params ? (int)lhb_lds_bytes(in.D) : 0;
    hipError_t err = select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        const auto kernel = loss_head_bwd_kernel<T, RT, decltype(form)::MAXC>;
        // the attribute is set once per kernel: to what the widest row of this instantiation needs (D = 512 MAXC)
        if (lds > 0)
            if (hipError_t e = ensure_dynamic_lds((const void*)kernel, (int)lhb_lds_bytes(512 * decltype(form)::MAXC))) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(256), lds, s, (const T*)in.h, (const RT*)in.res, in.w, a.emb_f32, a.comp8, a.labels,
                           a.loss_w, a.ignore_index, a.dsum, a.dnll, (T*)a.dh, (RT*)a.dres, part, in.B, in.L, in.D, in.eps, nseg);
        return hipGetLastError();
    });
    if (err != hipSuccess || !params) return err;
    // the output nobody asked for is summed into the spare row behind the blocks' rows
    float* const spare = part + blocks * 9 * in.D;
    return launch_sum_partials(part, blocks, a.demb ? a.demb : spare, 8 * in.D, a.dnorm_w ? a.dnorm_w : spare + (int64_t)8 * in.D, in.D, s);
}

}  // namespace pcad
