// Masked-LM loss head (CaduceusForMaskedLM with labels): final_head_kernel's logits (head_row.hpp: the same row
// arithmetic and rounding points) followed by the cross entropy of every labelled position, reduced per window.
//
//   logit[v] = round(round(H_f . Emb[v]) + round(H_r . Emb[comp[v]]))     H_f / H_r = round(norm_f(res + h)) of rows (b, p) / (B + b, L-1-p)
//   nll      = logsumexp_v(logit) - logit[label]                           fp32, over all 8 logits (F.cross_entropy)
//   sums[b]  = { sum w nll, sum w, labelled positions, labelled positions whose arg-max logit is the label }
//
// Two launches, no floating-point atomics:
//   stage 1  one block per (window, 64-position segment): each of the 4 waves walks positions t0 + wave, t0 + wave + 4, ... and runs
//            BOTH strands' rows of a position itself (no hand-over between waves), keeps its four running sums in position order;
//            the waves' sums are added in wave order and the block writes one partial [4].  A position whose label is ignored is
//            skipped before any row is loaded unless logits_out is wanted.
//   stage 2  one block per window adds the segments' partials in segment order.
// The segmentation depends on L only, so a window's four numbers do not depend on the batch or chunk it runs in.
#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int LOSS_STATUS_BAD_TOKEN_BIT = 1, LOSS_STATUS_BAD_LABEL_BIT = 4;     // = pcad.h PCAD_STATUS_BAD_TOKEN / PCAD_STATUS_BAD_LABEL

int loss_segments(int L) { return (L + LOSS_SEG - 1) / LOSS_SEG; }

size_t loss_partial_bytes(int B, int L) { return (size_t)B * (size_t)loss_segments(L) * 4 * sizeof(float); }

template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(256) void loss_stage1_kernel(const T* __restrict__ h, const RT* __restrict__ res,
                                                          const float* __restrict__ w, const float* __restrict__ emb,
                                                          const int32_t* __restrict__ comp8, const int32_t* __restrict__ labels,
                                                          const float* __restrict__ loss_w, int ignore_index,
                                                          float* __restrict__ part, float* __restrict__ nll_out,
                                                          float* __restrict__ logits_out, int B, int L, int D, float eps, int nseg,
                                                          const int32_t* __restrict__ ids, int32_t* __restrict__ status,
                                                          int res_frag) {
    __shared__ float red[3][4];          // waves 1..3 hand their sums to wave 0
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;
    const int g = blockIdx.x % nseg;
    const int b = blockIdx.x / nseg;
    // input validation as final_head_kernel does it: the first block of every window scans its ids
    if (status != nullptr && ids != nullptr && g == 0) {
        bool bad = false;
        for (int t = threadIdx.x; t < L; t += 256) bad |= (unsigned)ids[(int64_t)b * L + t] > 7u;
        if (__any(bad) && lane == 0) atomicOr(status, LOSS_STATUS_BAD_TOKEN_BIT);
    }
    const int t0 = g * LOSS_SEG, t1 = min(L, t0 + LOSS_SEG);
    float s_wnll = 0.f, s_w = 0.f, s_n = 0.f, s_ok = 0.f;
    for (int t = t0 + wv; t < t1; t += 4) {
        const int64_t at = (int64_t)b * L + t;
        const int label = labels[at];
        // ignored: ignore_index or any negative label; any other label outside the (padded) vocabulary is reported and skipped
        const bool labelled = !(label == ignore_index || label < 0) && label < 8;
        if (label > 7 && label != ignore_index && status != nullptr && lane == 0) atomicOr(status, LOSS_STATUS_BAD_LABEL_BIT);
        if (!labelled && logits_out == nullptr) {
            if (nll_out != nullptr && lane == 0) nll_out[at] = 0.f;
            continue;
        }
        const int64_t rf = at, rr = (int64_t)(B + b) * L + (L - 1 - t);
        float af[8], ar[8];
        head_row<T, RT, MAXC>(h + rf * D, res, rf, w, emb, comp8, D, eps, res_frag, 0, lane, nullptr, true, af);
        head_row<T, RT, MAXC>(h + rr * D, res, rr, w, emb, comp8, D, eps, res_frag, 1, lane, nullptr, true, ar);
        float lg[8];
#pragma unroll
        for (int k = 0; k < 8; ++k) lg[k] = Elem<T>::round(af[k] + ar[k]);
        if (logits_out != nullptr && lane < 8) {
            float mine = lg[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) mine = (lane == k) ? lg[k] : mine;
            logits_out[at * 8 + lane] = mine;
        }
        if (!labelled) {
            if (nll_out != nullptr && lane == 0) nll_out[at] = 0.f;
            continue;
        }
        // log_softmax as torch forms it: (x - max) - log(sum exp(x - max)); every lane holds the same 8 values
        float m = lg[0], pick = lg[0];
        int arg = 0;
#pragma unroll
        for (int k = 1; k < 8; ++k) {
            if (lg[k] > m || (lg[k] != lg[k] && m == m)) { m = lg[k]; arg = k; }      // first index on ties; a NaN wins (torch.argmax)
            pick = (label == k) ? lg[k] : pick;
        }
        float se = 0.f;
#pragma unroll
        for (int k = 0; k < 8; ++k) se += expf(lg[k] - m);
        const float nll = logf(se) - (pick - m);
        const float wt = loss_w != nullptr ? loss_w[at] : 1.0f;
        if (nll_out != nullptr && lane == 0) nll_out[at] = nll;
        s_wnll += wt * nll;
        s_w += wt;
        s_n += 1.0f;
        s_ok += (arg == label) ? 1.0f : 0.f;
    }
    if (wv > 0 && lane == 0) { red[wv - 1][0] = s_wnll; red[wv - 1][1] = s_w; red[wv - 1][2] = s_n; red[wv - 1][3] = s_ok; }
    __syncthreads();
    if (wv != 0 || lane != 0) return;
#pragma unroll
    for (int k = 0; k < 3; ++k) { s_wnll += red[k][0]; s_w += red[k][1]; s_n += red[k][2]; s_ok += red[k][3]; }      // wave order
    *reinterpret_cast<f32x4*>(part + ((int64_t)b * nseg + g) * 4) = f32x4{s_wnll, s_w, s_n, s_ok};
}

__global__ __launch_bounds__(64) void loss_stage2_kernel(const float* __restrict__ part, float* __restrict__ sums_out, int nseg) {
    const int b = blockIdx.x, k = threadIdx.x;
    if (k >= 4) return;
    const float* p = part + (int64_t)b * nseg * 4 + k;
    float a = p[0];
    for (int g = 1; g < nseg; ++g) a += p[(int64_t)g * 4];      // segment order: deterministic
    sums_out[(int64_t)b * 4 + k] = a;
}

hipError_t launch_loss_head(const LossHeadLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (in.L <= 0 || a.labels == nullptr || a.sums_out == nullptr || a.part == nullptr) return hipErrorInvalidValue;
    if (in.B <= 0) return hipSuccess;
    const int nseg = loss_segments(in.L);
    if ((int64_t)in.B * nseg > 0x7fffffff) return hipErrorInvalidValue;
    return select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        hipLaunchKernelGGL((loss_stage1_kernel<T, RT, decltype(form)::MAXC>), dim3((unsigned)((int64_t)in.B * nseg)), dim3(256), 0, s, (const T*)in.h, (const RT*)in.res,
                           in.w, a.emb_f32, a.comp8, a.labels, a.loss_w, a.ignore_index, (float*)a.part, a.nll_out, a.logits_out, in.B, in.L, in.D, in.eps, nseg,
                           in.ids, in.status, in.res_frag);
        if (hipError_t e = hipGetLastError()) return e;
        hipLaunchKernelGGL(loss_stage2_kernel, dim3((unsigned)in.B), dim3(64), 0, s, (const float*)a.part, a.sums_out, nseg);
        return hipGetLastError();
    });
}

}  // namespace pcad
