// Nucleotide-probability head: final_head_kernel's logits (head_row.hpp: the same row arithmetic and rounding
// points) followed by the softmax over four chosen vocabulary columns, at the evaluated positions only.
//
//   logit[v] = round(round(H_f . Emb[v]) + round(H_r . Emb[comp[v]]))     H_f / H_r = round(norm_f(res + h)) of rows (b, p) / (B + b, L-1-p)
//   probs[j] = exp(logit[cols[j]] - m) / sum_j exp(logit[cols[j]] - m)     fp32, m = max_j logit[cols[j]] (torch.softmax)
//
// Positions: all L, a shared by-value list (pos.n > 0; h may then hold the evaluated rows only, h_compact), or a device list per window
// (pos_per_window [B, Pw]; a value outside [0, L) is clamped and reported).  One launch: one WAVE per evaluated (window, position); it
// runs BOTH strands' rows itself and stores the four probabilities as one 16-byte vector - no hand-over between waves, no atomics on
// data, so a window's probabilities depend on its own rows only.
#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int PROBS_STATUS_BAD_TOKEN_BIT = 1, PROBS_STATUS_BAD_POSITION_BIT = 2;     // = pcad.h PCAD_STATUS_BAD_TOKEN / PCAD_STATUS_BAD_POSITION
constexpr int PROBS_WAVES = 4;                                                       // evaluated positions per block

template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(64 * PROBS_WAVES) void probs_head_kernel(const T* __restrict__ h, const RT* __restrict__ res,
                                                                      const float* __restrict__ w, const float* __restrict__ emb,
                                                                      const int32_t* __restrict__ comp8, ProbCols cols,
                                                                      float* __restrict__ probs_out, float* __restrict__ logits_out,
                                                                      int B, int L, int D, float eps, Positions pos,
                                                                      const int32_t* __restrict__ pos_per_window, int Pw, int h_compact,
                                                                      const int32_t* __restrict__ ids, int32_t* __restrict__ status,
                                                                      int res_frag) {
    const int lane = threadIdx.x & 63;
    const int Q = pos_per_window ? Pw : (pos.n ? pos.n : L);
    const int64_t item = (int64_t)blockIdx.x * PROBS_WAVES + (threadIdx.x >> 6);      // = b * Q + q, wave-uniform
    if (item >= (int64_t)B * Q) return;
    const int b = (int)(item / Q), q = (int)(item - (int64_t)b * Q);
    int p = q;
    // input validation as final_head_kernel does it: the wave of a window's first evaluated position scans the window's ids, and
    // every wave checks its own per-window position (clamped below so that nothing is read out of bounds)
    if (status != nullptr && ids != nullptr && q == 0) {
        bool bad = false;
        for (int t = lane; t < L; t += 64) bad |= (unsigned)ids[(int64_t)b * L + t] > 7u;
        if (__any(bad) && lane == 0) atomicOr(status, PROBS_STATUS_BAD_TOKEN_BIT);
    }
    if (pos_per_window) {
        const int raw = pos_per_window[item];
        if (status != nullptr && lane == 0 && (unsigned)raw >= (unsigned)L) atomicOr(status, PROBS_STATUS_BAD_POSITION_BIT);
        p = min(max(raw, 0), L - 1);
    } else if (pos.n) {
        // uniform select from the by-value array (avoids runtime-indexed kernarg scratch)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i == q) p = pos.p[i];
    }
    const int64_t rf = (int64_t)b * L + p, rr = (int64_t)(B + b) * L + (L - 1 - p);
    const int64_t hf = h_compact ? item : rf, hr = h_compact ? ((int64_t)(B + b) * Q + q) : rr;      // mixer output: evaluated rows only, or the full tensor
    float af[8], ar[8];
    head_row<T, RT, MAXC>(h + hf * D, res, rf, w, emb, comp8, D, eps, res_frag, 0, lane, nullptr, true, af);
    head_row<T, RT, MAXC>(h + hr * D, res, rr, w, emb, comp8, D, eps, res_frag, 1, lane, nullptr, true, ar);
    float lg[8];
#pragma unroll
    for (int k = 0; k < 8; ++k) lg[k] = Elem<T>::round(af[k] + ar[k]);
    if (logits_out != nullptr && lane < 8) {
        float mine = lg[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) mine = (lane == k) ? lg[k] : mine;
        logits_out[item * 8 + lane] = mine;
    }
    if (probs_out == nullptr || lane != 0) return;
    // the four chosen columns by uniform selects (no runtime-indexed registers), then softmax as torch forms it
    float x[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        x[j] = lg[0];
#pragma unroll
        for (int k = 1; k < 8; ++k) x[j] = (cols.c[j] == k) ? lg[k] : x[j];
    }
    float m = x[0];
#pragma unroll
    for (int j = 1; j < 4; ++j) m = x[j] > m ? x[j] : m;
    float ex[4], se = 0.f;
#pragma unroll
    for (int j = 0; j < 4; ++j) { ex[j] = expf(x[j] - m); se += ex[j]; }
    *reinterpret_cast<f32x4*>(probs_out + item * 4) = f32x4{ex[0] / se, ex[1] / se, ex[2] / se, ex[3] / se};
}

hipError_t launch_probs_head(const ProbsHeadLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (in.L <= 0) return hipErrorInvalidValue;
    if (a.pos_per_window && (a.pos.n != 0 || a.Pw < 1 || a.Pw > 16)) return hipErrorInvalidValue;
    if (a.h_compact && (a.pos_per_window || a.pos.n == 0)) return hipErrorInvalidValue;
    if (((uintptr_t)a.probs_out) % 16) return hipErrorInvalidValue;                  // one 16-byte store per row
    for (int j = 0; j < 4; ++j)
        if ((unsigned)a.cols.c[j] > 7u) return hipErrorInvalidValue;
    if (in.B <= 0 || (a.probs_out == nullptr && a.logits_out == nullptr)) return hipSuccess;
    const int64_t blocks = ((int64_t)in.B * (a.pos_per_window ? a.Pw : (a.pos.n ? a.pos.n : in.L)) + PROBS_WAVES - 1) / PROBS_WAVES;
    if (blocks > 0x7fffffff) return hipErrorInvalidValue;
    return select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        hipLaunchKernelGGL((probs_head_kernel<T, RT, decltype(form)::MAXC>), dim3((unsigned)blocks), dim3(64 * PROBS_WAVES), 0, s, (const T*)in.h, (const RT*)in.res,
                           in.w, a.emb_f32, a.comp8, a.cols, a.probs_out, a.logits_out, in.B, in.L, in.D, in.eps, a.pos, a.pos_per_window, a.Pw,
                           a.h_compact ? 1 : 0, in.ids, in.status, in.res_frag);
        return hipGetLastError();
    });
}

}  // namespace pcad
