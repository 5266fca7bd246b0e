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

template <typename T, typename RT>
static hipError_t launch_probs_t(const void* h, const void* res, const float* w, const float* emb_f32, const int32_t* comp8,
                                 ProbCols cols, float* probs_out, float* logits_out, int B, int L, int D, float eps, Positions pos,
                                 const int32_t* pos_per_window, int Pw, int h_compact, const int32_t* ids, int32_t* status,
                                 int res_frag, hipStream_t s) {
    const int64_t items = (int64_t)B * (pos_per_window ? Pw : (pos.n ? pos.n : L));
    const dim3 grid((unsigned)((items + PROBS_WAVES - 1) / PROBS_WAVES)), blk(64 * PROBS_WAVES);
#define PCAD_PROBS(MC)                                                                                                           \
    hipLaunchKernelGGL((probs_head_kernel<T, RT, MC>), grid, blk, 0, s, (const T*)h, (const RT*)res, w, emb_f32, comp8, cols,   \
                       probs_out, logits_out, B, L, D, eps, pos, pos_per_window, Pw, h_compact, ids, status, res_frag)
    if (D <= 512) PCAD_PROBS(1);
    else if (D <= 1024) PCAD_PROBS(2);
    else PCAD_PROBS(4);
#undef PCAD_PROBS
    return hipGetLastError();
}

hipError_t launch_probs_head(const void* h, const void* res, const float* w, const float* emb_f32, const int32_t* comp8, ProbCols cols,
                             float* probs_out, float* logits_out, int B, int L, int D, float eps, Positions pos,
                             const int32_t* pos_per_window, int Pw, int dt, int rdt, hipStream_t s, bool h_compact, const int32_t* ids,
                             int32_t* status, int res_frag) {
    if (D % 8 || D > 2048 || L <= 0) return hipErrorInvalidValue;
    if (pos_per_window && (pos.n != 0 || Pw < 1 || Pw > 16)) return hipErrorInvalidValue;
    if (h_compact && (pos_per_window || pos.n == 0)) return hipErrorInvalidValue;
    if (((uintptr_t)probs_out) % 16) return hipErrorInvalidValue;                    // one 16-byte store per row
    for (int j = 0; j < 4; ++j)
        if ((unsigned)cols.c[j] > 7u) return hipErrorInvalidValue;
    if (res_frag && (rdt != F32 || res_frag % 256 || res_frag < D || ((int64_t)2 * B * L) % 256)) return hipErrorInvalidValue;
    if (B <= 0 || (probs_out == nullptr && logits_out == nullptr)) return hipSuccess;
    const int64_t items = (int64_t)B * (pos_per_window ? Pw : (pos.n ? pos.n : L));
    if ((items + PROBS_WAVES - 1) / PROBS_WAVES > 0x7fffffff) return hipErrorInvalidValue;
    const int hc = h_compact ? 1 : 0;
    if (dt == BF16 && rdt == F32)
        return launch_probs_t<bf16_t, float>(h, res, w, emb_f32, comp8, cols, probs_out, logits_out, B, L, D, eps, pos, pos_per_window, Pw, hc, ids, status, res_frag, s);
    if (dt == BF16 && rdt == BF16)
        return launch_probs_t<bf16_t, bf16_t>(h, res, w, emb_f32, comp8, cols, probs_out, logits_out, B, L, D, eps, pos, pos_per_window, Pw, hc, ids, status, res_frag, s);
    if (dt == F32 && rdt == F32)
        return launch_probs_t<float, float>(h, res, w, emb_f32, comp8, cols, probs_out, logits_out, B, L, D, eps, pos, pos_per_window, Pw, hc, ids, status, res_frag, s);
    return hipErrorInvalidValue;
}

}  // namespace pcad
