// One strand's row of the LM head, shared by final_head_kernel (norm.hip), loss_stage1_kernel (loss.hip), probs_head_kernel (probs.hip) and
// loss_head_bwd_kernel (loss_bwd.hip, which recomputes the forward's logits through it): ONE
// head arithmetic:  v = h + res (fp32);  o = round(v * rstd(v) * w);  acc[k] = round(o . Emb[strand 0: k, strand 1: comp[k]]).
// One wave per row, 8 columns per lane and step (16-byte accesses); `row` indexes the full [2B * L, D] residual tensor, h_row
// points at the mixer output's row.  res_frag != 0: fp32 residual in the GEMM's fragment layout of that (padded) width.
#pragma once
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

// ---- host side: which <T, RT, MAXC> instantiation of a one-wave-per-row kernel family (norm.hip, pool.hip, loss.hip, probs.hip) a
// launch runs.  A launcher names its family once, in a generic callable that takes the RowForm, and launches with one statement.
template <typename T, typename RT, int MC>
struct RowForm { using X = T;  using R = RT;  static constexpr int MAXC = MC; };      // activation type, residual type, 64-lane steps of 8 columns per row
// the width selector: D <= 512 / <= 1024 / <= 2048 columns
template <typename T, typename RT, typename F>
static hipError_t select_row_width(int D, F&& f) {
    return D <= 512 ? f(RowForm<T, RT, 1>{}) : D <= 1024 ? f(RowForm<T, RT, 2>{}) : f(RowForm<T, RT, 4>{});
}
// the dtype-pair selector: the three (activation, residual) pairs the library contains
template <typename F>
static hipError_t select_row_form(int dt, int rdt, int D, F&& f) {
    if (dt == BF16 && rdt == F32) return select_row_width<bf16_t, float>(D, f);
    if (dt == BF16 && rdt == BF16) return select_row_width<bf16_t, bf16_t>(D, f);
    if (dt == F32 && rdt == F32) return select_row_width<float, float>(D, f);
    return hipErrorInvalidValue;
}

// hidden_dst (or nullptr): the [2D] row of hidden_states[-1] this strand's half is written to (rc strand: reversed channels).
// want_logits: acc[0..7] = the strand's 8 partial logits, rounded to the model dtype, the same value in every lane.
// `keep` is handed what a backward needs of the row: v = h + res of the lane's chunks and the row's rstd.  The inference callers pass
// none and both are dropped (HeadRowDrop); loss_bwd.hip passes a HeadRowKept, which stores them.
struct HeadRowDrop {
    template <int MAXC> __device__ __forceinline__ void take(const float (&)[MAXC][8], float, int, int) {}
};
template <int MAXC>
struct HeadRowKept {
    float v[MAXC][8];                 // chunks beyond the row are not written
    float rstd;
    __device__ __forceinline__ void take(const float (&src)[MAXC][8], float r, int lane, int nchunk) {
        rstd = r;
#pragma unroll
        for (int j = 0; j < MAXC; ++j)
            if (lane + 64 * j < nchunk) {
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j][i] = src[j][i];
            }
    }
};
template <typename T, typename RT, int MAXC, typename Keep = HeadRowDrop>
__device__ __forceinline__ void head_row(const T* __restrict__ h_row, const RT* __restrict__ res, int64_t row,
                                         const float* __restrict__ w, const float* __restrict__ emb,
                                         const int32_t* __restrict__ comp8, int D, float eps, int res_frag, int strand, int lane,
                                         T* __restrict__ hidden_dst, bool want_logits, float (&acc)[8], Keep&& keep = Keep{}) {
    // every product below is rounded before it is added (no fused multiply-add), whatever kernel this is inlined into: the two
    // callers must give the same logits bit for bit, and contraction is otherwise decided per call site
#pragma clang fp contract(off)
    const int nchunk = D >> 3;
    float v[MAXC][8];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            float r[8];
            load8<T>(h_row + c * 8, v[j]);
            if (res_frag) {                  // norm-folded form: fp32 residual in the GEMM's fragment layout (RT == float)
                const float* rp = reinterpret_cast<const float*>(res) + res_frag_off(row, c * 8, res_frag);      // res_frag = padded width Dp
                const f32x4 a = *reinterpret_cast<const f32x4*>(rp), b = *reinterpret_cast<const f32x4*>(rp + 256);
                r[0] = a[0]; r[1] = a[1]; r[2] = a[2]; r[3] = a[3]; r[4] = b[0]; r[5] = b[1]; r[6] = b[2]; r[7] = b[3];
            } else {
                load8<RT>(res + row * D + c * 8, r);
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) { v[j][i] += r[i]; ss += v[j][i] * v[j][i]; }
        }
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)D + eps);
    keep.take(v, rstd, lane, nchunk);
#pragma unroll
    for (int k = 0; k < 8; ++k) acc[k] = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            float wvv[8], o[8];
            load8<float>(w + c * 8, wvv);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = Elem<T>::round(v[j][i] * rstd * wvv[i]);
            if (hidden_dst != nullptr) {
                if (strand == 0) {
                    store8<T>(hidden_dst + c * 8, o);
                } else {
                    float rv[8];
#pragma unroll
                    for (int i = 0; i < 8; ++i) rv[i] = o[7 - i];
                    store8<T>(hidden_dst + D + (D - 8 - c * 8), rv);
                }
            }
            if (want_logits) {
#pragma unroll
                for (int k = 0; k < 8; ++k) {
                    const int er = strand == 0 ? k : (comp8[k] & 7);
                    float e[8];
                    load8<float>(emb + (int64_t)er * D + c * 8, e);
#pragma unroll
                    for (int i = 0; i < 8; ++i) acc[k] += o[i] * e[i];
                }
            }
        }
    }
    if (want_logits) {
#pragma unroll
        for (int k = 0; k < 8; ++k) acc[k] = Elem<T>::round(wave_sum(acc[k]));
    }
}

}  // namespace pcad
