// Fused residual-add + RMSNorm family (HBM-bound; one wave per token row, 16-byte accesses).
//
// Replaces mamba_ssm.ops.triton.layer_norm.rms_norm_fn as called by RCPSMambaBlock (fused_add_norm=True)
// and the final norm_f.  The reference runs it twice per layer — once per RC
// half, the rc half on a flipped copy; here both strands are plain rows of the 2B-strand batch, so one
// launch covers them and no flip copy exists.  The layer-0 variant gathers the embedding rows on the fly
// (RCPSEmbedding: rc strand = complement of the reversed ids, by index arithmetic), and the final variant
// fuses norm_f, the RC re-assembly of hidden_states[-1] and the tied RCPS LM head at the requested
// positions only.
#include <type_traits>

#include "common.hpp"
#include "head_row.hpp"
#include "kernels.hpp"

namespace pcad {

constexpr int PCAD_STATUS_BAD_TOKEN_BIT = 1, PCAD_STATUS_BAD_POSITION_BIT = 2;     // = pcad.h PCAD_STATUS_*

// FOLD (norm-folded layer form, api.hip): y = the UN-normalised sum rounded to the model dtype and rstd_out[row] = its rstd; the
// norm weight lives in the in_proj weight (folded at bind time) and rstd is applied by in_proj's epilogue.
// SPLIT (T == float only; api.hip "f32_gemm_split"): y is a bf16 tensor [rows, 2 D] = [hi | lo] of the normalised row
// (hi = bf16(v), lo = bf16(v - hi)): the A operand of the split-bf16 in_proj (pack.hip), written here instead of the fp32 row.
template <typename T, typename RT, int MAXC, bool EMBED, bool FOLD = false, bool SPLIT = false>
__global__ __launch_bounds__(256) void add_rmsnorm_kernel(const T* __restrict__ x, const RT* __restrict__ res_in,
                                                          const float* __restrict__ w, T* __restrict__ y,
                                                          RT* __restrict__ res_out, int64_t rows, int D, float eps,
                                                          const int32_t* __restrict__ ids,
                                                          const int32_t* __restrict__ comp8, int B, int L,
                                                          float* __restrict__ rstd_out = nullptr, int Dp = 0) {
    const int lane = threadIdx.x & 63;
    const int64_t row = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    if (row >= rows) return;
    const int nchunk = D >> 3;
    const T* xr;
    if constexpr (EMBED) {
        const int s = (int)(row / L), t = (int)(row - (int64_t)s * L);
        int tok;
        if (s < B) tok = ids[(int64_t)s * L + t];
        else tok = comp8[ids[(int64_t)(s - B) * L + (L - 1 - t)] & 7];
        xr = x + (int64_t)(tok & 7) * D;
    } else {
        xr = x + row * D;
    }
    float v[MAXC][8];
    float ss = 0.f;
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            load8<T>(xr + c * 8, v[j]);
            if (res_in != nullptr) {
                float r[8];
                load8<RT>(res_in + row * D + c * 8, r);
#pragma unroll
                for (int i = 0; i < 8; ++i) v[j][i] += r[i];
            }
#pragma unroll
            for (int i = 0; i < 8; ++i) ss += v[j][i] * v[j][i];
            if constexpr (FOLD) {          // the fp32 residual stream in the 4-wave GEMM's fragment layout: 8 columns = two quads
                const int64_t o = res_frag_off(row, c * 8, Dp);
                float* ro = reinterpret_cast<float*>(res_out);
                *reinterpret_cast<f32x4*>(ro + o) = f32x4{v[j][0], v[j][1], v[j][2], v[j][3]};
                *reinterpret_cast<f32x4*>(ro + o + 256) = f32x4{v[j][4], v[j][5], v[j][6], v[j][7]};
            } else if (res_out != nullptr) {
                store8<RT>(res_out + row * D + c * 8, v[j]);
            }
        } else if constexpr (FOLD) {
            // d_model that is not a multiple of 256 (l20: 384): the residual tensor is Dp = round_up(D, 256) columns wide (the folded
            // out_proj runs whole 256-column tiles against zero weight rows); its padding columns must start as zeros
            if (c < (Dp >> 3)) {
                const int64_t o = res_frag_off(row, c * 8, Dp);
                float* ro = reinterpret_cast<float*>(res_out);
                *reinterpret_cast<f32x4*>(ro + o) = f32x4{0.f, 0.f, 0.f, 0.f};
                *reinterpret_cast<f32x4*>(ro + o + 256) = f32x4{0.f, 0.f, 0.f, 0.f};
            }
        }
    }
    ss = wave_sum(ss);
    const float rstd = rsqrtf(ss / (float)D + eps);
    if constexpr (FOLD) {
        if (lane == 0) rstd_out[row] = rstd;
#pragma unroll
        for (int j = 0; j < MAXC; ++j) {
            const int c = lane + 64 * j;
            if (y != nullptr && c < nchunk) store8<T>(y + row * Dp + c * 8, v[j]);       // u: rows of Dp elements (padding never read)
        }
        return;
    }
#pragma unroll
    for (int j = 0; j < MAXC; ++j) {
        const int c = lane + 64 * j;
        if (c < nchunk) {
            float wv[8], o[8];
            load8<float>(w + c * 8, wv);
#pragma unroll
            for (int i = 0; i < 8; ++i) o[i] = v[j][i] * rstd * wv[i];
            if constexpr (SPLIT) {
                bf16_t* ys = reinterpret_cast<bf16_t*>(y) + row * 2 * D + c * 8;
                float lo[8];
#pragma unroll
                for (int i = 0; i < 8; ++i) lo[i] = o[i] - round_to_bf16(o[i]);
                store8<bf16_t>(ys, o);
                store8<bf16_t>(ys + D, lo);
            } else {
                store8<T>(y + row * D + c * 8, o);
            }
        }
    }
}

// rstd[row] = rsqrt(sum_p ssq[row][p] / D + eps): the per-wave-tile partial sums of squares the folded out_proj epilogue wrote
// (gemm.hip EPI_RES), summed in a fixed order (deterministic)
__global__ __launch_bounds__(256) void rstd_kernel(const float* __restrict__ ssq, float* __restrict__ rstd, int64_t rows, int np,
                                                   float inv_d, float eps) {
    // a block owns 256 consecutive rows = one contiguous run of 256 * np partials: staged through LDS with coalesced loads (np = 6 at
    // d_model 768: per-thread reads of 24-byte rows cost 0.34 ms per launch before), then one thread per row adds its np values in
    // index order (deterministic)
    __shared__ float part[256 * 16];
    const int64_t row0 = (int64_t)blockIdx.x * 256;
    const int nrow = (int)min((int64_t)256, rows - row0);
    const float* src = ssq + row0 * np;
    for (int i = threadIdx.x; i < nrow * np; i += 256) part[i] = src[i];
    __syncthreads();
    if ((int)threadIdx.x >= nrow) return;
    float acc = 0.f;
    for (int i = 0; i < np; ++i) acc += part[threadIdx.x * np + i];
    rstd[row0 + threadIdx.x] = rsqrtf(acc * inv_d + eps);
}

hipError_t launch_rstd(const float* ssq, float* rstd, int64_t rows, int np, int D, float eps, hipStream_t s) {
    if (rows <= 0) return hipSuccess;
    if (np <= 0 || np > 16) return hipErrorInvalidValue;          // d_model <= 2048 -> at most 16 partials per row
    hipLaunchKernelGGL(rstd_kernel, dim3((unsigned)((rows + 255) / 256)), dim3(256), 0, s, ssq, rstd, rows, np, 1.0f / (float)D, eps);
    return hipGetLastError();
}

// One entry for both forms.  The kernel family: <T, RT, MAXC, EMBED> plain, <.., EMBED, false, true> split (fp32 only) and
// <.., true, true> folded (embed only).
template <bool EMBED>
static hipError_t launch_norm(const NormLaunch& n, const EmbedRows& e, int64_t rows, hipStream_t s) {
    if (n.D % 8 || n.D > 2048) return hipErrorInvalidValue;
    if (n.split_y && !(n.dt == F32 && n.rdt == F32 && n.rstd_out == nullptr)) return hipErrorInvalidValue;
    if (!EMBED && (n.rstd_out != nullptr || n.Dp != 0)) return hipErrorInvalidValue;
    return select_row_form(n.dt, n.rdt, n.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        constexpr int MAXC = decltype(form)::MAXC;
        if (rows <= 0) return hipSuccess;
        auto launch = [&](auto kernel, float* rstd_out, int Dp) {
            hipLaunchKernelGGL(kernel, dim3((unsigned)((rows + 3) / 4)), dim3(256), 0, s, (const T*)(EMBED ? e.emb : n.x), (const RT*)(EMBED ? nullptr : n.res_in),
                               n.w, (T*)n.y, (RT*)n.res_out, rows, n.D, n.eps, e.ids, e.comp8, e.B, e.L, rstd_out, Dp);
            return hipGetLastError();
        };
        if constexpr (std::is_same<T, float>::value)
            if (n.split_y) return launch(add_rmsnorm_kernel<T, RT, MAXC, EMBED, false, true>, nullptr, 0);      // fp32 model, split-bf16 in_proj operand
        if constexpr (EMBED)
            if (n.rstd_out != nullptr) return launch(add_rmsnorm_kernel<T, RT, MAXC, true, true>, n.rstd_out, n.Dp ? n.Dp : n.D);      // layer 0 of the norm-folded form
        return launch(add_rmsnorm_kernel<T, RT, MAXC, EMBED>, nullptr, 0);
    });
}

hipError_t launch_add_rmsnorm(const NormLaunch& n, hipStream_t s) {
    return launch_norm<false>(n, {.ids = nullptr, .emb = nullptr, .comp8 = nullptr, .B = 0, .L = 1}, n.rows, s);
}

hipError_t launch_embed_rmsnorm(const NormLaunch& n, const EmbedRows& e, hipStream_t s) {
    return launch_norm<true>(n, e, (int64_t)2 * e.B * e.L, s);
}

// ------------------------------------------------------------------------------------------------
// final: res = h + res ; H = norm_f(res) ; hidden[b,q] = cat(Hf[b,p], reverse_channels(Hr[b,L-1-p])) ;
// logits[b,q,v] = Hf[b,p].Emb[v] + Hr[b,L-1-p].Emb[comp[v]]   (RCPSLMHead, weight tied to the embedding)
// block = 2 waves: wave 0 the forward strand row, wave 1 the rc strand row.
// ------------------------------------------------------------------------------------------------
template <typename T, typename RT, int MAXC>
__global__ __launch_bounds__(128) void final_head_kernel(const T* __restrict__ h, const RT* __restrict__ res,
                                                         const float* __restrict__ w, const float* __restrict__ emb,
                                                         const int32_t* __restrict__ comp8, T* __restrict__ hidden_out,
                                                         float* __restrict__ logits_out, int B, int L, int D, float eps,
                                                         Positions pos, const int32_t* __restrict__ pos_per_seq, int h_compact,
                                                         const int32_t* __restrict__ ids, int32_t* __restrict__ status, int res_frag) {
    __shared__ float part[8];
    const int lane = threadIdx.x & 63;
    const int wv = threadIdx.x >> 6;   // 0: forward strand, 1: rc strand
    const int Q = pos_per_seq ? 1 : (pos.n ? pos.n : L);
    const int b = blockIdx.x / Q, q = blockIdx.x - b * Q;
    int p = q;
    // Input validation without a host round trip: the reference's nn.Embedding / tensor indexing raise for a token id outside the
    // vocabulary or a position outside the window; here the first block of every window scans its ids (the embedding gather
    // aliased them to id & 7) and every block checks its own position (clamped below so that nothing is read out of bounds), and
    // a violation sets a bit of the caller's status word, which the host reads whenever it next synchronises (pcad.h).
    if (status != nullptr) {
        if (q == 0 && wv == 0 && ids != nullptr) {
            bool bad = false;
            for (int t = lane; t < L; t += 64) bad |= (unsigned)ids[(int64_t)b * L + t] > 7u;
            if (__any(bad) && lane == 0) atomicOr(status, PCAD_STATUS_BAD_TOKEN_BIT);
        }
        if (pos_per_seq && wv == 0 && lane == 0 && (unsigned)pos_per_seq[b] >= (unsigned)L) atomicOr(status, PCAD_STATUS_BAD_POSITION_BIT);
    }
    if (pos_per_seq) {
        p = min(max(pos_per_seq[b], 0), L - 1);      // one evaluated position per window (in-silico mutagenesis sweeps)
    } else if (pos.n) {
        // uniform select from the by-value array (avoids runtime-indexed kernarg scratch)
#pragma unroll
        for (int i = 0; i < 16; ++i)
            if (i == q) p = pos.p[i];
    }
    const int64_t row = wv == 0 ? ((int64_t)b * L + p) : ((int64_t)(B + b) * L + (L - 1 - p));
    const int64_t hrow = h_compact ? ((int64_t)(wv == 0 ? b : B + b) * Q + q) : row;     // mixer output: full tensor or evaluated rows only
    // the strand's row: add + norm_f + its half of hidden_states[-1] + its 8 partial logits (head_row.hpp, shared with loss.hip)
    float acc[8];
    head_row<T, RT, MAXC>(h + hrow * D, res, row, w, emb, comp8, D, eps, res_frag, wv, lane,
                          hidden_out != nullptr ? hidden_out + ((int64_t)b * Q + q) * 2 * D : nullptr, logits_out != nullptr, acc);
    if (logits_out != nullptr) {
        if (wv == 1 && lane < 8) {
            float mine = acc[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) mine = (lane == k) ? acc[k] : mine;
            part[lane] = mine;
        }
        __syncthreads();
        if (wv == 0 && lane < 8) {
            float mine = acc[0];
#pragma unroll
            for (int k = 1; k < 8; ++k) mine = (lane == k) ? acc[k] : mine;
            logits_out[((int64_t)b * Q + q) * 8 + lane] = Elem<T>::round(mine + part[lane]);
        }
    }
}

hipError_t launch_final_head(const FinalHeadLaunch& a, hipStream_t s) {
    const HeadInput& in = a.in;
    if (hipError_t e = head_input_check(in)) return e;
    if (a.h_compact && (a.pos_per_seq || a.pos.n == 0)) return hipErrorInvalidValue;
    const int Q = a.pos_per_seq ? 1 : (a.pos.n ? a.pos.n : in.L);
    if (in.B * Q == 0) return hipSuccess;
    return select_row_form(in.dt, in.rdt, in.D, [&](auto form) {
        using T = typename decltype(form)::X;
        using RT = typename decltype(form)::R;
        hipLaunchKernelGGL((final_head_kernel<T, RT, decltype(form)::MAXC>), dim3((unsigned)(in.B * Q)), dim3(128), 0, s, (const T*)in.h, (const RT*)in.res, in.w,
                           a.emb_f32, a.comp8, (T*)a.hidden_out, a.logits_out, in.B, in.L, in.D, in.eps, a.pos, a.pos_per_seq, a.h_compact ? 1 : 0,
                           in.ids, in.status, in.res_frag);
        return hipGetLastError();
    });
}

// ------------------------------------------------------------------------------------------------
// a = round(a + b) elementwise in the model dtype: BiMambaWrapper's `out + out_rev` (bidirectional_strategy "add") on the two
// directions' out_proj outputs, each already stored in the model dtype - only the strict reference-order form
// (pcad_set_option("reference_order", 2)) materialises them separately.
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void add_round_kernel(T* __restrict__ a, const T* __restrict__ b, int64_t nchunk) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nchunk; i += (int64_t)gridDim.x * blockDim.x) {
        float x[8], y[8];
        load8<T>(a + i * 8, x);
        load8<T>(b + i * 8, y);
#pragma unroll
        for (int k = 0; k < 8; ++k) x[k] += y[k];
        store8<T>(a + i * 8, x);
    }
}

hipError_t launch_add_round(void* a, const void* b, int64_t n, int dt, hipStream_t s) {
    if (n <= 0) return hipSuccess;
    if (n % 8) return hipErrorInvalidValue;
    const int64_t nchunk = n / 8;
    const unsigned grid = (unsigned)((nchunk + 255) / 256 > 16384 ? 16384 : (nchunk + 255) / 256);
    if (dt == BF16) hipLaunchKernelGGL(add_round_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (bf16_t*)a, (const bf16_t*)b, nchunk);
    else hipLaunchKernelGGL(add_round_kernel<float>, dim3(grid), dim3(256), 0, s, (float*)a, (const float*)b, nchunk);
    return hipGetLastError();
}

// ------------------------------------------------------------------------------------------------
// hidden_states[i] in the reference's RCPS layout from the 2B-strand tensor:
// out[b,l,:D] = h[b,l,:] ; out[b,l,D+j] = h[B+b, L-1-l, D-1-j]
// ------------------------------------------------------------------------------------------------
template <typename T>
__global__ __launch_bounds__(256) void assemble_hidden_kernel(const T* __restrict__ h, T* __restrict__ out, int B,
                                                              int L, int D) {
    const int nchunk = D >> 3;
    const int64_t total = (int64_t)2 * B * L * nchunk;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % nchunk);
        const int64_t row = i / nchunk;
        const int s = (int)(row / L), t = (int)(row - (int64_t)s * L);
        float v[8];
        load8<T>(h + row * D + c * 8, v);
        if (s < B) {
            store8<T>(out + ((int64_t)s * L + t) * 2 * D + c * 8, v);
        } else {
            float rv[8];
#pragma unroll
            for (int k = 0; k < 8; ++k) rv[k] = v[7 - k];
            store8<T>(out + ((int64_t)(s - B) * L + (L - 1 - t)) * 2 * D + D + (D - 8 - c * 8), rv);
        }
    }
}

hipError_t launch_assemble_hidden(const void* h, void* out, int B, int L, int D, int dt, hipStream_t s) {
    if (B * L == 0) return hipSuccess;
    const int64_t total = (int64_t)2 * B * L * (D >> 3);
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    if (dt == BF16)
        hipLaunchKernelGGL(assemble_hidden_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, (const bf16_t*)h, (bf16_t*)out,
                           B, L, D);
    else
        hipLaunchKernelGGL(assemble_hidden_kernel<float>, dim3(grid), dim3(256), 0, s, (const float*)h, (float*)out, B,
                           L, D);
    return hipGetLastError();
}

template <typename T>
__global__ __launch_bounds__(256) void embed_only_kernel(const int32_t* __restrict__ ids, const T* __restrict__ emb,
                                                         const int32_t* __restrict__ comp8, T* __restrict__ h, int B,
                                                         int L, int D) {
    const int nchunk = D >> 3;
    const int64_t total = (int64_t)2 * B * L * nchunk;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < total;
         i += (int64_t)gridDim.x * blockDim.x) {
        const int c = (int)(i % nchunk);
        const int64_t row = i / nchunk;
        const int s = (int)(row / L), t = (int)(row - (int64_t)s * L);
        int tok;
        if (s < B) tok = ids[(int64_t)s * L + t];
        else tok = comp8[ids[(int64_t)(s - B) * L + (L - 1 - t)] & 7];
        float v[8];
        load8<T>(emb + (int64_t)(tok & 7) * D + c * 8, v);
        store8<T>(h + row * D + c * 8, v);
    }
}

hipError_t launch_embed_only(const int32_t* ids, const void* emb, const int32_t* comp8, void* h, int B, int L, int D,
                             int dt, hipStream_t s) {
    if (B * L == 0) return hipSuccess;
    const int64_t total = (int64_t)2 * B * L * (D >> 3);
    const unsigned grid = (unsigned)((total + 255) / 256 > 8192 ? 8192 : (total + 255) / 256);
    if (dt == BF16)
        hipLaunchKernelGGL(embed_only_kernel<bf16_t>, dim3(grid), dim3(256), 0, s, ids, (const bf16_t*)emb, comp8,
                           (bf16_t*)h, B, L, D);
    else
        hipLaunchKernelGGL(embed_only_kernel<float>, dim3(grid), dim3(256), 0, s, ids, (const float*)emb, comp8,
                           (float*)h, B, L, D);
    return hipGetLastError();
}

}  // namespace pcad
