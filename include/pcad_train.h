/* pcad_train.h - C ABI of libpcad_train.so: the backward operators of the MI355X engine's kernels (training support).
 *
 * A library of its own beside libpcad.so (include/pcad.h), whose exported symbol set is the inference ABI and stays as it is: a
 * program that only runs the model neither loads nor sees these entries.  libpcad_train.so links libpcad.so (same directory) and
 * shares its conventions: status codes (pcad_status), dtypes (pcad_dtype), pcad_stream, and the calling thread's pcad_last_error()
 * text.  Built by the same Makefile from csrc/train_api.hip and csrc/scan_bwd.hip. */
#ifndef PCAD_TRAIN_H
#define PCAD_TRAIN_H
#include "pcad.h"

#ifdef __cplusplus
extern "C" {
#endif

/* Backward of pcad_selective_scan (accumulate 0), one direction.  Replaces: the backward of `selective_scan_fn` (mamba-ssm 2.2.2
 * `SelectiveScanFn.backward`).  Walk step s = 0..L-1 visits row t = s (reverse: t = L-1-s); per strand and channel c, state n < 16:
 *   d_t    = softplus(delta_t + bias_c)   (v > 20: v)
 *   a_s[n] = exp(d_t A[c,n]);  h_s[n] = a_s[n] h_{s-1}[n] + d_t u_t B_t[n];  h_{-1} = 0
 *   y_t    = sum_n h_s[n] C_t[n] + D_c u_t;   out_t = y_t silu(z_t)  (z NULL: y_t)
 * and with g = dL/dout:
 *   dy_t   = g_t silu(z_t)  (z NULL: g_t)
 *   dz_t   = g_t y_t sig(z_t) (1 + z_t (1 - sig(z_t)))                      (y_t recomputed, unrounded)
 *   k_s[n] = dy_t C_t[n] + a_{s+1}[n] k_{s+1}[n],  k_L = 0                  (walked from s = L-1 down to 0)
 *   dC_t[n] = sum_c dy_t h_s[n]          dB_t[n] = sum_c k_s[n] d_t u_t      (sums over the E channels of the strand)
 *   du_t   = dy_t D_c + d_t sum_n k_s[n] B_t[n]
 *   dd_t   = sum_n k_s[n] (A[c,n] a_s[n] h_{s-1}[n] + u_t B_t[n])
 *   ddelta_t = dd_t sig(delta_t + bias_c)                                   (1 where delta_t + bias_c > 20)
 *   dA[c,n] = sum_{strand,s} k_s[n] d_t a_s[n] h_{s-1}[n]     dD_c = sum_{strand,t} dy_t u_t     dbias_c = sum_{strand,t} ddelta_t
 * All products and sums are fp32; the only roundings are the stores of du, ddelta and dz in the model dtype.  No floating-point
 * atomics: every sum has a fixed order and a call's results are bit-reproducible.
 *   inputs     exactly pcad_selective_scan's: u, delta [S, L, E] dtype; z [S, L, ldz >= E] dtype or NULL; bc fp32 [S*L, 32] = B_t | C_t
 *              (16-byte aligned); A fp32 [E, 16] raw; Dskip, delta_bias fp32 [E]; E % 64 == 0
 *   dout, du, ddelta  [S, L, E] dtype;  dz [S, L, E] dtype, required exactly when z is given
 *   dbc        fp32 [S*L, 32] = dB_t | dC_t (16-byte aligned);  dA fp32 [E, 16];  dD, ddelta_bias fp32 [E]
 *              every output is overwritten, not accumulated
 *   scratch    pcad_selective_scan_bwd_scratch_bytes(S, L, E) bytes, 256-byte aligned (too small / misaligned: PCAD_ERR_WORKSPACE): the
 *              states at the chunk boundaries (the forward saves none; they are recomputed) and the partial sums
 * PCAD_ERR_INVALID names the argument (message via pcad_last_error of libpcad.so, which this library links): a null tensor, E % 64 != 0, a bad dtype, misaligned bc / dbc, dz without z or z without dz.
 * S == 0 or L == 0: OK, nothing is done.  No allocation, no synchronisation; all work goes on `stream`. */
size_t pcad_selective_scan_bwd_scratch_bytes(int S, int L, int E);
int pcad_selective_scan_bwd(const void* u, const void* delta, const void* z, int64_t ldz, const float* bc,
                            const float* A, const float* Dskip, const float* delta_bias, const void* dout,
                            void* du, void* ddelta, void* dz, float* dbc, float* dA, float* dD, float* ddelta_bias,
                            void* scratch, size_t scratch_bytes, int S, int L, int E, int reverse, int dtype, pcad_stream stream);

#ifdef __cplusplus
}
#endif
#endif /* PCAD_TRAIN_H */
