// Host-side launcher declarations (one per kernel family). All launch on the given stream; no sync.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <stdlib.h>

namespace pcad {

enum DType { F32 = 0, BF16 = 1 };

// Developer A/B switches are environment variables that are honoured ONLY when PCAD_DEV=1 is also set; a production
// process never changes behaviour because of a stray variable.  (Numerics / sizing options of the ABI: pcad_set_option.)
inline const char* dev_env(const char* name) {
    static const bool dev = [] { const char* d = getenv("PCAD_DEV"); return d && d[0] == '1'; }();
    return dev ? getenv(name) : nullptr;
}

// Per-device launch state.  A handle is bound to the device that was current when it was created and several handles on several
// devices may live in one process (include/pcad.h "Threading / streams"), so nothing about a device is cached process-wide:
// the CU count and the "this kernel may use > 64 KiB of dynamic LDS" attribute are kept per (device ordinal[, kernel]).
hipError_t ensure_dynamic_lds(const void* kernel, int bytes);   // hipFuncSetAttribute once per (current device, kernel)
int device_cu_count();                                          // multiProcessorCount of the current device (256 on MI355X)

struct Positions {            // by-value kernel argument: the positions evaluated by the head kernel
    int n;                    // 0 => all L positions
    int p[16];
};

// norm.hip --------------------------------------------------------------------------------------
// The norm and head launchers take a plain struct of named fields (defaults in place) and the stream, like the mixer launchers below.
// fused residual add + RMSNorm (rms_norm_fn prenorm=True).
struct NormLaunch {
    const void* x = nullptr;          // [rows, D], dtype dt (launch_embed_rmsnorm: unused, the rows are gathered from EmbedRows::emb)
    const void* res_in = nullptr;     // [rows, D], dtype rdt, or nullptr (launch_embed_rmsnorm: unused)
    const float* w;                   // norm weight [D]
    void* y;                          // [rows, D], dtype dt
    void* res_out;                    // [rows, D], dtype rdt, or nullptr
    int64_t rows = 0;                 // (launch_embed_rmsnorm: unused, 2 B L)
    int D;  float eps;  int dt, rdt;
    bool split_y = false;             // (dt == rdt == F32 only): y is written as a bf16 tensor [rows, 2 D] = [hi | lo] (pack.hip launch_split_rows' format)
    // launch_embed_rmsnorm only.  rstd_out != nullptr: the norm-folded form - y (may be nullptr) = the un-normalised embedding row,
    // rstd_out[row] = its rstd, and res_out (fp32) is written in the 4-wave GEMM's fragment layout (common.hpp res_frag_off;
    // 2 B L % 256 == 0) as a tensor of Dp = round_up(D, 256) columns whose padding columns are zeroed; y rows are Dp elements apart.
    float* rstd_out = nullptr;
    int Dp = 0;                       // padded width of res / y rows (0: D)
};
hipError_t launch_add_rmsnorm(const NormLaunch& n, hipStream_t s);
// layer-0 variant: x = Emb[strand token] gathered on the fly (RCPS strands by index arithmetic), rows = 2 B L.
struct EmbedRows { const int32_t* ids;  const void* emb;  const int32_t* comp8;  int B, L; };     // ids [B, L], emb [8, D] (dtype dt)
hipError_t launch_embed_rmsnorm(const NormLaunch& n, const EmbedRows& e, hipStream_t s);
// rstd[row] = rsqrt(sum of the np partial sums of squares of the row / D + eps)
hipError_t launch_rstd(const float* ssq, float* rstd, int64_t rows, int np, int D, float eps, hipStream_t s);

// What every head (final / pooled / loss / probs) reads: the last mixer output, the residual stream and norm_f.
struct HeadInput {
    const void* h;                    // mixer output [2B * L, D], dtype dt (final / probs with h_compact: the evaluated rows only)
    const void* res;                  // residual stream, always the full tensor [2B * L, D], dtype rdt
    const float* w;                   // norm_f weight [D]
    int B, L, D;  float eps;  int dt, rdt;
    int res_frag = 0;                 // != 0: fp32 residual in the GEMM's fragment layout (common.hpp res_frag_off) of that (padded) width
    const int32_t* ids = nullptr;     // [B, L] + status (device word): token ids outside [0, 8) set status bit 1
    int32_t* status = nullptr;
};
// the heads' shared preconditions: the width the row kernels cover, a dtype pair they exist for, the fragment layout's shape
inline hipError_t head_input_check(const HeadInput& in) {
    if (in.D % 8 || in.D > 2048) return hipErrorInvalidValue;
    if ((in.dt != BF16 && in.dt != F32) || (in.rdt != F32 && in.rdt != in.dt)) return hipErrorInvalidValue;
    if (in.res_frag && (in.rdt != F32 || in.res_frag % 256 || in.res_frag < in.D || ((int64_t)2 * in.B * in.L) % 256)) return hipErrorInvalidValue;
    return hipSuccess;
}
// final add + norm_f + RC re-assembly + tied RCPS LM head, only at the requested positions.  Per-window positions outside [0, L)
// are clamped and set bit 2 of in.status.
struct FinalHeadLaunch {
    HeadInput in;
    const float* emb_f32;  const int32_t* comp8;      // the tied embedding [8, D] in fp32, the complement map [8]
    void* hidden_out = nullptr;       // [B, Q, 2D], dtype dt, or nullptr
    float* logits_out = nullptr;      // [B, Q, 8], or nullptr
    Positions pos = {};               // the shared list (n == 0: all L positions)
    const int32_t* pos_per_seq = nullptr;     // device [B]: one position per window instead (pos.n == 0)
    bool h_compact = false;           // (shared list only): in.h holds only the evaluated rows, [(strand * P + q), D] as launch_gather_rows orders them
};
hipError_t launch_final_head(const FinalHeadLaunch& a, hipStream_t s);
// pool.hip: pooled sequence-classification head (pcad.h pcad_pooled_head).  pooling: POOL_* (= pcad.h pcad_pooling).  Stage 1 writes
// pool_partial_bytes(B, L, D, pooling) bytes of fp32 partials to `part` (256-byte aligned); the segmentation depends on L only.
enum { POOL_MEAN = 0, POOL_MAX = 1, POOL_FIRST = 2, POOL_LAST = 3 };
int pool_segments(int L, int pooling);
size_t pool_partial_bytes(int B, int L, int D, int pooling);
struct PooledHeadLaunch {
    HeadInput in;
    const float* score_w = nullptr;  int NL = 0;      // score head [NL, D], 1 <= NL <= 256 (needed for logits_out)
    float* pooled_out = nullptr;      // [B, 2D] fp32, or nullptr
    float* logits_out = nullptr;      // [B, NL], or nullptr
    int pooling;
    void* part;                       // the stage-1 partials
};
hipError_t launch_pooled_head(const PooledHeadLaunch& a, hipStream_t s);
// loss.hip: masked-LM loss head (pcad.h pcad_loss_head): launch_final_head's logits at every position + the cross entropy of the
// labelled ones, reduced per window.  Stage 1 writes loss_partial_bytes(B, L) bytes of fp32 partials to `part` (16-byte aligned);
// the segmentation depends on L only.
constexpr int LOSS_SEG = 64;          // positions per stage-1 segment (and per block of loss_bwd.hip)
int loss_segments(int L);
size_t loss_partial_bytes(int B, int L);
struct LossHeadLaunch {
    HeadInput in;
    const float* emb_f32;  const int32_t* comp8;
    const int32_t* labels;            // [B, L]; ignored: == ignore_index or < 0; other values outside [0, 8) set status bit 4
    const float* loss_w = nullptr;    // [B, L], or nullptr (all 1)
    int ignore_index;
    float* sums_out;                  // [B, 4] = { sum w nll, sum w, labelled, arg-max hits }
    float* nll_out = nullptr;         // [B, L], or nullptr
    float* logits_out = nullptr;      // [B, L, 8], or nullptr
    void* part;                       // the stage-1 partials
};
hipError_t launch_loss_head(const LossHeadLaunch& a, hipStream_t s);
// probs.hip: nucleotide-probability head (pcad.h pcad_probs_head): launch_final_head's logits at the evaluated positions + the fp32
// softmax over the four vocabulary columns `cols`.
struct ProbCols { int c[4]; };        // by-value kernel argument
struct ProbsHeadLaunch {
    HeadInput in;
    const float* emb_f32;  const int32_t* comp8;
    ProbCols cols;
    float* probs_out = nullptr;       // [B, Q, 4] (16-byte aligned), or nullptr
    float* logits_out = nullptr;      // [B, Q, 8], or nullptr
    Positions pos = {};               // the shared list (n == 0: all L positions, or the per-window list)
    const int32_t* pos_per_window = nullptr;  int Pw = 0;     // device [B, Pw], 1 <= Pw <= 16, pos.n == 0; values outside [0, L) are clamped and set status bit 2
    bool h_compact = false;           // (shared list only): in.h holds only the evaluated rows
};
hipError_t launch_probs_head(const ProbsHeadLaunch& a, hipStream_t s);
// layers.hip: one level of hidden_states at the evaluated positions only (pcad.h pcad_layer_rows).
struct LayerRowsLaunch {
    const void* src;                  // plain rows [2B * L, D] (a mixer output h / the RCPS embedding), or see assembled / compact
    // model dtype [B, P, 2D] = launch_assemble_hidden's rows (b, p_q), or - average - fp32 [B, P, D] = (fwd + rc) * 0.5 in straight channel order
    void* out;
    int B, L, D, dt;
    Positions pos = {};               // the shared list (pos.n == P), unless pos_per_window or assembled
    const int32_t* pos_per_window = nullptr;  // device [B, P]; values outside [0, L) are clamped and set status bit 2
    int P;
    // src holds rows of 2D elements already in the reference's layout (final_head_kernel's hidden_out; positions are not read):
    bool assembled = false;
    int64_t sb = 0;                   // (assembled) rows between two windows' slot 0: the row of (window b, slot q) is b * sb + q * sq
    int64_t sq = 0;                   // (assembled) rows between two slots of a window
    bool average = false;
    bool compact = false;             // (shared list, not assembled): src = launch_gather_rows' [2B, P, D] rows of h
    int32_t* status = nullptr;
};
hipError_t launch_layer_rows(const LayerRowsLaunch& a, hipStream_t s);
// token ids outside [0, 8) among ids[0, n) (any 4-byte alignment) set status bit 1, as the heads' own check does; status == nullptr: no launch
hipError_t launch_ids_check(const int32_t* ids, int64_t n, int32_t* status, hipStream_t s);
// dst [P, B] = the columns of src [B, P] (device int32): slot q's positions of every window as one contiguous list
hipError_t launch_position_columns(const int32_t* src, int32_t* dst, int B, int P, hipStream_t s);
// hidden_states[i] (block input = previous mixer output / embedding) assembled in RCPS layout.
hipError_t launch_assemble_hidden(const void* h, void* out, int B, int L, int D, int dt, hipStream_t s);
hipError_t launch_embed_only(const int32_t* ids, const void* emb, const int32_t* comp8, void* h, int B, int L,
                             int D, int dt, hipStream_t s);
// a[i] = round_dt(a[i] + b[i]), n % 8 == 0: the sum of the two directions' out_proj outputs (strict reference order only)
hipError_t launch_add_round(void* a, const void* b, int64_t n, int dt, hipStream_t s);

// gemm.hip --------------------------------------------------------------------------------------
// C[M,N] = A[M,K] W[N,K]^T in four forms that share their operands (GemmOperands) and differ in where the result goes (Gemm*Out).
// Every option is a named field whose default is its initialiser; the stream is the launchers' last parameter.
struct GemmOperands {
    const void* A;  int64_t lda;      // [M, K]; lda / ldw multiples of 16 bytes
    const void* W;  int64_t ldw;      // [N, K]
    int64_t M;  int N, K;             // K a multiple of 128 bytes
    int dt;
    bool a_blocked = false;           // A is in the blocked layout with rows of lda elements (not the `two` form)
    // ksplit != 0 (dt == BF16, fp32 result only; plain and `two` forms): the wrap-around K cursor of the split-bf16 GEMMs (api.hip
    // "f32_gemm_split") - both operands are bf16 [hi | lo] tensors of 2 Ko columns, K = 3 Ko, ksplit = Ko / 64 (K-tiles per part): the
    // cursor reads A as hi, lo, hi and W as hi, hi, lo, i.e. C = a_hi w_hi + a_lo w_hi + a_hi w_lo accumulated in fp32 in that order.
    int ksplit = 0;
};
struct GemmPlainOut {
    void* C;  int64_t ldc;
    int out_dt;                       // F32 or == dt
    bool round_bf16 = false;          // round the fp32 result to bf16 precision before an F32 store
};
// x_proj form: columns [0, nsplit) -> C (dtype dt, ld ldc); columns [nsplit, N) -> C2 (fp32, rounded to dt's
// precision, ld ldc2).  nsplit % 16 == 0.
struct GemmSplitOut { void* C;  int64_t ldc;  float* C2;  int64_t ldc2;  int nsplit; };
// in_proj form on the 256x256 kernel: columns [0, nsplit) -> C1, [nsplit, N) -> C2 (separate tensors of nsplit and
// N - nsplit columns; both plain or both blocked).
struct GemmTwoOut {
    void *C1, *C2;  int nsplit;
    bool out_blocked = false;
    const float* rscale = nullptr;    // per-row factor [M] applied to the result before it is rounded (the norm-folded in_proj: rstd of the row)
    // -1 = dt; F32 with dt == BF16: bf16 operands, fp32 outputs (no rscale) - the split-bf16 in_proj of the fp32 model, with
    // ksplit = Ko / 64 and [hi | lo] operands
    int out_dt = -1;
};
// out_proj of the norm-folded layer form, on the 4-wave kernel only (gemm_fold_shapes_ok):
//   res [M, N] fp32 (FRAGMENT layout, common.hpp res_frag_off) += A . W^T (in place);  C [M, N] (plain rows, dtype dt; unused for
//   fp32: see api.hip) = round(res);  ssq [M, N / 128] = per-row partial
//   sums of squares of the updated residual, one per 128-column wave tile (deterministic; reduced by launch_rstd).
struct GemmResOut { void* C;  float* res;  float* ssq; };
hipError_t launch_gemm_nt(const GemmOperands& g, const GemmPlainOut& o, hipStream_t s);
hipError_t launch_gemm_nt_split(const GemmOperands& g, const GemmSplitOut& o, hipStream_t s);
hipError_t launch_gemm_nt_two(const GemmOperands& g, const GemmTwoOut& o, hipStream_t s);
hipError_t launch_gemm_nt_res(const GemmOperands& g, const GemmResOut& o, hipStream_t s);
// whether a chunk of M token-rows of a (D, E) model can run the folded form (whole 256 x 256 tiles for both projections)
bool gemm_fold_shapes_ok(int64_t M, int D, int E, int dt);
inline int fold_padded_width(int D) { return (D + 255) / 256 * 256; }     // width of res / u in the folded form (l20: 384 -> 512)

// conv.hip --------------------------------------------------------------------------------------
// y[t] = silu(b + sum_k w[k] x[t-3+k]) (fwd: causal) or silu(b + sum_k w[k] x[t+3-k]) (rev: anti-causal).
struct ConvDirection { const float* w;  const float* b;  void* y; };        // taps [E, 4], bias [E], output (nullptr in launch_conv_bidir: not written)
struct ConvLaunch {
    const void* x;  int64_t ldx;      // plain rows of ldx elements (a multiple of 16 bytes), 16-byte aligned
    ConvDirection fwd, rev;
    int64_t ldy = 0;                  // launch_conv_dir: elements between plain output rows (launch_conv_bidir writes rows of E)
    int S, L, E, dt;                  // E * elem a multiple of 16 bytes (blocked: of 128)
    bool in_blocked = false;          // x is a [S*L, E] tensor in the blocked layout (ldx ignored)
    bool out_blocked = false;         // y in the blocked layout (common.hpp::blocked_off; ldy ignored), buffers padded to a multiple of 8 rows
};
hipError_t launch_conv_bidir(const ConvLaunch& c, hipStream_t s);       // both directions from one read of x
// One direction ("untied_directions": each direction has its own x): c.rev if `reverse`, else c.fwd (refused if that side's w, b or
// y is null; the other side is not read) - the same arithmetic order per output as launch_conv_bidir.
hipError_t launch_conv_dir(const ConvLaunch& c, bool reverse, hipStream_t s);

// convx.hip -------------------------------------------------------------------------------------
// Fused conv1d+SiLU (both directions) + x_proj (both directions), Rp == 64 or 96: x [S*L, E] blocked -> xc0 / xc1 [S*L, E]
// blocked, dtl_d [S*L, Rp] (dtype dt), bc_d [S*L, 32] fp32; Wx_d [Rp + 32, E].  convw: taps packed by launch_pack_convw.
size_t convx_packed_bytes(int E, int dt);
hipError_t launch_pack_convw(const float* wf, const float* bf, const float* wr, const float* br, float* out, int E, int dt,
                             hipStream_t s);
struct ConvxDirection { const void* Wx;  void* xc;  void* dtl;  float* bc; };
struct ConvxLaunch {
    const void* x;  const float* convw;
    ConvxDirection dir[2];            // 0: forward (causal), 1: reverse
    int S, L, E, dt;
    int Rp = 64;
    bool dtl_split = false;           // (dt == F32): dtl_d is written as bf16 [S*L, 2 Rp] = [hi | lo]
    bool w_split = false;             // (dt == F32): Wx_d is the bf16 [Rp + 32, 2E] copy of launch_pack_convx_wsplit and
                                      // x_proj runs as three bf16 MFMA products per fp32 product
    float* part_ws = nullptr;         // scratch of convx_split_bytes(): small launches split the channel walk over several
                                      // blocks per row tile (convx_ksplit) and a second tiny kernel adds their partial x_dbl
    int policy_S = 0;                 // strands the K-split policy is evaluated for (0: S; see scan_segment_bytes)
};
hipError_t launch_convx(const ConvxLaunch& c, hipStream_t s);
int convx_ksplit(int S, int L, int E, int dt);        // K-split factor for this launch shape (1: none)
size_t convx_split_bytes(int S, int L, int E, int dt, int Rp, int policy_S = 0);
hipError_t launch_pack_convx_wsplit(const float* src, int64_t ld, void* dst, int rows, int E, hipStream_t s);
// dt_rank padded to the K granule of the fused kernels: 64 up to dt_rank 64 (every PlantCaduceus size), else the next multiple of 32
// (PlantCAD2 Large: dt_rank 96 -> 96)
inline int padded_dt_rank(int R) { return R <= 64 ? 64 : (R + 31) / 32 * 32; }

// scan.hip --------------------------------------------------------------------------------------
// One direction's operands.  bc: fp32 [rows, 32] = B_t | C_t.  dt_low [rows, lddt] / Wdt [E, Rp]: the fused dt_proj's operands (null in
// launch_scan's unfused form, which reads delta from memory).
struct ScanDirection { const void *u, *dt_low, *Wdt; const float *bc, *A2, *Dskip, *dbias; };
// Selective scan of one direction.
struct ScanLaunch {
    ScanDirection dir;
    // delta == nullptr: fused dt_proj (delta tile = dt_low[rows, Rp] . Wdt[E, Rp]^T on MFMA inside the kernel, Rp % 32 == 0,
    // zero-padded K);  delta != nullptr: delta [rows, E] read from memory (lddt / Rp unused).
    const void* delta = nullptr;
    const void* z = nullptr;  int64_t ldz = 0;      // the gate (nullptr: ungated output); rows of ldz elements
    int64_t lddt = 0;  int Rp = 0;
    float a_scale = 1.0f;             // the recurrence uses A2 * a_scale as the base-2 decay rate: pass (A * log2(e), 1) or (A, log2(e))
    void* y;
    int S, L, E, dt;
    bool reverse = false;
    int accumulate = 0;               // 1: y += after the gate, each direction rounded; 2 (needs z): (y_prev + y) * silu(z), gated once
    bool uy_blocked = false;          // u and y are in the blocked layout (whole-tensor row index s*L + t, buffers padded to 8 rows)
    bool z_blocked = false;           // (needs uy_blocked): z is a separate [S*L, E] tensor in the same blocked layout (ldz ignored)
    // seg_ws (fused dt_proj form only): scratch of scan_segment_bytes(S, L, E) bytes; when given and scan_segments() > 1 the walk of
    // every strand is cut into segments that run as separate workgroups (long sequences with few strands: PlantCAD2's 8 192-bp windows).
    float* seg_ws = nullptr;
    // walk_len (0 or >= L: the whole strand): only the first walk_len steps of the walk are run (forward: rows [0, walk_len); reverse:
    // rows [L - walk_len, L)); the other rows of y are not written.  Ignored when the walk is cut into segments.
    int walk_len = 0;
    // ysplit (fp32 engine layouts only: dt == F32, fused dt_proj, blocked u / y / z, L % 8 == 0; reverse gating launch, unsegmented, whole
    // walk): the output is written NOT to y but as out_proj's split-bf16 operand, bf16 [rows8, 2E] blocked = [hi | lo] (pack.hip).
    void* ysplit = nullptr;
    // dt_split (dt == F32, fused dt_proj): dt_low is bf16 [rows, lddt >= 2 Rp] = [hi | lo] and Wdt bf16 [E, 2 Rp] = [hi | lo] (Rp = the padded
    // dt_rank, <= 96): the fp32 model's dt_proj as three bf16 MFMA products per fp32 product ("f32_gemm_split"; K walk hi.hi, lo.hi, hi.lo).
    bool dt_split = false;
    int policy_S = 0;                 // strands the segment policy is evaluated for (0: S; see scan_segment_bytes)
};
hipError_t launch_scan(const ScanLaunch& a, hipStream_t s);

// Segments per strand for the scan of S strands of L steps over E channels.  Pass A + pass B cost ~1.8x the arithmetic of one
// walk, and a single wave per SIMD already keeps the VALU ~65 % busy, so cutting only pays when most SIMDs would otherwise idle
// (measured: 1 536 waves at L = 8 192 are 15 % FASTER uncut).  Cut when the launch has at most 768 waves (0.75 per SIMD): into
// enough segments for ~2 300 waves, at most 8 (16 for short strands); long strands (L >= 2 048) into segments of at least 512 steps (16 blocks of 32),
// short ones (the reference's 512-bp windows in batches of at most 8 at l32: notebooks/examples.ipynb:141-170 runs B = 1) into
// segments of at least 64 steps when the launch has at most 512 waves, where the chip is so empty that two 64-step passes beat one
// 512-step walk (profiles/r04j_small_batch.txt, seq/s without -> with: l32 B = 1 61 -> 107, B = 8 455 -> 548; l20 B = 1 119 -> 257,
// B = 8 929 -> 1682; at 768 waves - l20 B = 32 - it loses 13 %, hence the lower bound for short strands).  Round 5: short strands into up
// to 16 segments of at least 32 steps (one delta tile): l32 B = 1 107 -> 118 seq/s, l20 B = 1 / 2 / 4 243 / 474 / 918 -> 283 / 546 / 996,
// B >= 8 unchanged (profiles/r05g_small_batch.txt, same box).
inline int scan_segments(int S, int L, int E, int* seg_blocks) {
    const int64_t waves = (int64_t)S * (E / 64);
    const int nblk = (L + 31) / 32;
    const int min_blocks = L >= 2048 ? 16 : 1;
    int G = 1;
    if (L >= 256 && waves > 0 && waves <= (L >= 2048 ? 768 : 512)) {
        G = (int)((2304 + waves - 1) / waves);
        if (G > (L >= 2048 ? 8 : 16)) G = L >= 2048 ? 8 : 16;
        if (G > nblk / min_blocks) G = nblk / min_blocks;
        if (G < 3) G = 1;                              // below ~3x the waves the second pass is not paid for
    }
    const int sb = (nblk + G - 1) / G;
    G = (nblk + sb - 1) / sb;                          // no empty segment
    if (seg_blocks) *seg_blocks = sb;
    return G;
}
// policy_S (here and in ScanLaunch / ConvxLaunch; 0: S): the strand count the small-launch policy is evaluated for.  The engine
// passes the strands of the WHOLE pcad_forward batch, so that every chunk of a call runs the same form and results do not depend on
// how the batch was cut into chunks, bit for bit; the scratch is sized for the S strands of the launch.
inline size_t scan_segment_bytes(int S, int L, int E, int policy_S = 0) {
    const int G = scan_segments(policy_S > 0 ? policy_S : S, L, E, nullptr);
    return G > 1 ? (size_t)S * G * E * 17 * sizeof(float) : 0;        // [S][G][E][16] states + [S][G][E] delta sums
}

// "Pair" walks (launches with few waves - PlantCAD2's 8 192-bp windows in batches of a few dozen, 512-bp windows in batches of a few
// dozen: at most 3.5 waves per SIMD; at 2 the VALU idles a third of the time): both directions of the layer in ONE launch, each
// walking half of its strand per launch - launch 1: forward rows [0, L/2) and reverse rows [L/2, L) from zero states, outputs ungated
// (or each gated, "gate_each"), end states kept; launch 2: the second halves from those states, each adding what the OTHER direction's
// first launch left in y and gating.  Twice the waves per launch, the same arithmetic, no extra pass.  Against the plain two-launch
// form the bf16 model's gate-once sum is rounded at the other direction's partial on half of the rows (y_rev stored, y_fwd added in
// fp32, instead of the reverse): results of a pair walk and of a plain walk agree to bf16 rounding of one addend (fp32 model: to fp32
// summation order), exactly as the segmented form does - and the form is chosen like it: from the strands of the whole pcad_forward
// call, governed by "scan_segments".
inline bool scan_pair_wanted(int S, int L, int E) {
    const int64_t waves = (int64_t)S * (E / 64);
    static const int64_t max_waves = [] { const char* v = dev_env("PCAD_PAIR_MAX_WAVES"); return v ? (int64_t)atoll(v) : (int64_t)3584; }();   // PCAD_DEV=1 A/B knob
    return L % 64 == 0 && L >= 128 && waves > 0 && waves <= max_waves && scan_segments(S, L, E, nullptr) == 1;
}
inline size_t scan_pair_bytes(int S, int E) { return (size_t)2 * S * 2 * E * 16 * sizeof(float); }     // [dir][S][2][E][16] states
// u / y / z blocked [S*L (8-row padded), E]; dt_low [S*L, lddt]; Wdt [E, Rp] (dt_split: bf16 [hi | lo] operands as in ScanLaunch);
// A2 pre-scaled by log2(e).
struct ScanPairLaunch {
    ScanDirection fwd, rev;
    const void* z;
    int64_t lddt;  int Rp;
    void* y;
    int S, L, E, dt;
    bool gate_each = false;           // each direction gated and rounded (default: the sum of both gated once)
    float* ws;                        // scan_pair_bytes(S, E)
    void* ysplit = nullptr;           // (fp32 + f32_gemm_split): the gated output as out_proj's [hi | lo] operand
    bool dt_split = false;
    int phases = 3;                   // bit 0: the first-half launch, bit 1: the second-half launch
};
hipError_t launch_scan_pair(const ScanPairLaunch& a, hipStream_t s);

// scan_bwd.hip ----------------------------------------------------------------------------------
// Backward of launch_scan's unfused plain-layout form (pcad_train.h pcad_selective_scan_bwd): inputs as ScanLaunch takes them there (A raw,
// not scaled), dout / du / ddelta / dz [S, L, E] in dtype dt (dz exactly when z is given), dbc fp32 [S L, 32] = dB_t | dC_t, dA fp32
// [E, 16], dD / ddbias fp32 [E]; every output is overwritten.  scratch: scan_bwd_bytes(S, L, E) bytes, 256-byte aligned - the states
// at the chunk boundaries and the partial sums a second kernel adds in index order (no floating-point atomics).
constexpr int SCAN_BWD_CHUNK = 8;     // walk steps between two stored states = steps whose states one lane keeps in registers
struct ScanBwdLaunch {
    const void *u, *delta;
    const void* z = nullptr;  int64_t ldz = 0;
    const float *bc, *A, *Dskip, *dbias;
    const void* dout;
    void *du, *ddelta;
    void* dz = nullptr;
    float *dbc, *dA, *dD, *ddbias;
    void* scratch;
    int S, L, E, dt;
    bool reverse = false;
};
size_t scan_bwd_bytes(int S, int L, int E);
hipError_t launch_scan_bwd(const ScanBwdLaunch& a, hipStream_t s);

// scan_bwd_seg.hip (libpcad_bwd.so, pcad_bwd.h pcad_selective_scan_bwd_seg): the same operator with every strand cut into
// up to `segments` segments of scan_bwd_seg_steps(L, segments) walk steps (a multiple of SCAN_BWD_CHUNK; 0: L < 1 or segments outside
// [1, SCAN_BWD_MAX_SEGMENTS]), one wave per (strand, segment, 64 channels).  scratch: scan_bwd_seg_bytes(S, L, E, segments) bytes.
constexpr int SCAN_BWD_MAX_SEGMENTS = 64;
int scan_bwd_seg_steps(int L, int segments);
size_t scan_bwd_seg_bytes(int S, int L, int E, int segments);
hipError_t launch_scan_bwd_seg(const ScanBwdLaunch& a, int segments, hipStream_t s);

// scan_fwd_seg.hip (libpcad_bwd.so, pcad_bwd.h pcad_selective_scan_fwd_seg): the FORWARD of launch_scan's unfused plain-layout
// form (explicit delta, A raw) cut by the same rule, scan_bwd_seg_steps, one wave per (strand, segment, 64 channels); y [S, L, E] in dtype
// dt is overwritten.  scratch: scan_fwd_seg_bytes(S, L, E, segments) bytes.  scan_fwd_seg_grid_ok: whether its grids fit 31 bits.
struct ScanFwdSegLaunch {
    const void *u, *delta;
    const void* z = nullptr;  int64_t ldz = 0;
    const float *bc, *A, *Dskip, *dbias;
    void* y;
    void* scratch;
    int S, L, E, dt;
    bool reverse = false;
};
size_t scan_fwd_seg_bytes(int S, int L, int E, int segments);
bool scan_fwd_seg_grid_ok(int S, int L, int E, int segments);
hipError_t launch_scan_fwd_seg(const ScanFwdSegLaunch& a, int segments, hipStream_t s);

// conv_bwd.hip, norm_bwd.hip (libpcad_bwd.so, include/pcad_bwd.h) --------------------
// Both backward kernels keep their parameter-gradient partials in registers, store them once per unit of work to the caller's
// scratch as rows of `n` floats, and launch_sum_partials adds the P rows into out[n]: the rows of each of 32 slices of P in index order, the
// 32 slice sums in index order (a fixed order: no floating-point atomics, results are bit-reproducible).  out0 takes the first n0
// floats of a row, out1 the rest.
hipError_t launch_sum_partials(const float* part, int64_t P, float* out0, int n0, float* out1, int n1, hipStream_t s);

// Backward of launch_conv_dir's plain-layout form (pcad_bwd.h pcad_causal_conv1d_silu_bwd): x [S, L, ldx] and dout / dx [S, L, E] in dtype
// dt, w / dw fp32 [E, 4], b / db fp32 [E]; every output is overwritten.  scratch: conv_bwd_bytes(S, L, E) bytes, 256-byte aligned -
// one row of 5 E partials (dw | db) per (strand, segment of CONV_BWD_SEG walk steps).
constexpr int CONV_BWD_SEG = 64;      // walk steps per lane
struct ConvBwdLaunch {
    const void* x;  int64_t ldx;
    const float *w, *b;
    const void* dout;
    void* dx;
    float *dw, *db;
    void* scratch;
    int S, L, E, dt;
    bool reverse = false;
};
size_t conv_bwd_bytes(int S, int L, int E);
hipError_t launch_conv_bwd(const ConvBwdLaunch& a, hipStream_t s);

// Backward of launch_add_rmsnorm (pcad_bwd.h pcad_add_rmsnorm_bwd): x, dy, dx [rows, D] in dtype dt; res_in, dres_out, dres_in
// [rows, D] in dtype rdt (res_in and dres_in both given or both null; dres_out may be null); w, dw fp32 [D]; every output is
// overwritten.  scratch: norm_bwd_bytes(rows, D) bytes, 256-byte aligned - one row of D partials of dw per slab of NORM_BWD_ROWS rows.
constexpr int NORM_BWD_ROWS = 16;     // consecutive rows one wave walks
struct NormBwdLaunch {
    const void* x;
    const void* res_in = nullptr;
    const float* w;
    const void* dy;
    const void* dres_out = nullptr;
    void* dx;
    void* dres_in = nullptr;
    float* dw;
    void* scratch;
    int64_t rows;  int D;
    float eps;
    int dt, rdt;
};
size_t norm_bwd_bytes(int64_t rows, int D);
hipError_t launch_norm_bwd(const NormBwdLaunch& a, hipStream_t s);

// loss_bwd.hip (libpcad_bwd.so): backward of launch_loss_head on plain rows (pcad_bwd.h pcad_loss_head_bwd).  `in` as
// the forward takes it (res_frag, ids and status unused).  dh [2B * L, D] dtype dt and dres [2B * L, D] dtype rdt: every row is
// written, zeros where the position carries no label; demb fp32 [8, D], dnorm_w fp32 [D]; each output may be null, not all of them.
// scratch (needed for demb / dnorm_w): loss_head_bwd_bytes(B, L, D) bytes, 256-byte aligned - one row of 9 D partials
// (demb | dnorm_w) per (window, segment of LOSS_SEG positions), which launch_sum_partials adds, and one spare row.
struct LossHeadBwdLaunch {
    HeadInput in;
    const float* emb_f32;  const int32_t* comp8;
    const int32_t* labels;            // [B, L], read as launch_loss_head reads them
    const float* loss_w = nullptr;    // [B, L], or nullptr (all 1)
    int ignore_index;
    const float* dsum;                // [B]: the gradient of sums_out[b, 0]
    const float* dnll = nullptr;      // [B, L]: the gradient of nll_out, or nullptr (zero)
    void* dh = nullptr;
    void* dres = nullptr;
    float* dnorm_w = nullptr;
    float* demb = nullptr;
    void* scratch = nullptr;
};
size_t loss_head_bwd_bytes(int B, int L, int D);
hipError_t launch_loss_head_bwd(const LossHeadBwdLaunch& a, hipStream_t s);

// pool_bwd.hip (libpcad_bwd.so): backward of launch_pooled_head on plain rows (pcad_bwd.h pcad_pooled_head_bwd), pooling
// POOL_MEAN / POOL_FIRST / POOL_LAST (POOL_MAX is refused: its gradient needs a tie rule nothing pins).  `in` as the forward takes it
// (res_frag, ids and status unused).  dh [2B * L, D] dtype dt and dres [2B * L, D] dtype rdt: every row is written, zeros where the
// pooling did not read the row; dnorm_w fp32 [D]; dscore_w fp32 [NL, D]; each output may be null, not all of them.
// scratch: pooled_head_bwd_bytes(B, L, D, pooling) bytes, 256-byte aligned - the windows' cotangent rows [B, D], then one partial row of
// dnorm_w per (window, strand, segment of POOL_BWD_SEG rows that carries a gradient), which launch_sum_partials adds.
constexpr int POOL_BWD_SEG = 64;      // rows per block = pool.hip's POOL_SEG: the segmentation depends on L only
struct PooledHeadBwdLaunch {
    HeadInput in;
    const float* score_w = nullptr;  int NL = 0;      // score head [NL, D] fp32 (the dtype-rounded weight), 1 <= NL <= 256
    const float* pooled = nullptr;    // [B, 2, D] fp32: the forward's pooled_out (read for dscore_w only)
    const float* dlogits = nullptr;   // [B, NL] fp32: the gradient of logits_out
    int pooling = POOL_MEAN;
    void* dh = nullptr;
    void* dres = nullptr;
    float* dnorm_w = nullptr;
    float* dscore_w = nullptr;
    void* scratch = nullptr;
};
size_t pooled_head_bwd_bytes(int B, int L, int D, int pooling);
hipError_t launch_pooled_head_bwd(const PooledHeadBwdLaunch& a, hipStream_t s);

// pool_feat.hip (libpcad_bwd.so): the score head on cached pooled vectors (pcad_bwd.h pcad_pooled_logits /
// pcad_pooled_logits_bwd).  The forward restates the logits half of pool.hip's stage 2 (one block of 256 per window), the backward
// pool_bwd.hip's prep kernel without the mean's / L (one block per window for dpooled, one per label for dscore_w).  D % 8 == 0,
// D <= 2048, 1 <= NL <= 256; B == 0: nothing is launched.  No scratch.
struct PooledLogitsLaunch {
    const float* pooled = nullptr;    // [B, 2, D] fp32: launch_pooled_head's pooled_out
    const float* score_w = nullptr;   // [NL, D] fp32 (the dtype-rounded weight)
    float* logits = nullptr;          // [B, NL] fp32
    int B = 0, D = 0, NL = 0;
    int dt = BF16;                    // the model dtype: fixes the rounding points
};
hipError_t launch_pooled_logits(const PooledLogitsLaunch& a, hipStream_t s);
struct PooledLogitsBwdLaunch {
    const float* pooled = nullptr;    // [B, 2, D] fp32 (read for dscore_w only)
    const float* score_w = nullptr;   // [NL, D] fp32 (read for dpooled only)
    const float* dlogits = nullptr;   // [B, NL] fp32
    float* dscore_w = nullptr;        // [NL, D] fp32 or null
    float* dpooled = nullptr;         // [B, 2, D] fp32 or null; not both null
    int B = 0, D = 0, NL = 0;
};
hipError_t launch_pooled_logits_bwd(const PooledLogitsBwdLaunch& a, hipStream_t s);

// optim.hip (libpcad_bwd.so): one AdamW step with global-norm clipping over a table of tensors (pcad_bwd.h pcad_adamw_step) and
// the zeroing of its gradients (pcad_zero_grads).  table: device array of pcad_optim_tensor; map: device int32 [chunks, 2] = (tensor,
// chunk within the tensor), as pcad_optim_plan fills it; one block per chunk of OPTIM_CHUNK elements, chunks never straddle two tensors.
constexpr int OPTIM_CHUNK = 4096;     // elements per chunk = per block of 256 lanes (pcad_bwd.h PCAD_OPTIM_CHUNK)
struct AdamwLaunch {
    const void* table;  const int32_t* map;  int64_t chunks;
    void* state;                      // pcad_optim_state
    float* part;                      // optim_scratch_bytes(chunks): one sum of squares per chunk
    float max_norm, grad_scale;
    float decay, b1, omb1, b2, omb2, step_size, bc2_sqrt, eps;     // 1 - lr wd, beta1, 1 - beta1, beta2, 1 - beta2, lr / bc1, sqrt(bc2), eps
};
size_t optim_scratch_bytes(int64_t chunks);
hipError_t launch_adamw_step(const AdamwLaunch& a, hipStream_t s);
hipError_t launch_zero_grads(const void* table, const int32_t* map, int64_t chunks, hipStream_t s);
// flat[offsets[t] + i] = float(grad_t[i]) over the same chunks (pcad_grads_gather); offsets: device int64 [count], multiples of 4;
// a chunk that would not lie within flat_elems is not written
hipError_t launch_grads_gather(const void* table, const int32_t* map, int64_t chunks, const int64_t* offsets, float* flat, int64_t flat_elems,
                               hipStream_t s);

// wgrad.hip (libpcad_bwd.so): dw[n, k] = (accumulate ? dw[n, k] : 0) + sum_m dy[m, n] x[m, k] with bf16 dy [M, N] / x [M, K]
// and fp32 dw [N, K] (pcad_bwd.h pcad_linear_wgrad) - the one operator here that ADDS to its output.  N, K multiples of 8.
// The rows are cut into slabs by (M, N, K) and these constants alone, never by the device:
//   tiles = ceil(N / WGRAD_BN) ceil(K / WGRAD_BK)     want = clamp(WGRAD_TARGET_BLOCKS / tiles, 1, WGRAD_MAX_SLABS)   (integer division)
//   rows_per_slab = round_up(ceil(M / want), WGRAD_SLAB_ROWS)     slabs = ceil(M / rows_per_slab)                    (M == 0: 0 and 0)
// scratch: wgrad_bytes(M, N, K) = slabs > 1 ? round_up(slabs N K 4, 256) : 0 bytes, 256-byte aligned - one partial [N][K] per slab,
// which a second kernel adds in slab order before the old value is added once.
constexpr int WGRAD_BN = 128, WGRAD_BK = 128;     // the tile of dw one block owns
constexpr int WGRAD_TM = 64;                      // rows of dy / x per LDS stage (two 32-row MFMA steps)
constexpr int WGRAD_TARGET_BLOCKS = 256;          // blocks the split aims for
constexpr int WGRAD_MAX_SLABS = 32;
constexpr int WGRAD_SLAB_ROWS = 256;              // rows_per_slab is a multiple of this
struct LinearWgradLaunch {
    const void* dy;  int64_t lddy;
    const void* x;   int64_t ldx;
    float* dw;       int64_t lddw;
    int64_t M;  int N, K;
    bool accumulate = false;
    void* scratch = nullptr;
};
int64_t wgrad_slabs(int64_t M, int N, int K, int64_t* rows_per_slab);
size_t wgrad_bytes(int64_t M, int N, int K);
hipError_t launch_linear_wgrad(const LinearWgradLaunch& a, hipStream_t s);

// lora.hip (libpcad_bwd.so): the dropout-masked down-projection of a LoRA branch and its backward (pcad_bwd.h
// pcad_lora_down / pcad_lora_down_bwd / pcad_lora_dropout_mask).  The keep mask is a pure function of (seed, stream, row, column):
// one Philox4x32-10 call per 8 consecutive columns of a row, 16 bits per element, keep = (bits >= T).
//   x [M, K] dtype (row stride ldx), A fp32 [r, K], t / u fp32 [M, r], dx [M, K] dtype (row stride lddx), dA fp32 [r, K]
//   K % 8 == 0, 8 <= K <= LORA_MAX_K, r in {4, 8, 16}, 0 <= M < 2^32
// Forward: a wave owns LORA_FWD_ROWS rows and walks their LORA_CHUNK-column chunks in index order; a lane owns 8 consecutive columns
// of a chunk; the r sums of a row are added over the lanes by the xor butterfly (32, 16, ... 1) and scaled by c once.
// Backward: grid (chunks, slabs), a block of 4 waves owns one LORA_CHUNK-column chunk of one row slab; wave w takes the slab's rows
// w, w + 4, ... in index order, the 4 waves' dA sums are added in wave order through LDS and go to scratch [slab][r][K]; a second
// kernel adds the slabs in index order and scales by c once.  The rows are cut into slabs by (M, K) and these constants alone:
//   chunks = ceil(K / LORA_CHUNK)     want = clamp(LORA_TARGET_BLOCKS / chunks, 1, LORA_MAX_SLABS)            (integer division)
//   rows_per_slab = round_up(ceil(M / want), LORA_SLAB_ROWS)     slabs = ceil(M / rows_per_slab)             (M == 0: 0 and 0)
// scratch: lora_down_bwd_bytes(M, K, r) = round_up(slabs r K 4, 256) bytes, 256-byte aligned.
constexpr int LORA_CHUNK = 512;                   // columns a wave covers at once: 64 lanes x 8
constexpr int LORA_FWD_ROWS = 4;                  // rows a wave of the forward walks together
constexpr int LORA_TARGET_BLOCKS = 1024;          // blocks the backward's split aims for
constexpr int LORA_MAX_SLABS = 256;
constexpr int LORA_SLAB_ROWS = 64;                // rows_per_slab is a multiple of this
constexpr int LORA_MAX_K = 8192;
struct LoraMask {
    uint32_t T;                       // drop threshold in [0, 65535]: floor(p 65536 + 0.5)
    float c;                          // keep scale 65536 / (65536 - T), rounded once
    uint32_t seed_lo, seed_hi, stream_lo, stream_hi;
};
LoraMask lora_mask(double p, uint64_t seed, uint64_t stream_id);     // the caller has checked p (lora_threshold(p) <= 65535)
int64_t lora_threshold(double p);     // floor(p 65536 + 0.5), or -1 for a p that is negative or not finite
struct LoraDownLaunch {
    const void* x;  int64_t ldx;
    const float* A;
    float* t;
    int64_t M;  int K, r;
    LoraMask mask;
    int dt;
};
struct LoraDownBwdLaunch {
    const void* x;  int64_t ldx;
    const float* A;
    const float* u;
    void* dx;  int64_t lddx;          // in place on dx0; nullptr: not computed
    float* dA;                        // nullptr: not computed
    void* scratch;
    int64_t M;  int K, r;
    LoraMask mask;
    int dt;
};
int64_t lora_down_bwd_slabs(int64_t M, int K, int64_t* rows_per_slab);
size_t lora_down_bwd_bytes(int64_t M, int K, int r);
hipError_t launch_lora_dropout_mask(uint8_t* keep, int64_t M, int K, int64_t ldk, const LoraMask& mask, hipStream_t s);
hipError_t launch_lora_down(const LoraDownLaunch& a, hipStream_t s);
hipError_t launch_lora_down_bwd(const LoraDownBwdLaunch& a, hipStream_t s);

// pack.hip --------------------------------------------------------------------------------------
// rows (strand b, p_q) and (strand B + b, L - 1 - p_q) of a [2B*L, E] activation tensor -> out[(strand * P + q), E]
struct GatherRowsLaunch {
    const void* src;  void* out;
    int B, L, E;
    Positions pos;
    int dt;
    bool blocked = false;             // src is in the blocked layout (common.hpp::blocked_off)
};
hipError_t launch_gather_rows(const GatherRowsLaunch& g, hipStream_t s);
// generic 2-D copy/convert with zero padding: dst[r, c] (dst_dt, ld = dst_ld) = src[r, c] for r < rows, c < cols else 0
hipError_t launch_pack2d(const void* src, int src_dt, int64_t src_ld, void* dst, int dst_dt, int64_t dst_ld,
                         int rows, int cols, int dst_rows, int dst_cols, hipStream_t s);
// dst[r, c] (dst_dt) = src[r, c] * scale[c]: in_proj weight with the RMSNorm weight folded into its columns (norm-folded form)
hipError_t launch_pack_scale_cols(const void* src, int src_dt, int64_t src_ld, const float* scale, void* dst, int dst_dt,
                                  int64_t dst_ld, int rows, int cols, hipStream_t s);
// Layer 0 of the norm-folded form.  Its in_proj operand is one of the V embedding rows, so its output is one of V rows:
//   tab [V, N2] (dtype dt) = round((emb [V, D] . Wf [N2, D]^T) * rstd(emb row))                 (bind time)
//   x, z [2 B L, E] blocked = rows of tab gathered by token (rc strand by index arithmetic)    (instead of the layer-0 in_proj launch)
hipError_t launch_embed_inproj_table(const void* emb, const void* Wf, void* tab, int V, int D, int N2, float eps, int dt, hipStream_t s);
hipError_t launch_embed_xz_gather(const int32_t* ids, const int32_t* comp8, const void* tab, void* x, void* z, int B, int L, int E, int dt,
                                  hipStream_t s);
// split-bf16 operands of the fp32 model's big GEMMs ("f32_gemm_split"): v = hi + lo, hi = bf16(v), lo = bf16(v - hi);
//   weights     [rows, cols] (fp32 / bf16 source) -> bf16 [rows, 2 cols] = [hi | lo]                    (bind time)
//   activations fp32 [rows, K] (plain or blocked) -> bf16 [rows, 2 K]    = [hi | lo] (plain or blocked), K % 64 == 0
// so that a_hi w_hi + a_lo w_hi + a_hi w_lo is ONE bf16 GEMM of 3 K / 64 K-tiles whose cursor wraps around both operands
// (gemm.hip "wrap-around K cursor": launch_gemm_nt with GemmOperands K = 3 K, ksplit = K / 64) with an fp32 result.
hipError_t launch_pack_split_w(const void* src, int src_dt, int64_t src_ld, void* dst, int rows, int cols, hipStream_t s);
hipError_t launch_split_rows(const float* src, int64_t src_ld, void* dst, int64_t rows, int K, bool src_blocked, bool dst_blocked,
                             hipStream_t s);       // src_ld: elements between plain source rows (ignored for a blocked source)
// A2[e, n] = -exp(A_log[e, n]) * log2(e)   (A_log read through its storage dtype)
hipError_t launch_pack_A(const void* A_log, int src_dt, float* A2, int64_t n, float scale, hipStream_t s);

}  // namespace pcad
