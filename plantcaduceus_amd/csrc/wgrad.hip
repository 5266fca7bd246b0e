// Weight gradient of a linear layer with fp32 main gradients (include/pcad_bwd.h pcad_linear_wgrad, libpcad_bwd.so):
//   dw[n, k] = (accumulate ? dw[n, k] : 0) + s[n, k]        s[n, k] = sum_m dy[m, n] x[m, k]
// dy [M, N] and x [M, K] are bf16, dw [N, K] is fp32 and is accumulated IN PLACE: the bf16 [N, K] gradient that stock autograd would
// return is never formed and never rounded.  Every bf16 x bf16 product is exact in fp32 and the sum is fp32 in a fixed order.
//
// The reduction runs over the ROW index of both operands, so both MFMA operands are column reads of row-major tiles.  A block of 4
// waves owns a WG_BN x WG_BK tile of dw and one slab of rows; it walks its rows WG_TM at a time:
//   stage    each lane copies 4 + 4 chunks of 16 bytes (8 bf16) global -> registers -> LDS; rows past the slab's end and columns past
//            N / K are stored as zeros ("pad, don't mask": the reads below never branch).  The next step's chunks are loaded into
//            registers before this step's products are issued.
//   image    per operand [WG_TM rows][WG_LD = 144 bf16 = 288 bytes]: 128 data columns + 16 of padding that nothing reads.
//   read     v_mfma_f32_16x16x32_bf16 wants lane l to hold, for output row / column l & 15, the 8 values k = 8 (l >> 4) + j.  One
//            ds_read_b64_tr_b16 hands lane i of a 16-lane group column c0 + i of 4 consecutive rows; lane 4 q + p supplies the address
//            of row r0 + q, columns c0 + 4 p .. + 3.  Per 32-row step, group g = l >> 4 takes rows 4 g .. 4 g + 3 (elements 0..3) and
//            rows 16 + 4 g .. 16 + 4 g + 3 (elements 4..7).  Both operands use the same rows for the same (g, j), which is all the
//            sum over m needs.  EXEC is all ones at every read: the reads sit in block-uniform control flow only.
//   banks    bank = (byte / 4) % 64 per 32-lane half.  A half's two groups read rows 8 h .. 8 h + 7 of a 16-row band; row r starts
//            at dword 72 r + c0 / 2, i.e. bank 8 (r % 8) + const, and a row's four lanes cover 8 consecutive banks: the half's 32
//            lanes cover all 64 banks once - conflict-free.
//   wave     w: rows 64 (w >> 1) .. + 63 and columns 64 (w & 1) .. + 63 of the tile, 4 x 4 accumulators of 16 x 16.
// One slab (tiles alone fill the device): the epilogue adds the old dw once and stores.  Several slabs: each block stores its partial
// tile to the caller's scratch [slab][N][K] and wgrad_reduce_kernel adds the slabs in index order, then the old value once.  The slab
// rule (wgrad_slabs) is a function of (M, N, K) and the constants in kernels.hpp - never of the device - so the bits are the same on
// any box.  No floating-point atomics.  All in-tensor offsets are 64-bit.
#include "common.hpp"
#include "kernels.hpp"

namespace pcad {

namespace {
typedef __bf16 wg_bf16x8 __attribute__((ext_vector_type(8)));
typedef short wg_s16x4 __attribute__((ext_vector_type(4)));
typedef short wg_s16x8 __attribute__((ext_vector_type(8)));
typedef __attribute__((address_space(3))) wg_s16x4 wg_lds_s16x4;

constexpr int WG_LD = WGRAD_BK + 16;             // image row in bf16: 288 bytes (see `banks` above); WGRAD_BN == WGRAD_BK
constexpr int WG_CH = WGRAD_BK / 8;              // 16-byte chunks per image row
constexpr int WG_LOADS = WGRAD_TM * WG_CH / 256; // chunks per lane, operand and step
static_assert(WGRAD_BN == WGRAD_BK && WGRAD_BK == 128 && WGRAD_TM % 32 == 0 && WGRAD_TM * WG_CH % 256 == 0, "the lane maps below assume these");

// column-major fragment of 8 rows (4 + 4, 16 apart) for column c0 + (lane & 15): two transposed reads
__device__ __forceinline__ wg_bf16x8 wg_frag(const unsigned short* img, int row_lane, int col) {
    const unsigned short* p0 = img + row_lane * WG_LD + col;
    const wg_s16x4 lo = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)p0);
    const wg_s16x4 hi = __builtin_amdgcn_ds_read_tr16_b64_v4i16((wg_lds_s16x4*)(p0 + 16 * WG_LD));
    const wg_s16x8 v = __builtin_shufflevector(lo, hi, 0, 1, 2, 3, 4, 5, 6, 7);
    return __builtin_bit_cast(wg_bf16x8, v);
}
}  // namespace

int64_t wgrad_slabs(int64_t M, int N, int K, int64_t* rows_per_slab) {
    if (M <= 0) { *rows_per_slab = 0; return 0; }
    const int64_t tiles = (int64_t)((N + WGRAD_BN - 1) / WGRAD_BN) * ((K + WGRAD_BK - 1) / WGRAD_BK);
    int64_t want = WGRAD_TARGET_BLOCKS / tiles;
    want = want < 1 ? 1 : want > WGRAD_MAX_SLABS ? WGRAD_MAX_SLABS : want;
    int64_t rows = (M + want - 1) / want;
    rows = (rows + WGRAD_SLAB_ROWS - 1) / WGRAD_SLAB_ROWS * WGRAD_SLAB_ROWS;
    *rows_per_slab = rows;
    return (M + rows - 1) / rows;
}

size_t wgrad_bytes(int64_t M, int N, int K) {
    int64_t rows;
    const int64_t slabs = wgrad_slabs(M, N, K, &rows);
    if (slabs <= 1) return 0;
    return ((size_t)slabs * (size_t)N * (size_t)K * sizeof(float) + 255) / 256 * 256;
}

// grid (tiles_n * tiles_k, slabs).  out / ldo: dw / lddw with one slab, the slab's partial [N][K] / K otherwise (add_old 0).
__global__ __launch_bounds__(256) void wgrad_kernel(const unsigned short* __restrict__ dy, int64_t lddy, const unsigned short* __restrict__ x,
                                                    int64_t ldx, float* __restrict__ out, int64_t ldo, int64_t slab_stride, int64_t M, int N,
                                                    int K, int64_t rows_per_slab, int tiles_k, int add_old) {
    __shared__ __attribute__((aligned(16))) unsigned short img_a[WGRAD_TM * WG_LD];   // dy tile
    __shared__ __attribute__((aligned(16))) unsigned short img_b[WGRAD_TM * WG_LD];   // x tile
    const int tid = threadIdx.x, lane = tid & 63, wv = tid >> 6;
    const int n0 = ((int)blockIdx.x / tiles_k) * WGRAD_BN, k0 = ((int)blockIdx.x % tiles_k) * WGRAD_BK;
    const int64_t m_begin = (int64_t)blockIdx.y * rows_per_slab;
    const int64_t m_end = m_begin + rows_per_slab < M ? m_begin + rows_per_slab : M;
    out += (int64_t)blockIdx.y * slab_stride;

    // staging: chunk ch of rows (tid >> 4) + 16 i
    const int ch = tid & (WG_CH - 1), srow = tid / WG_CH;
    const bool a_in = n0 + ch * 8 < N, b_in = k0 + ch * 8 < K;     // N, K multiples of 8: a chunk is wholly inside or outside
    const unsigned short* const a_src = dy + n0 + ch * 8;
    const unsigned short* const b_src = x + k0 + ch * 8;
    u32x4 ra[WG_LOADS], rb[WG_LOADS];
    auto fetch = [&](int64_t m0) {
#pragma unroll
        for (int i = 0; i < WG_LOADS; ++i) {
            const int64_t m = m0 + srow + (256 / WG_CH) * i;
            const u32x4 z = {0u, 0u, 0u, 0u};
            ra[i] = (a_in && m < m_end) ? *(const u32x4*)(a_src + m * lddy) : z;
            rb[i] = (b_in && m < m_end) ? *(const u32x4*)(b_src + m * ldx) : z;
        }
    };
    auto stash = [&]() {
#pragma unroll
        for (int i = 0; i < WG_LOADS; ++i) {
            const int r = srow + (256 / WG_CH) * i;
            *(u32x4*)(img_a + r * WG_LD + ch * 8) = ra[i];
            *(u32x4*)(img_b + r * WG_LD + ch * 8) = rb[i];
        }
    };

    // reading: lane 4 q + p of group g addresses row 4 g + q, columns + 4 p
    const int g = lane >> 4, q = (lane >> 2) & 3, p = lane & 3;
    const int row_lane = 4 * g + q;
    const int wn = (wv >> 1) * 64, wk = (wv & 1) * 64;

    f32x4 acc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    if (m_begin < m_end) fetch(m_begin);
    for (int64_t m0 = m_begin; m0 < m_end; m0 += WGRAD_TM) {       // block-uniform: EXEC stays all ones
        stash();
        __syncthreads();
        if (m0 + WGRAD_TM < m_end) fetch(m0 + WGRAD_TM);
#pragma unroll
        for (int s = 0; s < WGRAD_TM / 32; ++s) {
            wg_bf16x8 fa[4], fb[4];
#pragma unroll
            for (int t = 0; t < 4; ++t) {
                fa[t] = wg_frag(img_a, 32 * s + row_lane, wn + 16 * t + 4 * p);
                fb[t] = wg_frag(img_b, 32 * s + row_lane, wk + 16 * t + 4 * p);
            }
#pragma unroll
            for (int i = 0; i < 4; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(fa[i], fb[j], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
    }

    // C/D map: column (k) = lane & 15, row (n) = 4 (lane >> 4) + register
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = k0 + wk + 16 * j + (lane & 15);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int n = n0 + wn + 16 * i + 4 * g + r;
                if (n < N && k < K) {
                    float* const d = out + (int64_t)n * ldo + k;
                    *d = add_old ? *d + acc[i][j][r] : acc[i][j][r];
                }
            }
        }
}

// dw[n, k..k+3] = (add_old ? dw : 0) + ((part[0] + part[1]) + ... + part[slabs - 1]): slab order, the old value added once, last
__global__ __launch_bounds__(256) void wgrad_reduce_kernel(const float* __restrict__ part, int slabs, float* __restrict__ dw, int64_t lddw,
                                                           int N, int K, int add_old) {
    const int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
    const int k4 = K >> 2;
    if (idx >= (int64_t)N * k4) return;
    const int n = (int)(idx / k4), k = (int)(idx % k4) * 4;
    const int64_t off = (int64_t)n * K + k, stride = (int64_t)N * K;
    f32x4 s = *(const f32x4*)(part + off);
    for (int i = 1; i < slabs; ++i) s += *(const f32x4*)(part + i * stride + off);
    f32x4* const d = (f32x4*)(dw + (int64_t)n * lddw + k);
    *d = add_old ? *d + s : s;
}

hipError_t launch_linear_wgrad(const LinearWgradLaunch& a, hipStream_t s) {
    if (!a.dw || a.N <= 0 || a.K <= 0 || a.N % 8 || a.K % 8 || a.M < 0) return hipErrorInvalidValue;
    if (a.M == 0 && a.accumulate) return hipSuccess;
    if (a.M > 0 && (!a.dy || !a.x)) return hipErrorInvalidValue;
    int64_t rows = 0;
    int64_t slabs = wgrad_slabs(a.M, a.N, a.K, &rows);
    if (slabs == 0) { slabs = 1; rows = 0; }                       // M == 0 without accumulate: every block stores its zero tile
    if (slabs > 1 && !a.scratch) return hipErrorInvalidValue;
    const int tiles_n = (a.N + WGRAD_BN - 1) / WGRAD_BN, tiles_k = (a.K + WGRAD_BK - 1) / WGRAD_BK;
    const dim3 grid((unsigned)(tiles_n * tiles_k), (unsigned)slabs);
    if (slabs == 1) {
        hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, s, (const unsigned short*)a.dy, a.lddy, (const unsigned short*)a.x, a.ldx, a.dw,
                           a.lddw, (int64_t)0, a.M, a.N, a.K, rows, tiles_k, a.accumulate ? 1 : 0);
        return hipGetLastError();
    }
    float* const part = (float*)a.scratch;
    hipLaunchKernelGGL(wgrad_kernel, grid, dim3(256), 0, s, (const unsigned short*)a.dy, a.lddy, (const unsigned short*)a.x, a.ldx, part,
                       (int64_t)a.K, (int64_t)a.N * a.K, a.M, a.N, a.K, rows, tiles_k, 0);
    if (hipError_t e = hipGetLastError()) return e;
    const int64_t quads = (int64_t)a.N * (a.K / 4);
    hipLaunchKernelGGL(wgrad_reduce_kernel, dim3((unsigned)((quads + 255) / 256)), dim3(256), 0, s, (const float*)part, (int)slabs, a.dw, a.lddw,
                       a.N, a.K, a.accumulate ? 1 : 0);
    return hipGetLastError();
}

}  // namespace pcad
