"""Inputs and float64 expected outputs for the GEMM launch forms of the engine (test helper; no tests here) - what tests/scan_ref.py is
to the scan.  Used by tests/test_gemm_forms.py (CPU) and tests/test_gpu_gemm_forms.py.

The exact-integer method: operands uniform in {-3 .. 3}.  bf16 and fp32 hold them exactly, every product is an integer of at most 9
and every partial sum of a K <= 2048 product is an integer of magnitude <= 9 K (27 K for the three products of the split form) < 2^24,
so fp32 accumulation is exact in ANY order: the kernel's result does not depend on its summation order, its K-tile order or its MFMA
shape, and must equal the float64 product bit for bit after the one rounding to the stored dtype.  Two different sums of this kind
are equal by chance about once in a hundred (sigma ~ 4 sqrt(K)), so a wrong operand row, K-tile, part or scale shows on ~99 % of
the outputs it touches (tests/test_gemm_forms.py measures that for each modelled fault)."""
import torch

INT_MAX_K = 2048           # 27 * 2048 < 2^24


def ints(seed, rows, cols, r=3):
    """fp32 [rows, cols], integers uniform in {-r .. r}"""
    g = torch.Generator().manual_seed(seed)
    return torch.randint(-r, r + 1, (rows, cols), generator=g).float()


def randn_pair(seed, M, N, K, dtype):
    """ordinary operands, scaled as tests/test_gpu_ops.py test_linear_* scales them, rounded to dtype.  -> (x [M, K], w [N, K]) dtype"""
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    return x, w


def rscale(M):
    """per-row powers of two whose exponent has period 7 in the row index - coprime to the 16 rows of an MFMA tile, the 128 of a wave
    tile and the 256 of a block tile, so that a factor taken from another row of any of those strides is a different factor"""
    return torch.pow(2.0, (torch.arange(M) % 7 - 3).float())


def product(a, w):
    """float64 a . w^T"""
    return a.double() @ w.double().t()


def split_product(a2, w2, Ko, parts=((0, 0), (1, 0), (0, 1))):
    """the split form on [hi | lo] operands a2 [M, 2 Ko], w2 [N, 2 Ko]: sum over (A part, W part) of the wrap-around K cursor -
    a_hi w_hi + a_lo w_hi + a_hi w_lo (csrc/gemm.hip ksplit_a / ksplit_w).  float64."""
    part = lambda t, p: t[:, p * Ko:(p + 1) * Ko]
    return sum(product(part(a2, pa), part(w2, pw)) for pa, pw in parts)


def stored(ref64, dtype):
    """the one rounding to the stored dtype (float64 -> fp32 is exact for every value here that fp32 holds)"""
    return ref64.float().to(dtype)


def c2_of(ref64, dtype):
    """the x_proj form's fp32 side output: values rounded to the model dtype, held in fp32"""
    return stored(ref64, dtype).float()


def ssq_of(res64):
    """[M, N / 128] float64: per-row sums of squares over each 128-column slab"""
    M, N = res64.shape
    return (res64 ** 2).view(M, N // 128, 128).sum(-1)


def same_bits(a, b):
    a, b = a.detach().cpu().contiguous(), b.detach().cpu().contiguous()
    if a.dtype != b.dtype or a.shape != b.shape:
        return False
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.view(it), b.view(it))


def relerr(got, ref):
    """the project's GEMM metric (tests/test_gpu_ops.py): max |got - ref| / max |ref|"""
    got, ref = got.double().cpu(), ref.double().cpu()
    return ((got - ref).abs().max() / ref.abs().max()).item()


def blocked_off(r, cb, pieces):
    """csrc/common.hpp blocked_off: byte offset of (row r, byte cb of the row) for rows of `pieces` x 128 bytes"""
    return (((r >> 3) * pieces + (cb >> 7)) << 10) + ((r & 7) << 7) + (cb & 127)


# ---- modelled faults (tests/test_gemm_forms.py): what a kernel with one wrong address, part or wait would compute -------------------
def stale_k_tile(a, w, kt, src_rows, kc=64):
    """K-tile kt (kc columns) of A taken from other rows of A (a ring slot that still holds another output tile's K-tile)"""
    bad = a.clone()
    bad[:, kt * kc:(kt + 1) * kc] = a[src_rows, kt * kc:(kt + 1) * kc]
    return product(bad, w)


def rows_rotated(ref64, by=1):
    """every 8-row block's rows rotated: a blocked operand or output addressed with (r + by) % 8"""
    M = ref64.shape[0] // 8 * 8
    out = ref64.clone()
    out[:M] = ref64[:M].view(M // 8, 8, -1).roll(-by, 1).reshape(M, -1)
    return out


def groups_exchanged(ref64, nsplit):
    """the two outputs' 16-column groups exchanged across nsplit: group j of C1 <-> group j of C2, as far as both exist"""
    n = min(nsplit, ref64.shape[1] - nsplit) // 16 * 16
    out = ref64.clone()
    out[:, :n], out[:, nsplit:nsplit + n] = ref64[:, nsplit:nsplit + n], ref64[:, :n]
    return out


# ---- refusals: calls the entries must answer with PCAD_ERR_INVALID before anything is launched ----------------------------------------
def refusals(p, device=False):
    """p: dict of (16-byte aligned) addresses A, W, C, C2, C3, rscale - never dereferenced by a refused call.
    -> [(why, entry, arguments without the stream)].  device: also the one refusal that is decided next to the launch itself (after
    the launcher has asked the device for its CU count)."""
    BF, F32 = 1, 0
    A, W, C, C2, C3 = p["A"], p["W"], p["C"], p["C2"], p["C3"]
    #   two:      A, lda, W, ldw, C1, C2, nsplit, rscale, M, N, K, a_blocked, out_blocked, ksplit, dtype, out_dtype
    #   x_proj:   A, lda, W, ldw, C, ldc, C2, ldc2, nsplit, M, N, K, a_blocked, ksplit, dtype
    #   residual: A, lda, W, ldw, C, res, ssq, M, N, K, a_blocked, ksplit, dtype
    #   plain:    A, lda, W, ldw, C, ldc, M, N, K, a_blocked, ksplit, dtype, out_dtype
    calls = [
        ("out_blocked with nsplit * elem % 128 != 0", "pcad_gemm_nt_two", (A, 128, W, 128, C, C2, 80, None, 256, 176, 64, 0, 1, 0, BF, BF)),
        ("a_blocked in the two form", "pcad_gemm_nt_two", (A, 64, W, 64, C, C2, 128, None, 256, 256, 64, 1, 0, 0, BF, BF)),
        ("ksplit in the x_proj form", "pcad_gemm_nt_xproj", (A, 192, W, 192, C, 64, C2, 32, 64, 256, 96, 192, 0, 1, BF)),
        ("ksplit in the residual form", "pcad_gemm_nt_residual_engine", (A, 192, W, 192, C, C2, C3, 256, 256, 192, 0, 1, BF)),
        ("ksplit with K != 3 ksplit 64, plain form", "pcad_gemm_nt_engine", (A, 128, W, 128, C, 256, 256, 256, 128, 0, 1, BF, F32)),
        ("ksplit with K != 3 ksplit 64, two form", "pcad_gemm_nt_two", (A, 128, W, 128, C, C2, 128, None, 256, 256, 128, 0, 0, 1, BF, F32)),
    ]
    if device:
        calls.append(("rscale on a shape that is not whole tiles", "pcad_gemm_nt_two",
                      (A, 64, W, 64, C, C2, 256, p["rscale"], 300, 512, 64, 0, 0, 0, BF, BF)))
    return calls


def accepted_twins(p):
    """the refusals above with the one offending argument put right: calls the argument checks of the entries let through (they are
    launches - for a device only)"""
    BF, F32 = 1, 0
    A, W, C, C2, C3 = p["A"], p["W"], p["C"], p["C2"], p["C3"]
    return [
        ("pcad_gemm_nt_two", (A, 128, W, 128, C, C2, 128, None, 256, 256, 64, 0, 1, 0, BF, BF)),
        ("pcad_gemm_nt_xproj", (A, 192, W, 192, C, 64, C2, 32, 64, 256, 96, 192, 0, 0, BF)),
        ("pcad_gemm_nt_residual_engine", (A, 192, W, 192, C, C2, C3, 256, 256, 192, 0, 0, BF)),
        ("pcad_gemm_nt_engine", (A, 128, W, 128, C, 256, 256, 256, 192, 0, 1, BF, F32)),
    ]


_cache = {}


def cached(key, fn):
    if key not in _cache:
        _cache[key] = fn()
    return _cache[key]
