"""-m gpu: pcad_linear_wgrad (include/pcad_bwd.h, csrc/wgrad.hip) as an operator, and ops.linear_fn on the device.

  exact      tests/gemm_ref.py's exact-integer method: operands from ints() in {-3 .. 3} cast to bf16, so that every partial sum stays an
             integer below 2^24 and the fp32 result must be torch.equal to the float64 product whatever the tile, slab and summation
             order.  Shapes (N, K): (8, 8) smallest; (96, 128) x_proj's form; (80, 256) Small's x_proj width; (128, 48) Small's dt_proj
             depth; (136, 72) neither a multiple of 16, one chunk past the 128-row tile; (136, 64) / (64, 136) one chunk past the
             128 x 128 tile's edge in each dimension; (264, 64) a third tile.  M: 1, 7, 31, 32, 33, 63, 64, 65, 257 and, all of these
             being shapes the slab rule splits, S - 1, S, S + 1, 2 S + 1 with S = rows_per_slab = 256
  further    accumulate=1 three times onto an integer-filled dw; strided operands (ldx = K + 32, lddy = N + 8, lddw = K + 4, a 3-d
             x_dbl[..., :R] view) read and written in place with the sentinels in the gaps intact; poison=True the same bits; two calls
             the same bits; M = 0 in both modes
  ordinary   randn operands at M = 1 000 and 8 192, (96, 128) and (256, 256): tests/scan_bwd_ref.py's metric against the float64 product
             of the same bf16 operands, under its bar for an fp32-stored tensor - max(3e-5, 8 x the deviation of the CPU fp32 matmul)
  linear_fn  with main_grad: dx = dy @ W bit for bit, the weight's .grad stays None, main_grad = linear_wgrad's output; the toy shapes
             (36, 128) and (128, 4) take the addmm path and meet the same bar
Every case prints its figures before it asserts.  Observed on an MI355X: every exact case exact; ordinary operands 1.4e-7 .. 2.2e-7
against a CPU fp32 matmul's 1.4e-7 .. 3.3e-7 [bar 3e-5]; the fallback shapes 2.0e-7."""
import pytest
import torch

import gemm_ref as G
import scan_bwd_ref as SB
from plantcaduceus_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
SHAPES = [(8, 8), (96, 128), (80, 256), (128, 48), (136, 72), (136, 64), (64, 136), (264, 64)]
MS = (1, 7, 31, 32, 33, 63, 64, 65, 257)


def int_pair(seed, M, N, K):
    """-> (dy [M, N], x [M, K]) bf16 on the CPU, small integers"""
    return G.ints(seed, M, N).to(BF), G.ints(seed + 1, M, K).to(BF)


def product(dy, x):
    """float64 dy^T x"""
    return dy.double().t() @ x.double()


@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: f"{s[0]}x{s[1]}")
def test_exact_integers(shape):
    N, K = shape
    S = ops.linear_wgrad_slabs(257, N, K)[1]
    assert S == 256 and ops.linear_wgrad_slabs(S, N, K)[0] == 1 and ops.linear_wgrad_slabs(S + 1, N, K)[0] == 2 \
        and ops.linear_wgrad_slabs(2 * S + 1, N, K) == (3, S)
    wrong = []
    for M in MS + (S - 1, S, S + 1, 2 * S + 1):
        dy, x = int_pair(100 + M, M, N, K)
        got = ops.linear_wgrad(dy.to(DEV), x.to(DEV)).cpu()
        ref = product(dy, x)
        assert got.dtype == F32 and got.shape == (N, K) and ref.abs().max().item() < 2 ** 24
        if not torch.equal(got.double(), ref):
            wrong.append((M, int((got.double() != ref).sum())))
    print(f"({N}, {K}): {len(MS) + 4} values of M, S = {S}; not exact at (M, elements): {wrong}")
    assert not wrong


def test_accumulate_three_times_is_exact():
    N, K, M = 96, 128, 300                                      # two slabs
    d0 = G.ints(7, N, K, r=50)
    dw = d0.to(DEV)
    want = d0.double()
    for i in range(3):
        dy, x = int_pair(20 + 2 * i, M + i, N, K)
        out = ops.linear_wgrad(dy.to(DEV), x.to(DEV), out=dw, accumulate=True)
        assert out is dw
        want = want + product(dy, x)
    print(f"accumulate x 3: max |dw| {want.abs().max().item():.0f}")
    assert torch.equal(dw.cpu().double(), want)
    # without accumulate the old content - NaN here - is never read
    dw.fill_(float("nan"))
    dy, x = int_pair(30, M, N, K)
    assert torch.equal(ops.linear_wgrad(dy.to(DEV), x.to(DEV), out=dw).cpu().double(), product(dy, x))


@pytest.mark.parametrize("M", [65, 513])
def test_strided_operands_in_place(M):
    N, K, SENT = 136, 72, -1024.0
    dy, x = int_pair(40 + M, M, N, K)
    ybuf = torch.full((M, N + 8), SENT, dtype=BF, device=DEV)
    xbuf = torch.full((M, K + 32), SENT, dtype=BF, device=DEV)
    wbuf = torch.full((N, K + 4), SENT, dtype=F32, device=DEV)
    ybuf[:, :N], xbuf[:, :K] = dy.to(DEV), x.to(DEV)
    yv, xv, wv = ybuf[:, :N], xbuf[:, :K], wbuf[:, :K]
    for v, ld in ((yv, N + 8), (xv, K + 32)):
        t, rows, got_ld = ops._wgrad_rows(v, "v")
        assert t.data_ptr() == v.data_ptr() and rows == M and got_ld == ld        # read in place, no copy
    d0 = G.ints(9, N, K, r=9)
    wv.copy_(d0)
    out = ops.linear_wgrad(yv, xv, out=wv, accumulate=True)
    assert out.data_ptr() == wbuf.data_ptr()
    assert torch.equal(wv.cpu().double(), d0.double() + product(dy, x))
    assert bool((wbuf[:, K:] == SENT).all()) and bool((ybuf[:, N:] == SENT).all()) and bool((xbuf[:, K:] == SENT).all())
    # a 3-d slice such as x_dbl[..., :R] collapses to one row stride; a transposed one does not and is copied
    x3 = torch.zeros((2, 33, 40), dtype=BF, device=DEV)
    t, rows, ld = ops._wgrad_rows(x3[..., :8], "x")
    assert t.data_ptr() == x3.data_ptr() and (rows, ld) == (66, 40)
    t, rows, ld = ops._wgrad_rows(x3.transpose(1, 2), "x")
    assert t.is_contiguous() and t.data_ptr() != x3.data_ptr() and (rows, ld) == (80, 33)
    xs = G.ints(77, 66, 40).to(BF).view(2, 33, 40).to(DEV)
    dys = G.ints(78, 66, 16).to(BF).view(2, 33, 16).to(DEV)
    got = ops.linear_wgrad(dys, xs[..., :8])
    assert torch.equal(got.cpu().double(), product(dys.cpu().view(66, 16), xs.cpu().view(66, 40)[:, :8]))


def test_poison_and_repeat_give_the_same_bits():
    for (N, K), M in (((96, 128), 513), ((264, 64), 65), ((8, 8), 257)):
        g = torch.Generator().manual_seed(M)
        dy = (torch.randn(M, N, generator=g) / M ** 0.5).to(BF).to(DEV)
        x = torch.randn(M, K, generator=g).to(BF).to(DEV)
        d0 = torch.randn(N, K, generator=g).to(DEV)
        for acc in (False, True):
            a = ops.linear_wgrad(dy, x, out=d0.clone(), accumulate=acc)
            assert ops.linear_wgrad.guards_ok is None
            b = ops.linear_wgrad(dy, x, out=d0.clone(), accumulate=acc)
            c = ops.linear_wgrad(dy, x, out=d0.clone(), accumulate=acc, poison=True)
            print(f"({N}, {K}) M {M} accumulate {acc}: repeat equal {torch.equal(a, b)}, poisoned equal {torch.equal(a, c)}, sentinels intact "
                  f"{ops.linear_wgrad.guards_ok}")
            assert bool(torch.isfinite(a).all()) and torch.equal(a, b) and torch.equal(a, c) and ops.linear_wgrad.guards_ok is True


def test_no_rows():
    N, K = 96, 128
    dy, x = torch.zeros((0, N), dtype=BF, device=DEV), torch.zeros((0, K), dtype=BF, device=DEV)
    d0 = torch.randn(N, K, generator=torch.Generator().manual_seed(3)).to(DEV)
    kept = ops.linear_wgrad(dy, x, out=d0.clone(), accumulate=True)
    zero = ops.linear_wgrad(dy, x, out=torch.full_like(d0, float("nan")))
    assert torch.equal(kept, d0) and bool((zero == 0).all())


_ordinary = {}


def ordinary(M, N, K):
    """(dy, x) bf16 CPU, the float64 product, the CPU fp32 matmul's deviation from it - computed once per case"""
    def make():
        g = torch.Generator().manual_seed(M + N)
        dy = (torch.randn(M, N, generator=g) / M ** 0.5).to(BF)
        x = torch.randn(M, K, generator=g).to(BF)
        ref = product(dy, x)
        return dy, x, ref, SB.metric(dy.float().t() @ x.float(), ref)
    return G.cached(("wgrad", M, N, K), make)


@pytest.mark.parametrize("M", [1000, 8192])
@pytest.mark.parametrize("shape", [(96, 128), (256, 256)], ids=["96x128", "256x256"])
def test_ordinary_operands(shape, M):
    N, K = shape
    dy, x, ref, dev32 = ordinary(M, N, K)
    bar = SB.bar("dw", {"dw": dev32}, False)
    got = ops.linear_wgrad(dy.to(DEV), x.to(DEV))
    err = SB.metric(got, ref)
    onto = torch.full((N, K), 0.5, device=DEV)
    err_acc = SB.metric(ops.linear_wgrad(dy.to(DEV), x.to(DEV), out=onto, accumulate=True), ref + 0.5)
    print(f"({N}, {K}) M {M}: slabs {ops.linear_wgrad_slabs(M, N, K)}; error {err:.2e}, onto 0.5 {err_acc:.2e} [bar {bar:.2e}; CPU fp32 matmul {dev32:.2e}]")
    assert bar == max(3e-5, 8 * dev32) and err <= bar and err_acc <= bar


def test_linear_fn_with_main_grad_on_the_device():
    g = torch.Generator().manual_seed(11)
    N, K = 40, 128                                              # the toy x_proj at dt_rank 8
    x = torch.randn(2, 69, K, generator=g).to(BF).to(DEV).requires_grad_(True)
    w = torch.nn.Parameter((torch.randn(N, K, generator=g) / K ** 0.5).to(BF).to(DEV))
    dy = torch.randn(2, 69, N, generator=g).to(BF).to(DEV)
    start = torch.randn(N, K, generator=g).to(DEV)
    w.main_grad = start.clone()
    y = ops.linear_fn(x, w)
    assert torch.equal(y, torch.nn.functional.linear(x.detach(), w.detach()))
    y.backward(dy)
    assert w.grad is None
    assert G.same_bits(x.grad, dy @ w.detach())
    assert torch.equal(w.main_grad, ops.linear_wgrad(dy, x.detach(), out=start.clone(), accumulate=True))
    assert not torch.equal(w.main_grad, start)


@pytest.mark.parametrize("shape", [(36, 128), (128, 4)], ids=["36x128", "128x4"])
def test_linear_fn_fallback_shapes_meet_the_bar(shape):
    N, K = shape
    assert not ops.wgrad_kernel_takes(N, K)
    g = torch.Generator().manual_seed(12)
    x = torch.randn(2, 69, K, generator=g).to(BF)
    w = (torch.randn(N, K, generator=g) / K ** 0.5).to(BF)
    dy = (torch.randn(2, 69, N, generator=g) / 138 ** 0.5).to(BF)
    ref = product(dy.view(-1, N), x.view(-1, K))
    dev32 = SB.metric(dy.view(-1, N).float().t() @ x.view(-1, K).float(), ref)
    bar = SB.bar("dw", {"dw": dev32}, False)
    xd = x.to(DEV).requires_grad_(True)
    wd = torch.nn.Parameter(w.to(DEV))
    wd.main_grad = torch.zeros((N, K), device=DEV)
    ops.linear_fn(xd, wd).backward(dy.to(DEV))
    err = SB.metric(wd.main_grad, ref)
    print(f"fallback ({N}, {K}): error {err:.2e} [bar {bar:.2e}; CPU fp32 matmul {dev32:.2e}]")
    assert wd.grad is None and G.same_bits(xd.grad, dy.to(DEV) @ wd.detach()) and err <= bar
