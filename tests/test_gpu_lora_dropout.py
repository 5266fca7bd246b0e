"""-m gpu: the LoRA dropout kernels as operators (include/pcad_bwd.h pcad_lora_dropout_mask / pcad_lora_down / pcad_lora_down_bwd,
csrc/lora.hip) and ops.lora_dropout_linear_fn.

  mask       the device generator == tests/lora_dropout_ref.py's numpy restatement, bit for bit, at (M, K) = (1, 8), (65, 72), (257, 520)
             and p = 0, 0.1, 0.5, written into a strided frame between sentinel bytes
  exact      tests/gemm_ref.py's exact-integer method: x, A, u, dx0 from ints() in {-3 .. 3} and p = 0.5, so c = 2 and every partial sum
             is an integer below 2^24: t, dA and dx must be torch.equal to the float64 result whatever the order (a bf16 dx: to its one
             rounding).  K in {8, 64, 72, 512, 520, 1536}: below a chunk, a whole chunk, one lane past it, three chunks; M in
             {1, 3, 63, 64, 65, 257} and S - 1, S, S + 1, 2 S + 1 around the slab boundary S the _slabs entry reports; r in {4, 8, 16};
             both dtypes
  ordinary   randn operands at M = 1 000, p = 0.1: scan_bwd_ref.metric against the float64 restatement under scan_bwd_ref.bar -
             fp32-stored outputs max(3e-5, 8 x the CPU fp32 restatement's own deviation), a bf16-stored dx 2^-7
  further    dropped elements of dx keep dx0's bits; dx alone and dA alone give the bits of the joint call; strided x and dx with the
             sentinels in the gaps intact; poison=True and a repeat give the same bits; M = 0
  function   lora_dropout_linear_fn at p = 0 against the float64 unmerged graph; what one call saves for the backward
Every case prints its figures before it asserts.  Observed on an MI355X: the mask and every exact case exact; ordinary operands t
8.9e-8 .. 1.5e-7, dA 1.2e-7 .. 2.2e-7, fp32 dx 3.7e-8 .. 4.7e-8 [bar 3e-5; CPU fp32 restatement 3.7e-8 .. 5.0e-7], bf16 dx 1.8e-3 .. 3.1e-3
[2^-7]; the Function y / dx 2.2e-7 .. 2.7e-7 in fp32, 4.0e-3 .. 4.4e-3 in bf16, dA / dB 1.4e-7 .. 1.8e-7; saved 33 632 bytes (bf16; x alone
19 872) and 59 264 (fp32) [allowed 34 656 / 60 288]."""
import numpy as np
import pytest
import torch

import gemm_ref as G
import lora_dropout_ref as LD
import scan_bwd_ref as SB
from plantcaduceus_amd import ops

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32, F64 = torch.bfloat16, torch.float32, torch.float64
KS = (8, 64, 72, 512, 520, 1536)
MS = (1, 3, 63, 64, 65, 257)
SEED, STREAM = 1234, 5


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
@pytest.mark.parametrize("M,K", [(1, 8), (65, 72), (257, 520)])
def test_mask_is_the_restatement_bit_for_bit(M, K, p):
    ref = LD.keep_mask(M, K, p, SEED, STREAM)
    got = ops.lora_dropout_mask(M, K, p, SEED, STREAM, poison=True)
    assert got.dtype == torch.bool and got.shape == (M, K) and ops.lora_dropout_mask.guards_ok
    diff = int((got.cpu().numpy() != ref).sum())
    print(f"({M}, {K}) p={p}: kept {int(ref.sum())} of {M * K}, differing elements {diff}")
    assert diff == 0
    assert np.array_equal(ops.lora_dropout_mask(M, K, p, SEED, STREAM).cpu().numpy(), ref)        # the contiguous form
    hi = ops.lora_dropout_mask(M, K, p, SEED + (3 << 32), STREAM + (1 << 40)).cpu().numpy()        # the high words reach the generator
    assert np.array_equal(hi, LD.keep_mask(M, K, p, SEED + (3 << 32), STREAM + (1 << 40)))


def int_case(seed, M, K, r, dtype):
    """-> x [M, K] dtype, A [r, K], u [M, r], dx0 [M, K] dtype: small integers, on the CPU"""
    return G.ints(seed, M, K).to(dtype), G.ints(seed + 1, r, K), G.ints(seed + 2, M, r), G.ints(seed + 3, M, K).to(dtype)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K", KS)
def test_exact_integers(K, dtype):
    S = ops.lora_down_bwd_slabs(257, K, 8)[1]
    assert S == 64 and ops.lora_down_bwd_slabs(S, K, 8)[0] == 1 and ops.lora_down_bwd_slabs(S + 1, K, 8)[0] == 2 \
        and ops.lora_down_bwd_slabs(2 * S + 1, K, 8) == (3, S)
    p, c = 0.5, float(LD.keep_scale(0.5))
    assert c == 2.0
    wrong = []
    ms = sorted(set(MS + (S - 1, S, S + 1, 2 * S + 1)))
    for M in ms:
        keep = torch.from_numpy(LD.keep_mask(M, K, p, SEED, STREAM))
        for r in ops.LORA_RANKS:
            x, A, u, dx0 = int_case(10 * M + r, M, K, r, dtype)
            t_ref = LD.down(x.double(), A.double(), keep, c)
            dx_ref, dA_ref = LD.down_bwd(x.double(), A.double(), u.double(), dx0.double(), keep, c)
            assert max(t_ref.abs().max().item(), dA_ref.abs().max().item(), dx_ref.abs().max().item()) < 2 ** 24
            t = ops.lora_down(x.to(DEV), A.to(DEV), p, SEED, STREAM, poison=True)
            ok = ops.lora_down.guards_ok
            dx, dA = ops.lora_down_bwd(x.to(DEV), A.to(DEV), u.to(DEV), dx0.to(DEV), p, SEED, STREAM, poison=True)
            ok = ok and ops.lora_down_bwd.guards_ok
            assert t.dtype == F32 and t.shape == (M, r) and dA.dtype == F32 and dA.shape == (r, K) and dx.dtype == dtype and dx.shape == (M, K)
            bad = [n for n, got, ref in (("t", t, t_ref), ("dA", dA, dA_ref)) if not torch.equal(got.cpu().double(), ref)]
            if not G.same_bits(dx, dx_ref.float().to(dtype)):       # fp32: the float64 integers themselves; bf16: their one rounding
                bad.append("dx")
            if bad or not ok:
                wrong.append((M, r, bad, ok))
    print(f"K = {K} {dtype}: {len(ms)} values of M x r in {ops.LORA_RANKS}, S = {S}; not exact at (M, r, outputs, guards): {wrong}")
    assert not wrong


def ordinary(seed, M, K, r, dtype):
    g = torch.Generator().manual_seed(seed)
    x = torch.randn(M, K, generator=g).to(dtype)
    A = (torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5
    u = torch.randn(M, r, generator=g)
    dx0 = torch.randn(M, K, generator=g).to(dtype)
    return x, A, u, dx0


def reference(x, A, u, dx0, keep, c, dtype):
    """-> (t, dx, dA) of the restatement computed in `dtype` on the operands as stored"""
    t = LD.down(x.to(dtype), A.to(dtype), keep, c)
    dx, dA = LD.down_bwd(x.to(dtype), A.to(dtype), u.to(dtype), dx0.to(dtype), keep, c)
    return dict(t=t, dx=dx, dA=dA)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
@pytest.mark.parametrize("K,r", [(72, 4), (520, 16), (1536, 8)])
def test_ordinary_operands(K, r, dtype):
    M, p = 1000, 0.1
    x, A, u, dx0 = ordinary(K + r, M, K, r, dtype)
    keep, c = torch.from_numpy(LD.keep_mask(M, K, p, SEED, STREAM)), float(LD.keep_scale(p))
    r64, r32 = reference(x, A, u, dx0, keep, c, F64), reference(x, A, u, dx0, keep, c, F32)
    dev32 = {k: SB.metric(r32[k], r64[k]) for k in r64}
    t = ops.lora_down(x.to(DEV), A.to(DEV), p, SEED, STREAM)
    dx, dA = ops.lora_down_bwd(x.to(DEV), A.to(DEV), u.to(DEV), dx0.to(DEV), p, SEED, STREAM)
    torch.cuda.synchronize()
    fails = []
    for name, got in (("t", t), ("dA", dA), ("dx", dx)):
        m, bar = SB.metric(got, r64[name]), SB.bar(name, dev32, got.dtype == BF)
        print(f"({M}, {K}) r={r} {dtype} {name}: {m:.2e} [bar {bar:.2e}; CPU fp32 restatement {dev32[name]:.2e}]")
        if not m <= bar:
            fails.append((name, m, bar))
    assert not fails
    # dropped elements of dx keep dx0's bits, kept ones (almost surely) moved
    assert G.same_bits(dx.cpu()[~keep], dx0[~keep])
    assert int((dx.cpu()[keep] != dx0[keep]).sum()) > 0.9 * int(keep.sum())


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_single_outputs_strides_poison_and_repeat(dtype):
    M, K, r, p = 131, 520, 8, 0.1
    x, A, u, dx0 = ordinary(3, M, K, r, dtype)
    xd, Ad, ud = x.to(DEV), A.to(DEV), u.to(DEV)
    t = ops.lora_down(xd, Ad, p, SEED, STREAM)
    dx, dA = ops.lora_down_bwd(xd, Ad, ud, dx0.to(DEV), p, SEED, STREAM)
    # one output at a time: the other's bits
    dx_only, none = ops.lora_down_bwd(xd, Ad, ud, dx0.to(DEV), p, SEED, STREAM, want=("dx",))
    assert none is None and G.same_bits(dx_only, dx)
    keepme = dx0.to(DEV)
    none, dA_only = ops.lora_down_bwd(xd, Ad, ud, keepme, p, SEED, STREAM, want=("dA",))
    assert none is None and G.same_bits(dA_only, dA) and G.same_bits(keepme, dx0)                 # dx0 is not touched without "dx"
    none, dA_nodx = ops.lora_down_bwd(xd, Ad, ud, None, p, SEED, STREAM, want=("dA",))
    assert G.same_bits(dA_nodx, dA)
    # poison (0xFF scratch, NaN outputs, sentinels) and a repeat: the same bits
    tp = ops.lora_down(xd, Ad, p, SEED, STREAM, poison=True)
    assert ops.lora_down.guards_ok and G.same_bits(tp, t)
    dxp, dAp = ops.lora_down_bwd(xd, Ad, ud, dx0.to(DEV), p, SEED, STREAM, poison=True)
    assert ops.lora_down_bwd.guards_ok and G.same_bits(dxp, dx) and G.same_bits(dAp, dA)
    dx2, dA2 = ops.lora_down_bwd(xd, Ad, ud, dx0.to(DEV), p, SEED, STREAM)
    assert G.same_bits(dx2, dx) and G.same_bits(dA2, dA) and G.same_bits(ops.lora_down(xd, Ad, p, SEED, STREAM), t)
    # strided x and dx, read and written in place: sentinels in the gaps stay
    xbuf = torch.full((M, K + 32), ops.GUARD, dtype=dtype, device=DEV)
    dbuf = torch.full((M, K + 8), ops.GUARD, dtype=dtype, device=DEV)
    xbuf[:, :K] = xd
    dbuf[:, :K] = dx0.to(DEV)
    xv, dv = xbuf[:, :K], dbuf[:, :K]
    assert ops._lora_rows(xv, "x")[0].data_ptr() == xbuf.data_ptr() and ops._lora_rows(xv, "x")[2] == K + 32
    ts = ops.lora_down(xv, Ad, p, SEED, STREAM)
    dxs, dAs = ops.lora_down_bwd(xv, Ad, ud, dv, p, SEED, STREAM)
    assert dxs.data_ptr() == dbuf.data_ptr()
    assert G.same_bits(ts, t) and G.same_bits(dAs, dA) and G.same_bits(dxs.contiguous(), dx)
    assert bool((xbuf[:, K:] == ops.GUARD).all()) and bool((dbuf[:, K:] == ops.GUARD).all()) and G.same_bits(xbuf[:, :K].contiguous(), xd)
    # a 3-d x [S, L, K] is its S L rows; a stride the kernel cannot take (odd offset) goes through a copy
    x3 = xd[:130].view(2, 65, K)
    assert G.same_bits(ops.lora_down(x3, Ad, p, SEED, STREAM), t[:130])
    odd = torch.zeros((M, K + 1), dtype=dtype, device=DEV)
    odd[:, 1:] = xd
    assert G.same_bits(ops.lora_down(odd[:, 1:], Ad, p, SEED, STREAM), t)
    with pytest.raises(ValueError, match="in place"):
        ops.lora_down_bwd(xd, Ad, ud, odd[:, 1:], p, SEED, STREAM)
    # another stream: other bits
    assert not G.same_bits(ops.lora_down(xd, Ad, p, SEED, STREAM + 1), t)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_no_rows(dtype):
    K, r = 72, 8
    A = torch.randn(r, K, device=DEV)
    x = torch.zeros((0, K), dtype=dtype, device=DEV)
    u = torch.zeros((0, r), device=DEV)
    assert ops.lora_down(x, A, 0.1, 1, 2).shape == (0, r)
    dx, dA = ops.lora_down_bwd(x, A, u, torch.zeros_like(x), 0.1, 1, 2, poison=True)
    assert ops.lora_down_bwd.guards_ok and dx.shape == (0, K) and dA.shape == (r, K) and bool((dA == 0).all())
    assert ops.lora_dropout_mask(0, K, 0.1, 1, 2).shape == (0, K)


def fn_case(dtype, p):
    g = torch.Generator().manual_seed(17)
    S, L, K, N, r, scale = 2, 69, 72, 40, 8, 4.0
    x = torch.randn(S, L, K, generator=g).to(dtype)
    W = (torch.randn(N, K, generator=g) / K ** 0.5).to(dtype)
    A = (torch.rand(r, K, generator=g) * 2 - 1) / K ** 0.5
    B = torch.randn(N, r, generator=g) * 0.05
    dy = torch.randn(S, L, N, generator=g).to(dtype)
    return x, W, A, B, dy, scale


@pytest.mark.parametrize("p", [0.0, 0.1])
@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_linear_fn_against_the_float64_unmerged_graph(dtype, p):
    """p = 0 is the plain unmerged LoRA linear; p = 0.1 takes its mask from the restatement.  y and dx are stored in the model dtype,
    dA and dB in fp32; bars as in test_ordinary_operands."""
    x, W, A, B, dy, scale = fn_case(dtype, p)
    S, L, K = x.shape
    keep, c = torch.from_numpy(LD.keep_mask(S * L, K, p, SEED, STREAM)), float(LD.keep_scale(p))
    refs = []
    for dt in (F64, F32):
        x2, g2 = x.reshape(S * L, K).to(dt), dy.reshape(S * L, -1).to(dt)
        y, _ = LD.linear_forward(x2, W.to(dt), A.to(dt), B.to(dt), scale, keep, c)
        dx, dA, dB = LD.linear_backward(x2, W.to(dt), A.to(dt), B.to(dt), scale, keep, c, g2)
        refs.append(dict(y=y, dx=dx, dA=dA, dB=dB))
    dev32 = {k: SB.metric(refs[1][k], refs[0][k]) for k in refs[0]}
    xd, Ad, Bd = (t.to(DEV).requires_grad_(True) for t in (x, A, B))
    Wd = W.to(DEV)
    y = ops.lora_dropout_linear_fn(xd, Wd, Ad, Bd, scale, p, SEED, STREAM)
    assert type(y.grad_fn).__name__ == "_LoraDropoutLinearFnBackward" and y.dtype == dtype and y.shape == dy.shape
    (y * dy.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    with torch.no_grad():
        plain = ops.lora_dropout_linear_fn(xd, Wd, Ad, Bd, scale, p, SEED, STREAM)
    assert plain.grad_fn is None and G.same_bits(plain, y.detach())
    fails = []
    for name, got in (("y", y.reshape(S * L, -1)), ("dx", xd.grad.reshape(S * L, K)), ("dA", Ad.grad), ("dB", Bd.grad)):
        m, bar = SB.metric(got, refs[0][name]), SB.bar(name, dev32, got.dtype == BF)
        print(f"{dtype} p={p} {name}: {m:.2e} [bar {bar:.2e}; CPU fp32 restatement {dev32[name]:.2e}]")
        if not m <= bar:
            fails.append((name, m, bar))
    assert not fails and Ad.grad.dtype == F32 and Bd.grad.dtype == F32 and xd.grad.dtype == dtype
    # only the factors train (the model's case for the first projection of a frozen trunk): no dx is formed
    A2, B2 = (t.to(DEV).requires_grad_(True) for t in (A, B))
    (ops.lora_dropout_linear_fn(x.to(DEV), Wd, A2, B2, scale, p, SEED, STREAM) * dy.to(DEV)).sum().backward()
    assert G.same_bits(A2.grad, Ad.grad) and G.same_bits(B2.grad, Bd.grad)


def test_limits_raise_value_errors_on_the_device():
    x = torch.zeros(4, 24, device=DEV)
    W = torch.zeros(8, 24, device=DEV)
    for A, B, p, word in ((torch.zeros(3, 24), torch.zeros(8, 3), 0.1, "r must"), (torch.zeros(8, 24), torch.zeros(8, 8), 1.0, "p must")):
        with pytest.raises(ValueError, match=word):
            ops.lora_dropout_linear_fn(x, W, A.to(DEV), B.to(DEV), 4.0, p, 0, 0)
    with pytest.raises(ValueError, match="K must"):
        ops.lora_dropout_linear_fn(torch.zeros(4, 12, device=DEV), torch.zeros(8, 12, device=DEV), torch.zeros(8, 12, device=DEV),
                                   torch.zeros(8, 8, device=DEV), 4.0, 0.1, 0, 0)


@pytest.mark.parametrize("dtype", [BF, F32], ids=["bf16", "fp32"])
def test_saved_tensors_hold_no_mask_and_no_dropped_copy(dtype):
    """under saved_tensors_hooks one call saves at most x, the cast W, A, B and t (+ 1 KiB): distinct storages counted once"""
    x, W, A, B, dy, scale = fn_case(dtype, 0.1)
    xd, Ad, Bd = (t.to(DEV).requires_grad_(True) for t in (x, A, B))
    Wd = W.to(DEV)
    seen = {}

    def pack(t):
        seen[t.untyped_storage().data_ptr()] = t.untyped_storage().nbytes()
        return t
    with torch.autograd.graph.saved_tensors_hooks(pack, lambda t: t):
        y = ops.lora_dropout_linear_fn(xd, Wd, Ad, Bd, scale, 0.1, SEED, STREAM)
    M, K, N, r, e = x.shape[0] * x.shape[1], x.shape[2], W.shape[0], A.shape[0], x.element_size()
    allowed = M * K * e + N * K * e + r * K * 4 + N * r * 4 + M * r * 4 + 1024
    total = sum(seen.values())
    print(f"{dtype}: saved {total} bytes in {len(seen)} storages [allowed {allowed}; x alone {M * K * e}]")
    assert total <= allowed
    (y * dy.to(DEV)).sum().backward()
    assert bool(torch.isfinite(xd.grad).all())
