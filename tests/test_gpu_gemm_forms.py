"""-m gpu: the three persistent GEMM kernels of csrc/gemm.hip in the launch forms the ENGINE runs (csrc/forward.hip), through the operator
entries pcad_gemm_nt_engine / pcad_gemm_nt_xproj / pcad_gemm_nt_two / pcad_gemm_nt_residual_engine, against the float64 products of
tests/gemm_ref.py.

Method (gemm_ref.py): integer operands in {-3 .. 3} make every product and partial sum exact in fp32, so each EXACT case holds the
kernel's output bit-equal to the float64 product rounded once to the stored dtype - whatever the summation order.  Each exact case
also asserts: no NaN left in the (NaN-filled) outputs, guards before and after every output intact, padding rows of blocked outputs
untouched, a second call gives the same bits, and the blocked launch equals its plain-layout twin bit for bit.  Hand-over cases take
the persistent grid (multi_processor_count // 8 * 8) from the device and assert tiles > grid first.

Which kernel each case runs is derived from the dispatch rules restated in tests/launch_forms.py (gemm_kernel) and asserted:
  NT  = gemm_nt_kernel<T, OutT, ., VEC, SPLIT>   256 x 128 tiles, 8 waves, one 3-stage ring
  Q   = gemm256q_kernel<T, OutT, EPI>            256 x 256 tiles, 4 waves (whole tiles only); EPI_SCALE (rscale) / EPI_RES (residual)
  R   = gemm256r_kernel<T, OutT>                 256 x 256 tiles, 8 waves (edge tiles)

  case                      engine launch it stands for (csrc/forward.hip)                          kernel
  test_xproj_exact          x_proj: launch_gemm_nt_split, blocked A (xc), C = dt_low, C2 = B | C    NT <T, T, ., true, SPLIT>; N = 96: ragged N
                            tile with clamped W rows; M = 37, 300: ragged, padded blocked buffer
  test_xproj_handover       the same with 258 m-tiles (the last of 37 rows) on one n-tile           NT; 1 K-tile: the ring spans 3 output tiles
  test_plain_exact          out_proj: launch_gemm_nt, a_blocked (the scan's y)                       (300, 384) NT; (2100, 528) R; (2048, 512) Q;
                                                                                                    hand-over (33 280, 512) Q 260 tiles,
                                                                                                    (33 300, 528) R 393 tiles
  test_plain_split_exact    out_proj under "f32_gemm_split": ksplit on a blocked [hi | lo] y        (2048, 512) Q <bf16, float>; (300, 384) NT <bf16, float>
  test_residual_exact       out_proj under "norm_fold": launch_gemm_nt_res, a_blocked                Q EPI_RES; (66 048, 512): 516 tiles
  test_two_quad_exact       in_proj: launch_gemm_nt_two, two blocked outputs, lda > K;               Q EPI_NONE / EPI_SCALE, <bf16, float> with ksplit;
                            rscale = the "norm_fold" in_proj; split = the fp32 model's              nsplit 128 of 256: on the wave boundary; 192 of
                            "f32_gemm_split" in_proj (bf16 [hi | lo] -> fp32)                       512: inside a wave
  test_two_quad_handover    the same at (8448, 2048, 1024): 264 tiles                               Q EPI_SCALE (1 and 3 K-tiles); Q <bf16, float> ksplit
  test_two_ring_exact       in_proj on shapes that are not whole tiles (generic geometries)          R; (2100, 384, 192): ragged M, half-empty n-tile;
                                                                                                    (40, 176, 80): a split off the 64-column groups
  test_random_*             every form and dtype once on ordinary values, at the project's bars
  test_the_exact_comparison_sees_a_wrong_operand   controls: a wrong operand handed to the same launches differs on > 99 % of the elements
  test_refusals             what the launchers reject comes back as PCAD_ERR_INVALID and nothing is written

Bars of the random cases (max |got - ref| / max |ref| against float64 of the rounded operands; tests/test_gpu_ops.py): fp32 2e-6;
bf16 -> fp32 1e-5; bf16 stored: equal to the rounded fp32 result, or 2^-8; x_proj C2: 2^-7 (bf16) / 3e-5 (fp32).
Observed on an MI355X (the figure each random case prints) [bar]:
  x_proj     bf16: C 1.7e-3 [2^-8 = 3.9e-3], C2 2.1e-3 [2^-7 = 7.8e-3]        fp32: C 3.3e-7 [2e-6], C2 3.3e-7 [3e-5]
  plain      bf16 -> fp32 1.9e-7 [1e-5]; bf16 stored: equal to the rounded fp32 result (2.6e-3 of max)
             fp32 3.7e-7 [2e-6]        split (bf16 [hi | lo] -> fp32, 8-wave kernel) 3.6e-7 [1e-5]
  residual   bf16: res 3.4e-7 [1e-5], ssq 1.6e-7 [1e-5]        fp32: res 6.5e-7 [2e-6], ssq 1.6e-7 [1e-5]; C == round(res) in both
  two        4-wave with rscale: bf16 1.9e-3 [2^-8], fp32 3.6e-7 [2e-6]        split 3.0e-7 [1e-5]
             8-wave: bf16 -> fp32 2.0e-7 [1e-5]; bf16 stored: equal to the rounded fp32 result (3.0e-3 of max)
Every integer case was bit-equal on the first run; no kernel change was needed.
"""
import ctypes as C

import pytest
import torch

import gemm_ref as G
import launch_forms as F
from scan_ref import split_hi_lo

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
ESZ = {BF: 2, F32: 4}
DTYPES = [BF, F32]
DID = ["bf16", "fp32"]
NT, Q, R = F.GEMM_NT, F.GEMM_256Q, F.GEMM_256R


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


@pytest.fixture(scope="module")
def cus():
    return torch.cuda.get_device_properties(0).multi_processor_count


def kcols(dt, tiles):
    """K of `tiles` K-tiles: 128 bytes of K per tile row"""
    return tiles * F.GEMM_ROWB // ESZ[dt]


def exact(name, got, want):
    got = got.cpu()
    assert not torch.isnan(got.float()).any(), f"{name}: NaN left where the kernel must write"
    if not G.same_bits(got, want):
        bad = got.float() != want.float()
        rows, cols = bad.any(1).nonzero().flatten(), bad.any(0).nonzero().flatten()
        pytest.fail(f"{name}: {int(bad.sum())} of {bad.numel()} elements differ from the float64 product; rows {rows[:6].tolist()} .. "
                    f"{rows[-6:].tolist()} ({rows.numel()}), columns {cols[:6].tolist()} .. {cols[-6:].tolist()} ({cols.numel()})")


def check_exact(name, run, want, twin=None):
    """run() -> dict of outputs (it asserts its own guards); want: dict of expected CPU tensors in the stored dtype"""
    got = run()
    for k, w in want.items():
        exact(f"{name} {k}", got[k], w)
    again = run()
    for k in want:
        assert G.same_bits(again[k], got[k]), f"{name} {k}: a second call gives other bits"
    if twin is not None:
        t = twin()
        for k in want:
            assert G.same_bits(t[k], got[k]), f"{name} {k}: the plain-layout twin of the launch gives other bits"
    return got


def assert_handover(cus, kernel, M, N):
    tiles, grid = F.gemm_tiles(kernel, M, N), cus // 8 * 8
    assert tiles > grid, f"{tiles} tiles on a grid of {grid}: no block walks a second tile on this device"
    return tiles


def gpu(t, dt):
    return t.to(dt).to(DEV)


# ---- runners: one launch -> its outputs on the CPU ------------------------------------------------------------------------------------
def run_xproj(ops, a, w, nsplit, dt, blocked):
    r = ops.gemm_nt_xproj(gpu(a, dt), gpu(w, dt), nsplit, a_blocked=blocked)
    assert r.guards_ok, "x_proj form: a guard was written"
    return dict(c=r.c.cpu(), c2=r.c2.cpu())


def run_plain(ops, a, w, dt, blocked, out_dt=None, K=None, ksplit=0):
    r = ops.gemm_nt_engine(gpu(a, dt), gpu(w, dt), K=K, a_blocked=blocked, ksplit=ksplit, out_dtype=out_dt)
    assert r.guards_ok, "plain form: a guard was written"
    return dict(c=r.c.cpu())


def run_residual(ops, a, w, res, dt, blocked):
    r = ops.gemm_nt_residual_engine(gpu(a, dt), gpu(w, dt), res.to(DEV), a_blocked=blocked)
    assert r.guards_ok, "residual form: a guard was written"
    return dict(res=r.res.cpu(), c=r.c.cpu(), ssq=r.ssq.cpu())


def run_two(ops, a, w, nsplit, dt, blocked, rscale=None, out_dt=None, K=None, ksplit=0, lda_extra=64):
    r = ops.gemm_nt_two(gpu(a, dt), gpu(w, dt), nsplit, K=K, out_blocked=blocked, rscale=None if rscale is None else rscale.to(DEV),
                        ksplit=ksplit, out_dtype=out_dt, lda_extra=lda_extra)
    assert r.guards_ok, "two form: a guard was written"
    for p in (r.pad1, r.pad2):
        assert torch.isnan(p.float()).all(), "two form: a padding row of a blocked output was written"
    if blocked:
        assert r.pad1.shape[0] == (-a.shape[0]) % 8
    return dict(c1=r.c1.cpu(), c2=r.c2.cpu())


def want_two(ref, nsplit, dt):
    return dict(c1=G.stored(ref[:, :nsplit], dt), c2=G.stored(ref[:, nsplit:], dt))


# ---- group 1: the x_proj form -----------------------------------------------------------------------------------------------------------
def xproj_case(ops, dt, M, N, nsplit, ktiles):
    K = kcols(dt, ktiles)
    a, w = G.ints(M + K, M, K), G.ints(N + K, N, K)
    ref = G.product(a, w)
    assert F.gemm_kernel("xproj", M, N, ESZ[dt], K, K) == NT
    want = dict(c=G.stored(ref[:, :nsplit], dt), c2=G.c2_of(ref[:, nsplit:], dt))
    check_exact(f"x_proj {dt} M={M} N={N} nsplit={nsplit} K-tiles={ktiles} blocked A", lambda: run_xproj(ops, a, w, nsplit, dt, True), want,
                twin=lambda: run_xproj(ops, a, w, nsplit, dt, False))


@pytest.mark.parametrize("N,nsplit", [(96, 64), (128, 96)])
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_xproj_exact(ops, dt, N, nsplit):
    for M in (37, 300):
        xproj_case(ops, dt, M, N, nsplit, 3)


@pytest.mark.parametrize("ktiles", [1, 3])
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_xproj_handover(ops, cus, dt, ktiles):
    M, N = 65829, 96
    assert assert_handover(cus, NT, M, N) == 258 and M % 256 == 37
    xproj_case(ops, dt, M, N, 64, ktiles)


# ---- group 2: the plain form with a blocked A ------------------------------------------------------------------------------------------
PLAIN = [(300, 384, 2, NT, False), (2100, 528, 1, R, False), (2100, 528, 3, R, False), (2048, 512, 1, Q, False), (2048, 512, 3, Q, False),
         (33280, 512, 1, Q, True), (33300, 528, 1, R, True)]


@pytest.mark.parametrize("M,N,ktiles,kernel,handover", PLAIN, ids=lambda v: str(v).split(" ")[0])
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_plain_exact(ops, cus, dt, M, N, ktiles, kernel, handover):
    K = kcols(dt, ktiles)
    assert F.gemm_kernel("plain", M, N, ESZ[dt], K, K) == kernel
    if handover:
        assert assert_handover(cus, kernel, M, N) == {33280: 260, 33300: 393}[M]
    a, w = G.ints(M + N, M, K), G.ints(M + N + 1, N, K)
    want = dict(c=G.stored(G.product(a, w), dt))
    check_exact(f"plain {dt} ({M}, {N}) K-tiles={ktiles} blocked A", lambda: run_plain(ops, a, w, dt, True), want,
                twin=lambda: run_plain(ops, a, w, dt, False))


@pytest.mark.parametrize("Ko", [64, 192])
@pytest.mark.parametrize("M,N,kernel", [(2048, 512, Q), (300, 384, NT)])
def test_plain_split_exact(ops, M, N, kernel, Ko):
    """hi and lo are independent integer matrices, so each of the three products and the order of the parts shows"""
    assert F.gemm_kernel("plain", M, N, 2, 2 * Ko, 2 * Ko, osz=4) == kernel
    a2, w2 = G.ints(M + Ko, M, 2 * Ko), G.ints(N + Ko, N, 2 * Ko)
    want = dict(c=G.stored(G.split_product(a2, w2, Ko), F32))
    kw = dict(out_dt=F32, K=3 * Ko, ksplit=Ko // 64)
    check_exact(f"plain split ({M}, {N}) Ko={Ko} blocked [hi | lo] A", lambda: run_plain(ops, a2, w2, BF, True, **kw), want,
                twin=lambda: run_plain(ops, a2, w2, BF, False, **kw))


# ---- group 3: the residual form with a blocked A ---------------------------------------------------------------------------------------
@pytest.mark.parametrize("M,N,ktiles", [(256, 256, 1), (2304, 768, 3), (66048, 512, 2)])
@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_residual_exact(ops, cus, dt, M, N, ktiles):
    K = kcols(dt, ktiles)
    assert F.gemm_kernel("residual", M, N, ESZ[dt], K, K) == Q
    if M == 66048:
        assert assert_handover(cus, Q, M, N) == 516
    # W in {-1, 0, 1}: |new residual| <= 3 + 3 K stays far below the 361 at which a 128-column sum of squares leaves the exact range
    a, w, res = G.ints(M + K, M, K), G.ints(N + K, N, K, r=1), G.ints(M + N, M, N)
    ref = res.double() + G.product(a, w)
    assert 128 * float(ref.abs().max()) ** 2 < 2 ** 24
    want = dict(res=G.stored(ref, F32), c=G.stored(ref, dt), ssq=G.stored(G.ssq_of(ref), F32))
    check_exact(f"residual {dt} ({M}, {N}) K-tiles={ktiles} blocked A", lambda: run_residual(ops, a, w, res, dt, True), want,
                twin=lambda: run_residual(ops, a, w, res, dt, False))


# ---- groups 4 and 5: the two form --------------------------------------------------------------------------------------------------------
def two_case(ops, variant, M, N, nsplit, ktiles, kernel, rscale=False, twin=True, blocked=True, Ko=128):
    """variant: bf16 / fp32 (ktiles K-tiles, A rows K + 64 elements apart) or "split" (bf16 [hi | lo] of Ko columns each -> fp32)"""
    if variant == "split":
        dt, out_dt, K, cols, ks = BF, F32, 3 * Ko, 2 * Ko, Ko // 64
    else:
        dt = out_dt = variant
        K = cols = kcols(dt, ktiles)
        ks = 0
    assert F.gemm_kernel("two", M, N, ESZ[dt], cols + 64, cols, osz=ESZ[out_dt], nsplit=nsplit, epilogue=rscale) == kernel
    a, w = G.ints(M + nsplit, M, cols), G.ints(N + nsplit, N, cols)
    ref = G.split_product(a, w, Ko) if variant == "split" else G.product(a, w)
    rs = G.rscale(M) if rscale else None
    if rscale:
        ref = ref * rs.double()[:, None]
    kw = dict(rscale=rs, out_dt=out_dt, K=K, ksplit=ks)
    name = f"two {variant} ({M}, {N}, {nsplit}) K={K}{' rscale' if rscale else ''} {'blocked' if blocked else 'plain'} outputs"
    check_exact(name, lambda: run_two(ops, a, w, nsplit, dt, blocked, **kw), want_two(ref, nsplit, out_dt),
                twin=(lambda: run_two(ops, a, w, nsplit, dt, False, **kw)) if twin else None)


VARIANTS = [BF, F32, "split"]
VID = ["bf16", "fp32", "split"]


QUAD = [(v, s, r) for v in VARIANTS for s in ((256, 256, 128), (512, 512, 192)) for r in (False, True) if not (v == "split" and r)]


@pytest.mark.parametrize("variant,shape,rscale", QUAD, ids=[f"{VID[VARIANTS.index(v)]}-{s[0]}-{s[2]}{'-rscale' if r else ''}" for v, s, r in QUAD])
def test_two_quad_exact(ops, variant, shape, rscale):
    """(256, 256, 128): the split falls on the wave boundary inside one tile; (512, 512, 192): inside a wave, unequal halves.  split with
    rscale is no launch (the launcher refuses it)"""
    two_case(ops, variant, *shape, 3, Q, rscale=rscale)


@pytest.mark.parametrize("variant,ktiles", [(BF, 1), (BF, 3), (F32, 1), (F32, 3), ("split", 3)],
                         ids=["bf16-1", "bf16-3", "fp32-1", "fp32-3", "split-Ko64"])
def test_two_quad_handover(ops, cus, variant, ktiles):
    M, N, nsplit = 8448, 2048, 1024
    assert assert_handover(cus, Q, M, N) == 264
    two_case(ops, variant, M, N, nsplit, ktiles, Q, rscale=variant != "split", Ko=64)


@pytest.mark.parametrize("variant", VARIANTS, ids=VID)
def test_two_ring_exact(ops, variant):
    two_case(ops, variant, 2100, 384, 192, 2, R, Ko=64)         # ragged M, M % 8 != 0; the second n-tile is half empty
    if variant != "split":
        two_case(ops, variant, 40, 176, 80, 2, R, twin=False, blocked=False)      # 80 columns: no blocked form


def test_the_exact_comparison_sees_a_wrong_operand(ops):
    """Controls: the launches of the exact cases with one operand wrong on purpose - W's [hi | lo] halves exchanged, the rscale of the
    next row, A's rows rotated inside their 8-row blocks - differ from the expected tensors on at least half of the elements (the
    condition tests/test_gemm_forms.py puts on the inputs, here through the whole path: wrappers, layouts, kernels, comparison)."""
    def share(got, want):
        return (got.float() != want.float()).double().mean().item()
    M, N, nsplit, Ko = 512, 512, 192, 128
    a2, w2 = G.ints(M + nsplit, M, 2 * Ko), G.ints(N + nsplit, N, 2 * Ko)
    want = want_two(G.split_product(a2, w2, Ko), nsplit, F32)
    bad = run_two(ops, a2, torch.cat([w2[:, Ko:], w2[:, :Ko]], 1), nsplit, BF, True, out_dt=F32, K=3 * Ko, ksplit=Ko // 64)
    a, w = G.ints(1, M, 192), G.ints(2, N, 192)
    rs = G.rscale(M + 1)
    want_rs = want_two(G.product(a, w) * rs[:M].double()[:, None], nsplit, BF)
    bad_rs = run_two(ops, a, w, nsplit, BF, True, rscale=rs[1:])
    want_rot = G.stored(G.product(a, w), BF)
    bad_rot = run_plain(ops, G.rows_rotated(a), w, BF, True)["c"]
    shares = dict(w_halves=min(share(bad[k], want[k]) for k in want), rscale=min(share(bad_rs[k], want_rs[k]) for k in want_rs),
                  rows=share(bad_rot, want_rot))
    print("controls: share of elements that differ:", {k: f"{v:.3f}" for k, v in shares.items()})
    assert all(v >= 0.5 for v in shares.values()), shares


# ---- ordinary values at the project's bars ---------------------------------------------------------------------------------------------
def figure(name, got, ref, bar):
    assert not torch.isnan(got.float()).any(), f"{name}: NaN left where the kernel must write"
    e = G.relerr(got, ref)
    print(f"{name}: {e:.2e} (bar {bar:.2e})")
    assert e < bar, f"{name}: {e:.3e} >= bar {bar:.3e}"


def stored_or(name, got, got32, ref, bar=2.0 ** -8):
    """a bf16 output: the rounded fp32 result of the same launch, or within 2^-8"""
    same = torch.equal(got, got32.to(BF))
    print(f"{name}: {'equal to the rounded fp32 result' if same else 'not the rounded fp32 result'}; {G.relerr(got, ref):.2e} (bar {bar:.2e})")
    assert same or G.relerr(got, ref) < bar


BAR32 = {BF: 1e-5, F32: 2e-6}                       # an fp32 result of bf16 / fp32 operands


def split_pair(seed, M, N, Ko):
    g = torch.Generator().manual_seed(seed)
    x, w = torch.randn(M, Ko, generator=g), torch.randn(N, Ko, generator=g) / Ko ** 0.5
    return torch.cat(split_hi_lo(x), 1).float(), torch.cat(split_hi_lo(w), 1).float()


@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_random_xproj(ops, dt):
    M, N, nsplit = 300, 128, 96
    a, w = G.randn_pair(1, M, N, kcols(dt, 3), dt)
    ref = G.product(a, w)
    o = run_xproj(ops, a, w, nsplit, dt, True)
    figure(f"random x_proj {dt} C", o["c"], ref[:, :nsplit], 2.0 ** -8 if dt == BF else 2e-6)
    figure(f"random x_proj {dt} C2", o["c2"], ref[:, nsplit:], 2.0 ** -7 if dt == BF else 3e-5)
    assert torch.equal(o["c2"], o["c2"].to(dt).float())           # C2 holds values of the model dtype


@pytest.mark.parametrize("variant", VARIANTS, ids=VID)
def test_random_plain(ops, variant):
    M, N = 2100, 528
    if variant == "split":
        a, w = split_pair(2, M, N, 192)
        figure("random plain split", run_plain(ops, a, w, BF, True, out_dt=F32, K=576, ksplit=3)["c"], G.split_product(a, w, 192), 1e-5)
        return
    a, w = G.randn_pair(2, M, N, kcols(variant, 3), variant)
    ref = G.product(a, w)
    o32 = run_plain(ops, a, w, variant, True, out_dt=F32)["c"]
    figure(f"random plain {variant} -> fp32", o32, ref, BAR32[variant])
    if variant == BF:
        stored_or("random plain bf16 stored", run_plain(ops, a, w, BF, True)["c"], o32, ref)


@pytest.mark.parametrize("dt", DTYPES, ids=DID)
def test_random_residual(ops, dt):
    M, N = 2304, 768
    a, w = G.randn_pair(3, M, N, kcols(dt, 3), dt)
    res = torch.randn(M, N, generator=torch.Generator().manual_seed(4)) * 3
    o = run_residual(ops, a, w, res, dt, True)
    figure(f"random residual {dt} res", o["res"], res.double() + G.product(a, w), BAR32[dt])
    assert torch.equal(o["c"], o["res"].to(dt)), "C is not the new residual rounded once"
    figure(f"random residual {dt} ssq", o["ssq"], G.ssq_of(o["res"].double()), 1e-5)


@pytest.mark.parametrize("variant", VARIANTS, ids=VID)
def test_random_two(ops, variant):
    M, N, nsplit = 512, 512, 192
    if variant == "split":
        a, w = split_pair(5, M, N, 128)
        o = run_two(ops, a, w, nsplit, BF, True, out_dt=F32, K=384, ksplit=2)
        figure("random two split", torch.cat([o["c1"], o["c2"]], 1), G.split_product(a, w, 128), 1e-5)
        return
    a, w = G.randn_pair(5, M, N, kcols(variant, 3), variant)
    rs = torch.rand(M, generator=torch.Generator().manual_seed(6)) * 1.5 + 0.5           # like a row's rstd
    o = run_two(ops, a, w, nsplit, variant, True, rscale=rs)
    ref = G.product(a, w) * rs.double()[:, None]
    figure(f"random two {variant} rscale", torch.cat([o["c1"], o["c2"]], 1), ref, 2.0 ** -8 if variant == BF else 2e-6)
    if variant == BF:                     # the 8-wave kernel, where the same launch has an fp32 twin
        M, N, nsplit = 2100, 384, 192
        a, w = G.randn_pair(7, M, N, 192, BF)
        ref = G.product(a, w)
        o32 = run_two(ops, a, w, nsplit, BF, True, out_dt=F32)
        o = run_two(ops, a, w, nsplit, BF, True)
        figure("random two bf16 -> fp32 (8-wave)", torch.cat([o32["c1"], o32["c2"]], 1), ref, 1e-5)
        stored_or("random two bf16 stored (8-wave)", torch.cat([o["c1"], o["c2"]], 1), torch.cat([o32["c1"], o32["c2"]], 1), ref)


# ---- refusals ----------------------------------------------------------------------------------------------------------------------------
def test_refusals(ops):
    """PCAD_ERR_INVALID from each entry, and every output buffer still holds its NaN afterwards"""
    from plantcaduceus_amd import engine
    lib = engine.load_library()
    a = torch.zeros(512 * 512, dtype=BF, device=DEV)
    w = torch.zeros(512 * 512, dtype=BF, device=DEV)
    rs = torch.ones(512, device=DEV)
    outs = [torch.full((512 * 512,), float("nan"), device=DEV) for _ in range(3)]
    p = dict(A=a.data_ptr(), W=w.data_ptr(), C=outs[0].data_ptr(), C2=outs[1].data_ptr(), C3=outs[2].data_ptr(), rscale=rs.data_ptr())
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    calls = G.refusals(p, device=True)
    assert len(calls) == 7
    for why, fn, args in calls:
        rc = getattr(lib, fn)(*args, stream)
        assert rc == -1, f"{why}: {fn} returned {rc} ({lib.pcad_last_error()})"
    torch.cuda.synchronize()
    for o in outs:
        assert torch.isnan(o).all(), "a refused call wrote to an output"
    # the same calls with the one offending argument put right are launches: it was that argument that was refused
    for fn, args in G.accepted_twins(p):
        assert getattr(lib, fn)(*args, stream) == 0, (fn, lib.pcad_last_error())
    torch.cuda.synchronize()
