"""-m gpu: the backward of the pooled classification head (csrc/pool_bwd.hip through include/pcad_bwd.h pcad_pooled_head_bwd,
ops.pooled_head_bwd and the autograd surface ops.pooled_head_fn) against the float64 CPU reference of tests/pool_bwd_ref.py.

Metric, per gradient tensor and over every element: max |got - ref| / max |ref|.  The reference is float64 autograd through the
straight-through restatement; the bar of a tensor is max(BAR_SCAN of the dtype it is stored in, 8 x the same metric of fp32 CPU autograd
through the identical restatement).  bf16 calls: every bf16-stored operand is rounded before the reference sees it, `pooled` is the
forward kernel's own pooled_out (handed to the reference's score head too), bf16-stored dh / dres are held at 2^-7 and the fp32-stored
outputs (dres of the bf16 / fp32 pair, dnorm_weight, dscore_w) at the fp32 bar: no cotangent depends on a rounded forward value other
than pooled, which both sides read.  Every case prints its figures before it asserts.

Shapes, with G = ops.POOL_BWD_SEG: D = 64 (8 of 64 lanes hold a chunk), 384 (a part wave), 1024 (two chunks per lane), 1536 (four chunk
steps, the last a part step); L = 1, G - 1, G, G + 1, 2 G + 5 (segment edges; `last` in another segment than `first`); B = 1, 3;
NL = 1, 2, 5; mean / first / last.

Observed on an MI355X, worst over the cases [bar]: fp32 / fp32 all four gradients 1.5e-7 .. 2.1e-7 [3e-5]; bf16 calls: bf16-stored dh /
dres 3.4e-3 [2^-7 = 7.8e-3], fp32-stored dres 2.3e-7, dnorm_weight 2.2e-7, dscore_w 8.0e-8 [3e-5]."""
import pytest
import torch

import pool_bwd_ref as PB
import scan_bwd_ref as SB

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
G = PB.SEG
KEYS = dict(h="dh", res="dres", norm_weight="dnorm_weight", score_w="dscore_w")

# (D, L, B, NL, pooling)
CASES = [(64, 1, 1, 1, "mean"), (64, G - 1, 3, 2, "mean"), (384, G, 1, 5, "mean"), (384, G + 1, 3, 2, "first"), (384, G + 1, 3, 5, "last"),
         (1024, 2 * G + 5, 1, 2, "mean"), (1024, 2 * G + 5, 3, 5, "last"), (1536, 2 * G + 5, 3, 1, "mean"), (1536, G + 1, 1, 2, "first"),
         (64, 2 * G + 5, 3, 5, "mean"), (64, 1, 3, 2, "last"), (1024, G, 3, 1, "first")]
PAIRS = {"f32": (F32, F32), "bf16_f32": (BF, F32), "bf16_bf16": (BF, BF)}


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    assert _ops.POOL_BWD_SEG == G
    return _ops


def case(D, L, B, NL, pooling, pair="f32"):
    bf, res_bf = pair != "f32", pair == "bf16_bf16"
    return PB.reference((D, L, B, NL, pooling, pair), lambda: PB.inputs(1000 * D + 10 * L + B + NL, B, L, D, NL, pooling, bf=bf, res_bf=res_bf))


def dev(c, pair):
    dt, rdt = PAIRS[pair]
    return dict(h=c["h"].to(DEV, dt), res=c["res"].to(DEV, rdt), norm_weight=c["norm_weight"].to(DEV), score_w=c["score_w"].to(DEV, dt),
                dlogits=c["dlogits"].to(DEV))


def kernel_pooled(ops, c, pair):
    x = dev(c, pair)
    _, pooled = ops.pooled_head(x["h"], x["res"], x["norm_weight"], x["score_w"], c["pooling"], c["eps"], B=c["B"], L=c["L"], want_pooled=True)
    return pooled


def run_bwd(ops, c, pair, pooled=None, **kw):
    x = dev(c, pair)
    pooled = kernel_pooled(ops, c, pair) if pooled is None else pooled
    g = ops.pooled_head_bwd(x["h"], x["res"], x["norm_weight"], x["score_w"], pooled, kw.pop("dlogits", x["dlogits"]), c["pooling"], c["eps"],
                            B=c["B"], L=c["L"], **kw)
    torch.cuda.synchronize()
    return g


def hold(tag, g, ref, bars):
    figs = {k: (SB.metric(getattr(g, KEYS[k]).float().cpu().view(ref[k].shape), ref[k]), bars[k]) for k in PB.NAMES if getattr(g, KEYS[k]) is not None}
    print(tag, " ".join(f"{k} {m:.1e}[{b:.1e}]" for k, (m, b) in figs.items()))
    for k, (m, b) in figs.items():
        assert m <= b, (tag, k, m, b)
    return figs


def silent_rows(c):
    """bool [2B*L]: the rows first / last pooling did not read (mean: none)"""
    m = torch.zeros(2 * c["B"], c["L"], dtype=torch.bool)
    if c["pooling"] != "mean":
        m[:] = True
        m[:, 0 if c["pooling"] == "first" else c["L"] - 1] = False
    return m.view(-1)


@pytest.mark.parametrize("D,L,B,NL,pooling", CASES)
def test_fp32_gradients_against_float64(ops, D, L, B, NL, pooling):
    """all four gradients at the fp32 bar, outputs between intact sentinels, zero rows where first / last did not read.
    Observed worst over the cases: dh / dres 2.1e-7 (D = 1536, L = 133), dnorm_weight 1.7e-7, dscore_w 1.5e-7 [3e-5]"""
    c, g64, dev32 = case(D, L, B, NL, pooling)
    g = run_bwd(ops, c, "f32", poison=True)
    assert g.guards_ok
    assert g.dh.dtype == F32 and g.dres.dtype == F32 and g.dnorm_weight.dtype == F32 and g.dscore_w.dtype == F32
    assert g.dh.shape == (2 * B * L, D) and g.dscore_w.shape == (NL, D) and g.dnorm_weight.shape == (D,)
    hold(f"pool bwd fp32 D={D} L={L} B={B} NL={NL} {pooling}", g, g64, {k: SB.bar(k, dev32, False) for k in PB.NAMES})
    quiet = silent_rows(c).to(DEV)
    assert bool((g.dh[quiet] == 0).all()) and bool((g.dres[quiet] == 0).all())
    assert bool(torch.isfinite(g.dh).all()) and bool(torch.isfinite(g.dscore_w).all()) and bool(torch.isfinite(g.dnorm_weight).all())
    assert torch.equal(g.dh, g.dres)


@pytest.mark.parametrize("pair", ["bf16_f32", "bf16_bf16"])
@pytest.mark.parametrize("D,L,B,NL,pooling", CASES)
def test_bf16_gradients_against_float64(ops, D, L, B, NL, pooling, pair):
    """bf16-stored dh / dres at 2^-7, every fp32-stored output at the fp32 bar; pooled is the forward kernel's own.
    Observed worst over the cases: bf16-stored dh / dres 3.4e-3 (D = 1536, L = 133) [7.8e-3]; fp32-stored dres 2.3e-7, dnorm_weight 2.2e-7,
    dscore_w 8.0e-8 [3e-5]"""
    c, _, dev32 = case(D, L, B, NL, pooling, pair)
    pooled = kernel_pooled(ops, c, pair)
    ref = PB.grads(c, kernel_pooled=pooled.cpu())
    g = run_bwd(ops, c, pair, pooled=pooled, poison=True)
    assert g.guards_ok
    assert g.dh.dtype == BF and g.dres.dtype == PAIRS[pair][1] and g.dnorm_weight.dtype == F32 and g.dscore_w.dtype == F32
    stored_bf = dict(h=True, res=PAIRS[pair][1] == BF, norm_weight=False, score_w=False)
    hold(f"pool bwd {pair} D={D} L={L} B={B} NL={NL} {pooling}", g, ref, {k: SB.bar(k, dev32, stored_bf[k]) for k in PB.NAMES})
    quiet = silent_rows(c).to(DEV)
    assert bool((g.dh[quiet] == 0).all()) and bool((g.dres[quiet] == 0).all())


@pytest.mark.parametrize("pair", ["f32", "bf16_f32"])
def test_reproducible_and_inside_its_bounds(ops, pair):
    """two calls agree bit for bit, and so does a call whose scratch starts as 0xFF bytes and whose outputs start as NaN between
    sentinel rows, which stay intact"""
    c, _, _ = case(1536, 2 * G + 5, 3, 5, "mean", pair)
    pooled = kernel_pooled(ops, c, pair)
    a, b, p = run_bwd(ops, c, pair, pooled), run_bwd(ops, c, pair, pooled), run_bwd(ops, c, pair, pooled, poison=True)
    assert p.guards_ok
    for k in KEYS.values():
        assert torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(getattr(a, k), getattr(p, k)), k


@pytest.mark.parametrize("pooling", ["mean", "last"])
def test_each_output_null_in_turn(ops, pooling):
    """leaving one output out leaves the others bit-equal; what was not asked for is None; a single output alone too"""
    c, _, _ = case(384, G + 1, 3, 2, pooling)
    pooled = kernel_pooled(ops, c, "f32")
    full = run_bwd(ops, c, "f32", pooled)
    names = tuple(KEYS.values())
    for skip in names:
        g = run_bwd(ops, c, "f32", pooled, want=tuple(k for k in names if k != skip), poison=True)
        assert g.guards_ok and getattr(g, skip) is None
        assert all(torch.equal(getattr(g, k), getattr(full, k)) for k in names if k != skip), skip
    for only in names:
        g = run_bwd(ops, c, "f32", pooled, want=(only,), poison=True)
        assert g.guards_ok and torch.equal(getattr(g, only), getattr(full, only)) and all(getattr(g, k) is None for k in names if k != only), only


def test_independent_of_the_batch(ops):
    """a window's rows of dh do not depend on the batch it runs in (the segmentation depends on L only): window 2 alone against inside B = 3"""
    c, _, _ = case(1024, 2 * G + 5, 3, 5, "mean")
    B, L, D = 3, c["L"], 1024
    full = run_bwd(ops, c, "f32").dh.view(2 * B, L, D)
    b = 2
    pick = lambda t: t.view(2 * B, L, D)[[b, B + b]].reshape(2 * L, D)
    alone = dict(c, h=pick(c["h"]), res=pick(c["res"]), dlogits=c["dlogits"][b:b + 1], B=1)
    got = run_bwd(ops, alone, "f32").dh.view(2, L, D)
    assert torch.equal(got[0], full[b]) and torch.equal(got[1], full[B + b])


@pytest.mark.parametrize("pooling", PB.POOLINGS)
def test_zero_cotangent_gives_exact_zeros(ops, pooling):
    c, _, _ = case(384, G + 1, 3, 2, pooling)
    g = run_bwd(ops, c, "f32", dlogits=torch.zeros_like(c["dlogits"]).to(DEV), poison=True)
    assert g.guards_ok
    assert all(bool((getattr(g, k) == 0).all()) for k in KEYS.values())


def test_autograd_surface(ops):
    """ops.pooled_head_fn: the plain call without grad, bit for bit pcad_pooled_head; with grad each gradient in its input's shape and
    dtype at the fp32 bar; a gradient nobody needs is not computed; with a bf16 trunk an fp32 score_w receives the kernel's fp32 dscore_w bit
    for bit (straight through its rounding to the model dtype); max pooling is refused with grad only"""
    D, L, B, NL = 384, G + 1, 3, 5
    c, g64, dev32 = case(D, L, B, NL, "mean")
    x = dev(c, "f32")
    args = lambda t: (t["h"].view(2 * B, L, D), t["res"].view(2 * B, L, D), t["norm_weight"], t["score_w"])
    ref_lg = ops.pooled_head(x["h"], x["res"], x["norm_weight"], x["score_w"], "mean", c["eps"], B=B, L=L)
    plain = ops.pooled_head_fn(*args(x), "mean", c["eps"])
    assert plain.grad_fn is None and not plain.requires_grad and plain.dtype == F32 and plain.shape == (B, NL) and torch.equal(plain, ref_lg)
    assert torch.equal(ops.pooled_head_fn(x["h"], x["res"], x["norm_weight"], x["score_w"], "mean", c["eps"], B=B, L=L), ref_lg)
    lv = dict(x, **{k: x[k].clone().requires_grad_(True) for k in PB.NAMES})
    with torch.no_grad():
        assert ops.pooled_head_fn(*args(lv), "mean", c["eps"]).grad_fn is None
    lg = ops.pooled_head_fn(*args(lv), "mean", c["eps"])
    assert lg.requires_grad and torch.equal(lg.detach(), ref_lg)
    (lg * x["dlogits"]).sum().backward()
    torch.cuda.synchronize()
    from types import SimpleNamespace
    got = SimpleNamespace(**{KEYS[k]: lv[k].grad for k in PB.NAMES})
    for k in PB.NAMES:
        assert lv[k].grad.shape == lv[k].shape and lv[k].grad.dtype == lv[k].dtype, k
    hold("pooled_head_fn fp32", got, g64, {k: SB.bar(k, dev32, False) for k in PB.NAMES})
    # only score_w requires grad (the frozen-trunk mode): dh, dres and dnorm_weight are not computed
    only = dict(x, score_w=x["score_w"].clone().requires_grad_(True))
    ops.pooled_head_bwd.last_outputs = ()
    ops.pooled_head_fn(*args(only), "mean", c["eps"]).sum().backward()
    assert ops.pooled_head_bwd.last_outputs == ("dscore_w",) and only["score_w"].grad is not None
    # bf16 trunk, fp32 score: the gradients come back in their inputs' dtypes
    xb = dev(c, "bf16_f32")
    lb = dict(h=xb["h"].clone().requires_grad_(True), res=xb["res"].clone().requires_grad_(True),
              norm_weight=xb["norm_weight"].to(BF).requires_grad_(True), score_w=c["score_w"].to(DEV).requires_grad_(True))
    ops.pooled_head_fn(*args(lb), "first", c["eps"]).sum().backward()
    assert lb["h"].grad.dtype == BF and lb["res"].grad.dtype == F32 and lb["norm_weight"].grad.dtype == BF and lb["score_w"].grad.dtype == F32
    assert lb["score_w"].grad.shape == (NL, D) and bool(torch.isfinite(lb["score_w"].grad).all())
    # ... and the fp32 score's gradient is straight-through: the kernel's fp32 dscore_w bit for bit, not its image in the model dtype
    nw = lb["norm_weight"].detach()                   # the bf16 norm weight of the call above: the same operands, through the raw wrappers
    _, pooled = ops.pooled_head(xb["h"], xb["res"], nw, lb["score_w"].detach(), "first", c["eps"], B=B, L=L, want_pooled=True)
    raw = ops.pooled_head_bwd(xb["h"], xb["res"], nw, lb["score_w"].detach(), pooled, torch.ones(B, NL, device=DEV), "first", c["eps"],
                              B=B, L=L, want=("dscore_w",))
    assert torch.equal(lb["score_w"].grad, raw.dscore_w)
    assert not torch.equal(raw.dscore_w, raw.dscore_w.to(BF).float())         # which a cast pair in the graph would have made of it
    for pooling in ("mean", "first"):                                          # and at the fp32 bar against the float64 reference
        cb, _, dev32b = case(D, L, B, NL, pooling, "bf16_f32")
        xs = dev(cb, "bf16_f32")
        sw = cb["score_w"].to(DEV).requires_grad_(True)                        # fp32 (bf16-representable values), as the model holds it
        pooled = kernel_pooled(ops, cb, "bf16_f32")
        (ops.pooled_head_fn(xs["h"].view(2 * B, L, D), xs["res"].view(2 * B, L, D), xs["norm_weight"], sw, pooling, cb["eps"]) * xs["dlogits"]).sum().backward()
        m, bar = SB.metric(sw.grad, PB.grads(cb, kernel_pooled=pooled.cpu())["score_w"]), SB.bar("score_w", dev32b, False)
        print(f"pooled_head_fn bf16 trunk, fp32 score ({pooling}): dscore_w {m:.1e}[{bar:.1e}]")
        assert sw.grad.dtype == F32 and m <= bar
    # max pooling: the forward alone
    assert ops.pooled_head_fn(*args(x), "max", c["eps"]).shape == (B, NL)
    with pytest.raises(NotImplementedError, match="max"):
        ops.pooled_head_fn(*args(lv), "max", c["eps"])
