"""-m gpu: the backward of the masked-LM loss head (csrc/loss_bwd.hip through include/pcad_bwd.h pcad_loss_head_bwd, ops.loss_head_bwd and
the autograd surface ops.mlm_loss_head_fn) against the float64 CPU reference of tests/head_bwd_ref.py.

Metric, per gradient tensor and over every element: max |got - ref| / max |ref|.  fp32 / fp32: all four gradients against the float64
autograd gradient, bar max(3e-5, 8 x the same metric of fp32 CPU autograd through the identical restatement).  bf16 calls: every
bf16-stored operand is rounded before the reference sees it, and the reference is the float64 vector-Jacobian product of the
straight-through head graph whose cotangent is formed in float64 from the FORWARD KERNEL'S OWN logits (a one-ulp flip of a bf16 logit
would otherwise move the softmax by more than any bar); all four tensors take the bf16 figure 2^-7, because each passes through o and
the logits, which the forward rounded to bf16.  Every case prints its figures before it asserts.

Shapes, with G = ops.LOSS_SEG: D = 64 (8 of 64 lanes hold a chunk), 384 (a part wave), 1024 (two chunks per lane), 1536 (four chunk
steps, the last a part step); L = 1, G - 1, G, G + 1, 2 G + 5 (segment edges; the rc row L-1-t in another segment than t); B = 1, 3.

Observed on an MI355X, worst over the cases [bar]: fp32 / fp32 all four gradients 1.0e-7 .. 4.1e-7 [3e-5]; bf16 calls: bf16-stored dh /
dres 1.6e-3 .. 3.3e-3, fp32-stored dres 1.7e-7, dnorm_weight 3.5e-7, demb 9.2e-4 (one o a bf16 ulp apart between the kernel's fp32 product
and the reference's rounded float64 one) [2^-7 = 7.8e-3]."""
import pytest
import torch

import head_bwd_ref as HB
import scan_bwd_ref as SB
import scan_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
G = HB.SEG
KEYS = dict(h="dh", res="dres", norm_weight="dnorm_weight", emb="demb")

# (D, L, B, labels, loss_weights, dnll)
CASES = [(64, 1, 1, "all", False, False), (64, G - 1, 3, "mixed", True, True), (384, G, 1, "some", False, True), (384, G + 1, 3, "some", True, False),
         (1024, 2 * G + 5, 1, "all", False, True), (1024, 2 * G + 5, 3, "some", True, True), (1536, 2 * G + 5, 3, "mixed", False, False),
         (1536, G + 1, 1, "all", True, True), (64, 2 * G + 5, 3, "some", True, False)]
PAIRS = {"f32": (F32, F32), "bf16_f32": (BF, F32), "bf16_bf16": (BF, BF)}


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    assert _ops.LOSS_SEG == G
    return _ops


def case(D, L, B, labels, weights, dnll, pair="f32"):
    bf, res_bf = pair != "f32", pair == "bf16_bf16"
    return HB.reference((D, L, B, labels, weights, dnll, pair),
                        lambda: HB.inputs(1000 * D + 10 * L + B, B, L, D, labels, weights, dnll, bf=bf, res_bf=res_bf))


def dev(c, pair):
    dt, rdt = PAIRS[pair]
    d = lambda t: None if t is None else t.to(DEV)
    return dict(h=c["h"].to(DEV, dt), res=c["res"].to(DEV, rdt), norm_weight=d(c["norm_weight"]), emb=c["emb"].to(DEV, dt), labels=d(c["labels"]),
                loss_weights=d(c["loss_weights"]), dsum=d(c["dsum"]), dnll=d(c["dnll"]))


def run_bwd(ops, c, pair, **kw):
    x = dev(c, pair)
    g = ops.loss_head_bwd(x["h"], x["res"], x["norm_weight"], x["emb"], HB.COMP, x["labels"], x["loss_weights"], c["ignore_index"], c["eps"],
                          B=c["B"], L=c["L"], dsum=x["dsum"], dnll=x["dnll"], **kw)
    torch.cuda.synchronize()
    return g


def kernel_logits(ops, c, pair):
    x = dev(c, pair)
    _, _, lg = ops.loss_head(x["h"], x["res"], x["norm_weight"], x["emb"], HB.COMP, x["labels"], x["loss_weights"], c["ignore_index"], c["eps"],
                             B=c["B"], L=c["L"], want_logits=True)
    return lg.cpu()


def hold(tag, g, ref, bars):
    figs = {k: (SB.metric(getattr(g, KEYS[k]).float().cpu().view(ref[k].shape), ref[k]), bars[k]) for k in HB.NAMES if getattr(g, KEYS[k]) is not None}
    print(tag, " ".join(f"{k} {m:.1e}[{b:.1e}]" for k, (m, b) in figs.items()))
    for k, (m, b) in figs.items():
        assert m <= b, (tag, k, m, b)
    return figs


def unlabelled_rows(c):
    """bool [2B*L]: the rows of positions without a label, on both strands"""
    m = HB.labelled_mask(c["labels"], c["ignore_index"])
    return ~torch.cat([m, m.flip(1)], 0).view(-1)


@pytest.mark.parametrize("D,L,B,labels,weights,dnll", CASES)
def test_fp32_gradients_against_float64(ops, D, L, B, labels, weights, dnll):
    """(1) all four gradients at the fp32 bar.  Observed worst over the cases: 4.1e-7 (dnorm_weight, D = 1536) [3e-5]"""
    c, g64, dev32 = case(D, L, B, labels, weights, dnll)
    g = run_bwd(ops, c, "f32", poison=True)
    assert g.guards_ok
    assert g.dh.dtype == F32 and g.dres.dtype == F32 and g.dnorm_weight.dtype == F32 and g.demb.dtype == F32
    hold(f"head bwd fp32 D={D} L={L} B={B} {labels}", g, g64, {k: SB.bar(k, dev32, False) for k in HB.NAMES})
    # (3) rows of unlabelled positions are exactly 0 although the outputs started as NaN
    un = unlabelled_rows(c).to(DEV)
    assert bool((g.dh[un] == 0).all()) and bool((g.dres[un] == 0).all())
    assert bool(torch.isfinite(g.dh).all()) and bool(torch.isfinite(g.demb).all()) and bool(torch.isfinite(g.dnorm_weight).all())
    assert torch.equal(g.dh, g.dres)


@pytest.mark.parametrize("pair", ["bf16_f32", "bf16_bf16"])
@pytest.mark.parametrize("D,L,B,labels,weights,dnll", CASES)
def test_bf16_gradients_against_the_float64_vjp(ops, D, L, B, labels, weights, dnll, pair):
    """(2) the float64 vector-Jacobian product of the straight-through graph, cotangent from the forward kernel's logits; 2^-7 for all four.
    Observed worst: dh 3.3e-3 (D = 384, L = 65), demb 9.2e-4, dnorm_weight 3.5e-7 [7.8e-3]"""
    c, _, _ = case(D, L, B, labels, weights, dnll, pair)
    ref = HB.grads(c, kernel_logits=kernel_logits(ops, c, pair))
    g = run_bwd(ops, c, pair, poison=True)
    assert g.guards_ok
    assert g.dh.dtype == BF and g.dres.dtype == PAIRS[pair][1] and g.dnorm_weight.dtype == F32 and g.demb.dtype == F32
    hold(f"head bwd {pair} D={D} L={L} B={B} {labels}", g, ref, {k: R.BAR_SCAN[True] for k in HB.NAMES})
    un = unlabelled_rows(c).to(DEV)
    assert bool((g.dh[un] == 0).all()) and bool((g.dres[un] == 0).all())


def test_window_without_labels(ops):
    """(3) a window without labels gives all-zero rows; a batch without any label leaves demb / dnorm_weight zero, not NaN"""
    c, _, _ = case(64, G - 1, 3, "mixed", True, True)
    g = run_bwd(ops, c, "f32", poison=True)
    L = c["L"]
    rows = g.dh.view(6, L, -1)
    assert bool((rows[1] == 0).all()) and bool((rows[3 + 1] == 0).all()) and bool((rows[0] != 0).any())
    none = dict(c, labels=torch.full_like(c["labels"], -100))
    g = run_bwd(ops, none, "f32", poison=True)
    assert g.guards_ok and bool((g.dh == 0).all()) and bool((g.dres == 0).all()) and bool((g.demb == 0).all()) and bool((g.dnorm_weight == 0).all())


@pytest.mark.parametrize("pair", ["f32", "bf16_f32"])
def test_reproducible_and_inside_its_bounds(ops, pair):
    """(4) two calls agree bit for bit, and so does a call whose scratch starts as 0xFF bytes and whose outputs start as NaN between
    sentinel rows, which stay intact"""
    c, _, _ = case(1536, 2 * G + 5, 3, "mixed", False, False, pair)
    a, b, p = run_bwd(ops, c, pair), run_bwd(ops, c, pair), run_bwd(ops, c, pair, poison=True)
    assert p.guards_ok
    for k in KEYS.values():
        assert torch.equal(getattr(a, k), getattr(b, k)) and torch.equal(getattr(a, k), getattr(p, k)), k


def test_partial_output_sets(ops):
    """dh only, and the parameters only: the same bits as the full call; what was not asked for is None"""
    c, _, _ = case(384, G + 1, 3, "some", True, False)
    full = run_bwd(ops, c, "f32")
    only = run_bwd(ops, c, "f32", want=("dh",), poison=True)
    assert only.guards_ok and only.dres is None and only.dnorm_weight is None and only.demb is None and torch.equal(only.dh, full.dh)
    par = run_bwd(ops, c, "f32", want=("dnorm_weight", "demb"), poison=True)
    assert par.guards_ok and par.dh is None and par.dres is None
    assert torch.equal(par.dnorm_weight, full.dnorm_weight) and torch.equal(par.demb, full.demb)
    one = run_bwd(ops, c, "f32", want=("dres", "demb"), poison=True)
    assert one.guards_ok and torch.equal(one.dres, full.dres) and torch.equal(one.demb, full.demb)


def test_independent_of_the_batch(ops):
    """(5) a window's rows of dh do not depend on the batch it runs in: window 2 alone against inside B = 3"""
    c, _, _ = case(1024, 2 * G + 5, 3, "some", True, True)
    B, L, D = 3, c["L"], 1024
    full = run_bwd(ops, c, "f32").dh.view(2 * B, L, D)
    b = 2
    pick = lambda t: t.view(2 * B, L, D)[[b, B + b]].reshape(2 * L, D)
    alone = dict(c, h=pick(c["h"]), res=pick(c["res"]), labels=c["labels"][b:b + 1], loss_weights=c["loss_weights"][b:b + 1],
                 dsum=c["dsum"][b:b + 1], dnll=c["dnll"][b:b + 1], B=1)
    got = run_bwd(ops, alone, "f32").dh.view(2, L, D)
    assert torch.equal(got[0], full[b]) and torch.equal(got[1], full[B + b])


def test_autograd_surface(ops):
    """(6) ops.mlm_loss_head_fn: the plain call without grad; with grad each gradient in its input's shape and dtype at bar (1); the
    other sums carry no graph; a gradient nobody needs is not computed"""
    D, L, B = 384, G + 1, 3
    c, g64, dev32 = case(D, L, B, "some", True, False)
    x = dev(c, "f32")
    args = lambda t: (t["h"].view(2 * B, L, D), t["res"].view(2 * B, L, D), t["norm_weight"], t["emb"], HB.COMP, t["labels"], t["loss_weights"])
    plain = ops.mlm_loss_head_fn(*args(x), c["ignore_index"], c["eps"])
    ref_sums, ref_nll, _ = ops.loss_head(x["h"], x["res"], x["norm_weight"], x["emb"], HB.COMP, x["labels"], x["loss_weights"], c["ignore_index"],
                                         c["eps"], B=B, L=L, want_nll=True)
    assert plain.grad_fn is None and not plain.requires_grad and torch.equal(plain, ref_sums)
    lv = dict(x, **{k: x[k].clone().requires_grad_(True) for k in HB.NAMES})
    with torch.no_grad():
        assert ops.mlm_loss_head_fn(*args(lv), c["ignore_index"], c["eps"]).grad_fn is None
    sums, nll = ops.mlm_loss_head_fn(*args(lv), c["ignore_index"], c["eps"], return_nll=True)
    assert sums.shape == (B, 4) and torch.equal(sums.detach(), ref_sums) and torch.equal(nll.detach(), ref_nll)
    assert sums.requires_grad and nll.requires_grad
    loss_sum, rest, _ = ops._MlmLossHeadFn.apply(lv["h"], lv["res"], lv["norm_weight"], lv["emb"], torch.tensor(HB.COMP, dtype=torch.int32, device=DEV),
                                                 x["labels"], x["loss_weights"], c["ignore_index"], c["eps"], B, L)
    assert loss_sum.requires_grad and not rest.requires_grad and rest.grad_fn is None          # sums[:, 1:] carry no graph
    (sums[:, 0] * x["dsum"]).sum().backward()
    torch.cuda.synchronize()
    from types import SimpleNamespace
    got = SimpleNamespace(**{KEYS[k]: lv[k].grad for k in HB.NAMES})
    for k in HB.NAMES:
        assert lv[k].grad.shape == lv[k].shape and lv[k].grad.dtype == lv[k].dtype, k
    hold("mlm_loss_head_fn fp32", got, g64, {k: SB.bar(k, dev32, False) for k in HB.NAMES})
    # the counts and the weight sum: their gradient is nothing
    for k in HB.NAMES:
        lv[k].grad = None
    sums = ops.mlm_loss_head_fn(*args(lv), c["ignore_index"], c["eps"])
    sums[:, 1:].sum().backward()
    assert all(lv[k].grad is None or bool((lv[k].grad == 0).all()) for k in HB.NAMES)
    # only h requires grad: dres, dnorm_weight and demb are not computed
    only_h = dict(x, h=x["h"].clone().requires_grad_(True))
    ops.loss_head_bwd.last_outputs = ()
    ops.mlm_loss_head_fn(*args(only_h), c["ignore_index"], c["eps"])[:, 0].sum().backward()
    assert ops.loss_head_bwd.last_outputs == ("dh",) and only_h["h"].grad is not None
    # bf16 parameters: the gradients come back in bf16 shapes of their own
    xb = dev(case(D, L, B, "some", True, False, "bf16_f32")[0], "bf16_f32")
    lb = dict(xb, h=xb["h"].clone().requires_grad_(True), res=xb["res"].clone().requires_grad_(True),
              norm_weight=xb["norm_weight"].to(BF).requires_grad_(True), emb=xb["emb"].clone().requires_grad_(True))
    ops.mlm_loss_head_fn(*args(lb), c["ignore_index"], c["eps"])[:, 0].sum().backward()
    assert lb["h"].grad.dtype == BF and lb["res"].grad.dtype == F32 and lb["norm_weight"].grad.dtype == BF and lb["emb"].grad.dtype == BF
    assert lb["emb"].grad.shape == (8, D) and bool(torch.isfinite(lb["emb"].grad.float()).all())
