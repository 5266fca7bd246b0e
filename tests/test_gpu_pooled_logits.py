"""-m gpu: the score head on cached pooled vectors (csrc/pool_feat.hip through include/pcad_bwd.h pcad_pooled_logits /
pcad_pooled_logits_bwd, ops.pooled_logits / pooled_logits_bwd and the autograd surface ops.pooled_logits_fn).

The point of the kernels is bit equality with the head that produced the pooled vectors, so the checks are `torch.equal`:
  forward    `pooled` is ops.pooled_head(..., want_pooled=True)'s on random h, res of L = 65 (two segments of 64 rows) for mean / first /
             last / max; pooled_logits of it equals that same call's logits
  dscore_w   equals ops.pooled_head_bwd(..., want=("dscore_w",))'s for mean / first / last (max has a forward only)
  dpooled    has no twin in the pooled head (its cotangent row carries the mean's 1 / L): held to the float64 restatement of
             tests/pooled_logits_ref.py under tests/scan_bwd_ref.py's metric, max |got - ref| / max |ref|, and its fp32 bar
             max(3e-5, 8 x the same metric of the fp32 CPU restatement)
Shapes: every (D, NL) of D = 64 (below one lane stride), 384, 1024, 1536, 2048 (the 512 / 1024 / 2048 width forms of the head that
makes `pooled`) x NL = 1, 2 (fewer labels than waves), 5 (an uneven wave split), 92, 256 (the limit); B = 1 and 3 alternate over them
and the poolings cycle, so that every D and every NL meets both batches and every pooling; model dtype fp32 and bf16 (h bf16, res fp32).
Every case prints its figures before it asserts.

Observed on an MI355X: see DESIGN.md §4x."""
import pytest
import torch

import pooled_logits_ref as PL
import scan_bwd_ref as SB
import scan_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
L, EPS = 65, 1e-5
DS, NLS = (64, 384, 1024, 1536, 2048), (1, 2, 5, 92, 256)
ALL_POOLINGS = ("mean", "first", "last", "max")
# (D, NL, B, pooling of the forward check, pooling of the backward checks)
CASES = [(D, NL, (1, 3)[(i + j) % 2], ALL_POOLINGS[(i + j) % 4], ALL_POOLINGS[(i + 2 * j) % 3]) for i, D in enumerate(DS) for j, NL in enumerate(NLS)]
DTYPES = {"f32": F32, "bf16": BF}


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def head_case(ops, D, NL, B, pooling, dt):
    """random rows through the pooled head, once per case: -> dict(h, res, norm_weight, score_w, dlogits, logits, pooled) on the device"""
    def run():
        g = torch.Generator().manual_seed(1000 * D + 10 * NL + B + ALL_POOLINGS.index(pooling))
        dtype = DTYPES[dt]
        c = dict(h=torch.randn(2 * B * L, D, generator=g).to(DEV, dtype), res=(torch.randn(2 * B * L, D, generator=g) * 0.5 + 0.25).to(DEV),
                 norm_weight=(torch.rand(D, generator=g) + 0.5).to(DEV), score_w=(torch.randn(NL, D, generator=g) * (3.0 / D ** 0.5)).to(DEV, dtype),
                 dlogits=torch.randn(B, NL, generator=g).to(DEV))
        c["logits"], c["pooled"] = ops.pooled_head(c["h"], c["res"], c["norm_weight"], c["score_w"], pooling, EPS, B=B, L=L, want_pooled=True)
        torch.cuda.synchronize()
        return c
    return R.cached(("pooled_logits", D, NL, B, pooling, dt), run)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("D,NL,B,pooling,_bwd", CASES)
def test_logits_of_cached_vectors_are_the_heads_bits(ops, D, NL, B, pooling, _bwd, dt):
    c = head_case(ops, D, NL, B, pooling, dt)
    got = ops.pooled_logits(c["pooled"], c["score_w"], DTYPES[dt])
    again = ops.pooled_logits(c["pooled"], c["score_w"], DTYPES[dt])
    torch.cuda.synchronize()
    worst = (got - c["logits"]).abs().max().item()
    print(f"pooled_logits D={D} NL={NL} B={B} {pooling} {dt}: max |d logit| {worst:.3e}, max |logit| {c['logits'].abs().max().item():.3f}")
    assert got.shape == (B, NL) and got.dtype == F32 and bool(torch.isfinite(got).all())
    assert torch.equal(got, c["logits"]) and torch.equal(got, again)
    # without grad the autograd surface is the raw call
    assert torch.equal(ops.pooled_logits_fn(c["pooled"], c["score_w"], DTYPES[dt]), got)


@pytest.mark.parametrize("dt", list(DTYPES))
@pytest.mark.parametrize("D,NL,B,_fwd,pooling", CASES)
def test_backward(ops, D, NL, B, _fwd, pooling, dt):
    """dscore_w bit-equal to the pooled head's; dpooled against float64; each output NULL in turn leaves the other's bits; two calls
    agree; sentinels intact around NaN-filled outputs; a zero cotangent gives exact zeros"""
    c = head_case(ops, D, NL, B, pooling, dt)
    W = c["score_w"].to(DTYPES[dt]).float()
    twin = ops.pooled_head_bwd(c["h"], c["res"], c["norm_weight"], c["score_w"], c["pooled"], c["dlogits"], pooling, EPS, B=B, L=L, want=("dscore_w",))
    both = ops.pooled_logits_bwd(c["pooled"], W, c["dlogits"], want=("dscore_w", "dpooled"), poison=True)
    again = ops.pooled_logits_bwd(c["pooled"], W, c["dlogits"], want=("dscore_w", "dpooled"))
    only_w = ops.pooled_logits_bwd(c["pooled"], W, c["dlogits"])
    only_p = ops.pooled_logits_bwd(c["pooled"], W, c["dlogits"], want=("dpooled",), poison=True)
    zero = ops.pooled_logits_bwd(c["pooled"], W, torch.zeros_like(c["dlogits"]), want=("dscore_w", "dpooled"))
    torch.cuda.synchronize()
    ref_w, ref_p = PL.backward(c["pooled"].cpu(), W.cpu(), c["dlogits"].cpu())
    w32, p32 = PL.backward(c["pooled"].cpu(), W.cpu(), c["dlogits"].cpu(), dtype=F32)
    dev32 = {"dscore_w": SB.metric(w32, ref_w), "dpooled": SB.metric(p32, ref_p)}
    mw, mp = SB.metric(both.dscore_w, ref_w), SB.metric(both.dpooled, ref_p)
    bw, bp = SB.bar("dscore_w", dev32, False), SB.bar("dpooled", dev32, False)
    print(f"pooled_logits_bwd D={D} NL={NL} B={B} {pooling} {dt}: dscore_w {mw:.1e}[{bw:.1e}] equal to the head's "
          f"{torch.equal(both.dscore_w, twin.dscore_w)}, dpooled {mp:.1e}[{bp:.1e}]")
    assert both.guards_ok and only_p.guards_ok
    assert both.dscore_w.shape == (NL, D) and both.dpooled.shape == (B, 2, D) and both.dscore_w.dtype == both.dpooled.dtype == F32
    assert torch.equal(both.dscore_w, twin.dscore_w)
    assert mw <= bw and mp <= bp
    assert torch.equal(both.dpooled[:, 0], both.dpooled[:, 1])
    assert only_w.dpooled is None and only_p.dscore_w is None and ops.pooled_logits_bwd.last_outputs == ("dscore_w", "dpooled")
    assert torch.equal(only_w.dscore_w, both.dscore_w) and torch.equal(only_p.dpooled, both.dpooled)
    assert torch.equal(again.dscore_w, both.dscore_w) and torch.equal(again.dpooled, both.dpooled)
    assert not bool(zero.dscore_w.any()) and not bool(zero.dpooled.any())


def test_no_windows_is_ok(ops):
    D, NL = 384, 5
    pooled, W = torch.zeros((0, 2, D), device=DEV), torch.randn(NL, D, device=DEV)
    lg = ops.pooled_logits(pooled, W, BF)
    g = ops.pooled_logits_bwd(pooled, W, torch.zeros((0, NL), device=DEV), want=("dscore_w", "dpooled"), poison=True)
    torch.cuda.synchronize()
    assert lg.shape == (0, NL) and g.dpooled.shape == (0, 2, D) and g.guards_ok
    assert bool(torch.isnan(g.dscore_w).all())              # nothing is done: the poisoned output is left as it was


def test_wrappers_refuse_what_the_entries_cannot_see(ops):
    pooled, W = torch.zeros((2, 2, 64), device=DEV), torch.zeros((3, 64), device=DEV)
    with pytest.raises(ValueError, match="pooled"):
        ops.pooled_logits(pooled.view(2, 128), W, F32)
    with pytest.raises(ValueError, match="pooled"):
        ops.pooled_logits(pooled.to(BF), W, BF)
    with pytest.raises(ValueError, match="score_w"):
        ops.pooled_logits(pooled, W[:, :32], F32)
    with pytest.raises(ValueError, match="dtype"):
        ops.pooled_logits(pooled, W, torch.float16)
    with pytest.raises(ValueError, match="dlogits"):
        ops.pooled_logits_bwd(pooled, W, torch.zeros((2, 4), device=DEV))
    with pytest.raises(ValueError, match="want"):
        ops.pooled_logits_bwd(pooled, W, torch.zeros((2, 3), device=DEV), want=())


@pytest.mark.parametrize("dt", list(DTYPES))
def test_autograd_hands_score_the_kernels_fp32_gradient(ops, dt):
    """an fp32 `score` under a bf16 model receives the fp32 dscore_w bit for bit, straight through its rounding to the model dtype; a
    pooled that requires grad receives dpooled; what nobody needs is not computed"""
    D, NL, B = 1024, 5, 3
    c = head_case(ops, D, NL, B, "mean", dt)
    g = torch.Generator().manual_seed(3)
    score = torch.nn.Parameter((torch.randn(NL, D, generator=g) * (3.0 / D ** 0.5)).to(DEV))       # fp32, not bf16-valued
    rounded = score.detach().to(DTYPES[dt]).float()
    lg = ops.pooled_logits_fn(c["pooled"], score, DTYPES[dt])
    assert lg.requires_grad and torch.equal(lg.detach(), ops.pooled_logits(c["pooled"], rounded, DTYPES[dt]))
    (lg * c["dlogits"]).sum().backward()
    assert ops.pooled_logits_bwd.last_outputs == ("dscore_w",)
    want = ops.pooled_logits_bwd(c["pooled"], rounded, c["dlogits"], want=("dscore_w", "dpooled"))
    assert score.grad.dtype == F32 and torch.equal(score.grad, want.dscore_w)
    if dt == "bf16":
        assert not torch.equal(rounded, score.detach()) and not torch.equal(score.grad, score.grad.to(BF).float())
    pooled = c["pooled"].clone().requires_grad_(True)
    (ops.pooled_logits_fn(pooled, score.detach(), DTYPES[dt]) * c["dlogits"]).sum().backward()
    assert ops.pooled_logits_bwd.last_outputs == ("dpooled",) and torch.equal(pooled.grad, want.dpooled)
    with torch.no_grad():
        assert not ops.pooled_logits_fn(pooled, score, DTYPES[dt]).requires_grad
