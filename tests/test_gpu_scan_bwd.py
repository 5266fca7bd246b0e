"""-m gpu: the backward of the selective scan (csrc/scan_bwd.hip through pcad_selective_scan_bwd and ops.selective_scan_fn's autograd
surface) against the float64 CPU reference of tests/scan_bwd_ref.py.

Metric, per gradient tensor and over every element: max |got - ref| / max |ref|.  Bar: max(scan_ref.BAR_SCAN of the dtype the tensor is
stored in - 3e-5 for fp32, 2^-7 for bf16 -, 8 x the same metric of fp32 CPU autograd through the identical restatement); dbc, dA, dD
and dbias of a bf16 call are fp32 tensors and take the fp32 bar.  bf16 cases: every bf16-stored operand is rounded before the
reference sees it.  Every case prints its figures before it asserts.

Shapes, with T = ops.SCAN_BWD_CHUNK (walk steps per stored state = per register-resident chunk): L around one, two and three chunks
(the hand-over of the state from the checkpoint and of the adjoint between chunks, part chunks at the end of the walk, L = 1), E = 192
(three waves' partials of dB | dC) and three strands of nine chunks (the per-strand partials of dA, dD, dbias).

Observed on an MI355X, worst over the cases of each group [bar]: fp32 tensors 4e-8 .. 1.1e-6 [3e-5; the bidirectional sum 3.1e-7
[6e-5]; the projection weights 5.0e-7, 9.1e-7 [3e-5]], bf16-stored tensors 1.0e-3 .. 2.5e-3 [2^-7 = 7.8e-3]; fp32 CPU autograd itself
deviates 4e-8 .. 5e-7 from float64 on these shapes, so the floors govern every bar."""
import pytest
import torch
import torch.nn.functional as F

import scan_bwd_ref as SB
import scan_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF_STORED = ("u", "delta", "z")       # the gradients pcad_selective_scan_bwd stores in the model dtype


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def T_():
    from plantcaduceus_amd import ops as _ops
    return _ops.SCAN_BWD_CHUNK


def to_dev(x, bf):
    """the operands as a call of the model dtype passes them: u, delta, B, C, z, dout in that dtype, A, D, delta_bias fp32"""
    dt = torch.bfloat16 if bf else torch.float32
    return {k: (None if v is None else v.to(DEV).to(dt if k in ("u", "delta", "B", "C", "z", "dout") else torch.float32)) for k, v in x.items()}


def run_raw(ops, x, reverse, bf, poison=False):
    d = to_dev(x, bf)
    g = ops.selective_scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["delta_bias"], d["dout"], reverse=reverse,
                               poison=poison)
    torch.cuda.synchronize()
    return g, dict(u=g.du, delta=g.ddelta, A=g.dA, B=g.dB, C=g.dC, D=g.dD, z=g.dz, delta_bias=g.ddelta_bias)


def hold(tag, got, g64, dev32, stored_bf16=(), factor=1.0):
    """every gradient the reference has, against its bar; -> the figures"""
    figs = {}
    for name in SB.NAMES:
        if g64[name] is None:
            continue
        figs[name] = (SB.metric(got[name], g64[name]), factor * SB.bar(name, dev32, name in stored_bf16))
    print(tag, " ".join(f"{k} {m:.1e}[{b:.1e}]" for k, (m, b) in figs.items()))
    for name, (m, b) in figs.items():
        assert m <= b, (tag, name, m, b)
    return figs


def case(key, Bsz, E, L, reverse, bf=False, bare=False):
    def make():
        x = SB.inputs(1000 * Bsz + 10 * L + E, Bsz, E, L, bf)
        if bare:
            x["z"] = x["D"] = x["delta_bias"] = None
        return x
    return SB.reference((key, Bsz, E, L, bf, bare), make, reverse)


def chunk_lengths():
    T = T_()
    return sorted({1, 7, T - 1, T, T + 1, 2 * T + 1, 3 * T + 4})


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("L", chunk_lengths())
def test_chunk_and_checkpoint_handovers(ops, L, reverse):
    x, g64, dev32 = case("chunks", 2, 128, L, reverse)
    _, got = run_raw(ops, x, reverse, False)
    hold(f"L={L} rev={reverse}", got, g64, dev32)


@pytest.mark.parametrize("reverse", [False, True])
def test_ungated_without_skip_and_bias(ops, reverse):
    """z = None, D = None, delta_bias = None at L = 2T + 1: the ungated kernel, and through autograd the None returns"""
    L = 2 * T_() + 1
    x, g64, dev32 = case("bare", 2, 128, L, reverse, bare=True)
    g, got = run_raw(ops, x, reverse, False)
    assert g.dz is None
    hold(f"bare rev={reverse}", {k: v for k, v in got.items()}, g64, dev32)
    d = to_dev(x, False)
    leaves = {k: d[k].clone().requires_grad_(True) for k in ("u", "delta", "A", "B", "C")}
    out = ops.selective_scan_fn(leaves["u"], leaves["delta"], leaves["A"], leaves["B"], leaves["C"], None, z=None, delta_bias=None,
                                delta_softplus=True, reverse=reverse)
    out.backward(d["dout"])
    hold(f"bare autograd rev={reverse}", {k: leaves[k].grad for k in leaves}, g64, dev32)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", ["three_waves", "three_strands"])
def test_channel_and_strand_partials(ops, shape, bf, reverse):
    T = T_()
    Bsz, E, L = (2, 192, 2 * T + 3) if shape == "three_waves" else (3, 64, 8 * T + 1)
    x, g64, dev32 = case("partials", Bsz, E, L, reverse, bf)
    _, got = run_raw(ops, x, reverse, bf)
    assert got["u"].dtype == (torch.bfloat16 if bf else torch.float32) and got["B"].dtype == torch.float32
    hold(f"{shape} bf={bf} rev={reverse}", got, g64, dev32, BF_STORED if bf else ())


def test_softplus_branches(ops):
    """tests/test_gpu_ops.py test_selective_scan_softplus_threshold_and_small_dt's inputs: 16 channels with delta + bias = 25 (the
    pass-through branch: ddelta = dd, the gradient of the time step) and 16 with -12 (ddelta = sig(-12) dd = 6.1e-6 dd), A x 0.01.
    Besides the bars of the whole tensors, each group of ddelta is held to the fp32 bar against the float64 value on the group's own
    scale, so that the cold group's 1e-5 share of the tensor's maximum does not hide it."""
    def make():
        x = SB.inputs(3, 1, 64, 32)
        x["delta"][:, :16] = 25.0
        x["delta"][:, 16:32] = -12.0
        x["delta_bias"].zero_()
        x["A"] = x["A"] * 0.01
        return x
    x, g64, dev32 = SB.reference("softplus", make, False)
    g32 = SB.grads(x, False, torch.float32)
    _, got = run_raw(ops, x, False, False)
    hold("softplus", got, g64, dev32)
    dd = got["delta"].double().cpu()
    hot, cold = slice(0, 16), slice(16, 32)
    for tag, grp, ref in (("hot", hot, g64["dd"][:, hot]), ("cold", cold, g64["delta"][:, cold])):
        m = SB.metric(dd[:, grp], ref)
        b = max(R.BAR_SCAN[False], R.ORACLE_FACTOR * SB.metric(g32["delta"][:, grp], ref))
        print(f"softplus {tag}: {m:.1e}[{b:.1e}]")
        assert m <= b, (tag, m, b)
    ratio = (dd[:, cold].abs().max() / g64["dd"][:, cold].abs().max()).item()
    print(f"softplus cold ddelta / dd = {ratio:.3e}")
    assert 5e-6 < ratio < 7e-6


@pytest.mark.parametrize("bf", [False, True])
def test_reproducible_complete_in_bounds(ops, bf):
    T = T_()
    x, g64, dev32 = case("partials", 2, 192, 2 * T + 3, True, bf)
    _, a = run_raw(ops, x, True, bf)
    _, b = run_raw(ops, x, True, bf)
    gp, p = run_raw(ops, x, True, bf, poison=True)
    for name in SB.NAMES:
        assert torch.equal(a[name], b[name]), name                       # the same call twice
        assert not torch.isnan(p[name]).any(), name                      # every element written, nothing read that was not written
        assert torch.equal(a[name], p[name]), name                       # ... and the scratch's prior content does not matter
    assert gp.guards_ok                                                  # one row before and after every output untouched


@pytest.mark.parametrize("bf", [False, True])
def test_autograd_surface(ops, bf):
    """ops.selective_scan_fn in the upstream (B, E, L) layout on non-contiguous leaves: .backward() fills .grad in each input's shape
    and dtype.  Here dB and dC come back in B's / C's dtype, so in a bf16 call they are bf16-stored too."""
    T = T_()
    Bsz, E, L = 2, 128, 2 * T + 1
    x, g64, dev32 = case("chunks", Bsz, E, L, False, bf)
    d = to_dev(x, bf)
    leaves = {}
    for k in SB.NAMES:
        t = d[k]
        leaves[k] = (t.transpose(1, 2).contiguous().transpose(1, 2) if t.dim() == 3 else t.clone()).requires_grad_(True)
    assert not leaves["u"].is_contiguous() and not leaves["B"].is_contiguous()
    out = ops.selective_scan_fn(leaves["u"], leaves["delta"], leaves["A"], leaves["B"], leaves["C"], leaves["D"], z=leaves["z"],
                                delta_bias=leaves["delta_bias"], delta_softplus=True)
    assert out.grad_fn is not None
    out.backward(d["dout"].transpose(1, 2).contiguous().transpose(1, 2))
    for k in SB.NAMES:
        assert leaves[k].grad.shape == leaves[k].shape and leaves[k].grad.dtype == leaves[k].dtype, k
    hold(f"autograd bf={bf}", {k: leaves[k].grad for k in SB.NAMES}, g64, dev32, ("u", "delta", "z", "B", "C") if bf else ())
    # nothing requires grad: today's path, no graph, the same bits
    plain = ops.selective_scan_fn(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], z=d["z"], delta_bias=d["delta_bias"], delta_softplus=True)
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain, out.detach())
    with pytest.raises(NotImplementedError):
        ops.selective_scan_fn(leaves["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], z=d["z"], delta_bias=d["delta_bias"],
                              delta_softplus=True, accumulate_into=plain)


def test_bidirectional_sum_composed_by_autograd(ops):
    """(forward call + reverse call, both ungated) x silu(z) in torch: the gradients of the shared operands within twice the bars"""
    T = T_()
    Bsz, E, L = 2, 128, T + 3

    def run():
        x = SB.inputs(77, Bsz, E, L)
        res = []
        for dtype in (torch.float64, torch.float32):
            lv = {k: x[k].detach().clone().to(dtype).requires_grad_(True) for k in SB.NAMES}
            ung = dict(lv, z=None)
            y = SB.forward(ung, False, dtype) + SB.forward(ung, True, dtype)
            ((y * (lv["z"] * torch.sigmoid(lv["z"]))) * x["dout"].to(dtype)).sum().backward()
            res.append({k: lv[k].grad for k in SB.NAMES})
        return x, res[0], {k: SB.metric(res[1][k], res[0][k]) for k in SB.NAMES}
    x, g64, dev32 = R.cached("scan_bwd_bidir", run)
    d = to_dev(x, False)
    lv = {k: d[k].clone().requires_grad_(True) for k in SB.NAMES}
    args = (lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"])
    y = ops.selective_scan_fn(*args, z=None, delta_bias=lv["delta_bias"], delta_softplus=True) + \
        ops.selective_scan_fn(*args, z=None, delta_bias=lv["delta_bias"], delta_softplus=True, reverse=True)
    (y * F.silu(lv["z"])).backward(d["dout"])
    hold("bidirectional", {k: lv[k].grad for k in SB.NAMES}, g64, dev32, factor=2.0)


def test_composed_with_the_projections(ops):
    """x_proj and dt_proj as torch F.linear around the op (mamba_inner_fn's tail, one direction), E = 128, R = 8, L = T + 3: the
    gradients of both projection weights against the all-float64 CPU graph at the fp32 bar"""
    T = T_()
    Bsz, E, Rk, L = 2, 128, 8, T + 3

    def graph(p, scan):
        xc, Wx, Wdt = p["xc"], p["Wx"], p["Wdt"]
        x_dbl = F.linear(xc, Wx)                                               # (B, L, R + 32)
        delta = F.linear(x_dbl[..., :Rk], Wdt).transpose(1, 2)                 # (B, E, L)
        Bm, Cm = x_dbl[..., Rk:Rk + 16].transpose(1, 2), x_dbl[..., Rk + 16:].transpose(1, 2)
        return scan(xc.transpose(1, 2), delta, p["A"], Bm, Cm, p["D"], p["z"], p["delta_bias"])

    def run():
        g = torch.Generator().manual_seed(5)
        base = SB.inputs(6, Bsz, E, L)
        p = dict(xc=torch.randn(Bsz, L, E, generator=g), Wx=torch.randn(Rk + 32, E, generator=g) * E ** -0.5,
                 Wdt=torch.randn(E, Rk, generator=g) * Rk ** -0.5 * 0.5, A=base["A"], D=base["D"], z=base["z"],
                 delta_bias=base["delta_bias"] - 3.0, dout=base["dout"])
        res = []
        for dtype in (torch.float64, torch.float32):
            q = {k: v.detach().clone().to(dtype) for k, v in p.items()}
            q["Wx"].requires_grad_(True)
            q["Wdt"].requires_grad_(True)
            out = graph(q, lambda u, dl, A, Bm, Cm, D, z, b: SB.forward(dict(u=u, delta=dl, A=A, B=Bm, C=Cm, D=D, z=z, delta_bias=b), False, dtype))
            (out * q["dout"]).sum().backward()
            res.append({"Wx": q["Wx"].grad, "Wdt": q["Wdt"].grad})
        return p, res[0], {k: SB.metric(res[1][k], res[0][k]) for k in res[0]}
    p, g64, dev32 = R.cached("scan_bwd_proj", run)
    q = {k: v.to(DEV) for k, v in p.items()}
    q["Wx"].requires_grad_(True)
    q["Wdt"].requires_grad_(True)
    out = graph(q, lambda u, dl, A, Bm, Cm, D, z, b: ops.selective_scan_fn(u, dl, A, Bm, Cm, D, z=z, delta_bias=b, delta_softplus=True))
    out.backward(q["dout"])
    torch.cuda.synchronize()
    for k in ("Wx", "Wdt"):
        m, b = SB.metric(q[k].grad, g64[k]), max(R.BAR_SCAN[False], R.ORACLE_FACTOR * dev32[k])
        print(f"projections d{k}: {m:.1e}[{b:.1e}]")
        assert q[k].grad.shape == p[k].shape
        assert m <= b, (k, m, b)
