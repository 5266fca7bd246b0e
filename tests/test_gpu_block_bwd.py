"""-m gpu: the backward of the conv and of the add + RMSNorm (csrc/conv_bwd.hip, csrc/norm_bwd.hip through include/pcad_bwd.h and the autograd
surface of ops.causal_conv1d_fn / causal_conv1d_dir / rms_norm_fn), the composed differentiable ops.mamba_inner_fn and one whole block,
against the float64 CPU references of tests/block_bwd_ref.py.

Metric, per gradient tensor and over every element: max |got - ref| / max |ref|.  Bar: max(scan_ref.BAR_SCAN of the dtype the tensor is
stored in - 3e-5 for fp32, 2^-7 for bf16 -, 8 x the same metric of fp32 CPU autograd through the identical restatement); dw, db and
dweight of a bf16 call are fp32 tensors and take the fp32 bar.  bf16 cases: every bf16-stored operand is rounded before the reference
sees it.  Every case prints its figures before it asserts.

Shapes, with G = ops.CONV_BWD_SEG (walk steps per lane) and Rw = ops.NORM_BWD_ROWS (rows per wave): L at the strand edges (1, 3, 4), around
one segment (the halo between segments) and with a part segment; E = 72 (a part wave of channels, fp32 E % 4 and bf16 E % 8) with three
strands' partials; rows around one and two slabs and D = 8, 384, 2048 (one lane, a part wave, four chunks per lane).

Observed on an MI355X, worst over the cases of each group [bar]: conv fp32 tensors 3.1e-7, norm fp32 tensors 2.1e-7 [3e-5]; bf16-stored
tensors 3.8e-3 (conv dx), 3.7e-3 (norm dx) [2^-7 = 7.8e-3]; mamba_inner_fn fp32 gradients 1.3e-6 [3e-5], one block 6.8e-7 [6e-5]; fp32 CPU
autograd itself deviates 2e-8 .. 1.1e-6 from float64 on these shapes, so the floors govern every bar.  Each test's docstring has its own."""
import pytest
import torch

import block_bwd_ref as BB
import scan_bwd_ref as SB
import scan_ref as R
from oracle import caduceus_oracle as O

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def G_():
    from plantcaduceus_amd import ops as _ops
    return _ops.CONV_BWD_SEG


def Rw_():
    from plantcaduceus_amd import ops as _ops
    return _ops.NORM_BWD_ROWS


def hold(tag, got, g64, dev32, stored_bf16=(), factor=1.0, check=True):
    """every gradient the reference has and `got` names, against its bar; -> the figures"""
    figs = {}
    for name, ref in g64.items():
        if ref is None or name not in got:
            continue
        figs[name] = (SB.metric(got[name], ref), factor * SB.bar(name, dev32, name in stored_bf16))
    print(tag, " ".join(f"{k} {m:.1e}[{b:.1e}]" for k, (m, b) in figs.items()))
    if check:
        for name, (m, b) in figs.items():
            assert m <= b, (tag, name, m, b)
    return figs


# ---- conv -----------------------------------------------------------------------------------------------------------------------------
def conv_case(S, L, E, reverse, bf=False):
    return BB.reference(("conv", S, L, E, reverse, bf), lambda: BB.conv_inputs(100 * S + 10 * L + E, S, L, E, bf),
                        lambda c, dtype: BB.conv_grads(c, reverse, dtype))


def run_conv(ops, c, reverse, bf, poison=False, x_dev=None):
    dt = BF if bf else F32
    x = c["x"].to(DEV).to(dt) if x_dev is None else x_dev
    g = ops.causal_conv1d_silu_bwd(x, c["w"].to(DEV), c["b"].to(DEV), c["dout"].to(DEV).to(dt), reverse=reverse, poison=poison)
    torch.cuda.synchronize()
    return g, dict(x=g.dx, w=g.dw, b=g.db)


def conv_lengths():
    G = G_()
    return sorted({1, 3, 4, G - 1, G, G + 1, G + 3, 2 * G + 5})


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("L", conv_lengths())
def test_conv_strand_edges_and_segment_halos(ops, L, reverse):
    """S = 2, E = 128, fp32, every L of conv_lengths() in both directions.  Observed worst: 3.1e-7 (dw) [3e-5]"""
    c, g64, dev32 = conv_case(2, L, 128, reverse)
    _, got = run_conv(ops, c, reverse, False)
    hold(f"conv L={L} rev={reverse}", got, g64, dev32)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bf", [False, True])
def test_conv_part_wave_and_strand_partials(ops, bf, reverse):
    """S = 3, E = 72, L = G + 3: a part wave of channels, nine rows of partials.  Observed worst: fp32 tensors 2.8e-7 (db) [3e-5], bf16
    dx 3.8e-3 [7.8e-3]"""
    c, g64, dev32 = conv_case(3, G_() + 3, 72, reverse, bf)
    _, got = run_conv(ops, c, reverse, bf)
    assert got["x"].dtype == (BF if bf else F32) and got["w"].dtype == F32 and got["b"].dtype == F32
    hold(f"conv E=72 bf={bf} rev={reverse}", got, g64, dev32, ("x",) if bf else ())


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bf", [False, True])
def test_conv_reads_x_in_place_from_the_first_half_of_xz(ops, bf, reverse):
    """x = the first half of a [S, L, 2E] buffer whose second half is NaN: rows ldx = 2E apart, nothing read beyond a row's E;
    the same bits as from packed rows.  Observed worst: fp32 tensors 3.1e-7 (dw) [3e-5], bf16 dx 3.1e-3 [7.8e-3]"""
    S, L, E = 2, G_() + 3, 128
    c, g64, dev32 = conv_case(S, L, E, reverse, bf)
    xz = torch.full((S, L, 2 * E), float("nan"), dtype=BF if bf else F32, device=DEV)
    xz[..., :E] = c["x"].to(DEV)
    x = xz[..., :E]
    assert not x.is_contiguous() and x.stride(1) == 2 * E
    _, got = run_conv(ops, c, reverse, bf, x_dev=x)
    for k, v in got.items():
        assert not torch.isnan(v).any(), k
    hold(f"conv ldx=2E bf={bf} rev={reverse}", got, g64, dev32, ("x",) if bf else ())
    _, packed = run_conv(ops, c, reverse, bf)
    for k in got:
        assert torch.equal(got[k], packed[k]), k


@pytest.mark.parametrize("bf", [False, True])
def test_conv_reproducible_complete_in_bounds(ops, bf):
    c, _, _ = conv_case(3, G_() + 3, 72, True, bf)
    _, a = run_conv(ops, c, True, bf)
    _, b = run_conv(ops, c, True, bf)
    gp, p = run_conv(ops, c, True, bf, poison=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name                       # the same call twice
        assert not torch.isnan(p[name]).any(), name                      # every element written, nothing read that was not written
        assert torch.equal(a[name], p[name]), name                       # ... and the scratch's prior content does not matter
    assert gp.guards_ok                                                  # one row before and after every output untouched


@pytest.mark.parametrize("bf", [False, True])
def test_conv_autograd_surface(ops, bf):
    """ops.causal_conv1d_fn in upstream's (B, E, L) layout on a non-contiguous leaf, weight (E, 4) in the model dtype: .backward() fills
    .grad in each input's shape and dtype (so dw, db of a bf16 call are bf16-stored here); ops.causal_conv1d_dir both ways.
    Observed worst: fp32 tensors 3.1e-7 (dw) [3e-5]; bf16-stored 3.1e-3 (dx), 2.8e-3 (dw) [7.8e-3]"""
    dt = BF if bf else F32
    S, L, E = 2, G_() + 3, 128
    c, g64, dev32 = conv_case(S, L, E, False, bf)
    if bf:                                    # the parameters are bf16 tensors here: the reference must see the rounded taps
        c, g64, dev32 = BB.reference(("conv_bf_params", S, L, E), lambda: {k: R.bf16(v) for k, v in BB.conv_inputs(7, S, L, E, True).items()},
                                     lambda cc, dtype: BB.conv_grads(cc, False, dtype))
    x = c["x"].to(DEV).to(dt).transpose(1, 2).requires_grad_(True)       # (B, E, L) view of token-major rows
    w, b = c["w"].to(DEV).to(dt).requires_grad_(True), c["b"].to(DEV).to(dt).requires_grad_(True)
    assert not x.is_contiguous()
    out = ops.causal_conv1d_fn(x, w, b, activation="silu")
    assert out.grad_fn is not None and out.shape == x.shape and out.dtype == dt
    out.backward(c["dout"].to(DEV).to(dt).transpose(1, 2))
    for t in (x, w, b):
        assert t.grad.shape == t.shape and t.grad.dtype == t.dtype
    hold(f"conv autograd bf={bf}", dict(x=x.grad.transpose(1, 2), w=w.grad, b=b.grad), g64, dev32, ("x", "w", "b") if bf else ())
    # nothing requires grad: today's path (the both-direction kernel), no graph, the same bits
    plain = ops.causal_conv1d_fn(x.detach(), w.detach(), b.detach(), activation="silu")
    assert plain.grad_fn is None and not plain.requires_grad
    assert torch.equal(plain, out.detach())
    with torch.no_grad():
        assert ops.causal_conv1d_fn(x, w, b, activation="silu").grad_fn is None
    # the one-direction form, token-major, either direction
    for reverse in (False, True):
        cr, gr64, devr = conv_case(S, L, E, reverse, bf)
        xt = cr["x"].to(DEV).to(dt).requires_grad_(True)
        wt, bt = cr["w"].to(DEV).requires_grad_(True), cr["b"].to(DEV).requires_grad_(True)
        y = ops.causal_conv1d_dir(xt, wt, bt, reverse=reverse)
        assert y.grad_fn is not None
        y.backward(cr["dout"].to(DEV).to(dt))
        hold(f"conv_dir autograd bf={bf} rev={reverse}", dict(x=xt.grad, w=wt.grad, b=bt.grad), gr64, devr, ("x",) if bf else ())
        assert wt.grad.dtype == F32 and wt.grad.shape == wt.shape
        plain = ops.causal_conv1d_dir(xt.detach(), wt.detach(), bt.detach(), reverse=reverse)
        assert plain.grad_fn is None and torch.equal(plain, y.detach())
        if (E * xt.element_size()) % 128 == 0:
            with pytest.raises(NotImplementedError):
                ops.causal_conv1d_dir(xt, wt, bt, reverse=reverse, blocked=True)


# ---- add + RMSNorm --------------------------------------------------------------------------------------------------------------------
MODES = {"fp32": (False, False), "bf16_res_fp32": (True, False), "bf16_res_bf16": (True, True)}       # -> (bf, residual stored in bf16)


def norm_case(rows, D, residual, prenorm, bf, res_bf):
    return BB.reference(("norm", rows, D, residual, prenorm, bf, res_bf),
                        lambda: BB.norm_inputs(rows + D, rows, D, residual, prenorm, bf, res_bf), BB.norm_grads)


def run_norm(ops, c, bf, res_bf, poison=False):
    dt, rdt = (BF if bf else F32), (BF if res_bf else F32)
    dev = lambda t, ty: None if t is None else t.to(DEV).to(ty)
    g = ops.add_rmsnorm_bwd(dev(c["x"], dt), dev(c["residual"], rdt), c["weight"].to(DEV), dev(c["dy"], dt), dev(c["dres_out"], rdt), c["eps"],
                            residual_in_fp32=not res_bf, poison=poison)
    torch.cuda.synchronize()
    got = dict(x=g.dx, weight=g.dweight)
    if g.dresidual_in is not None:
        got["residual"] = g.dresidual_in
    return g, got


def norm_rows():
    Rw = Rw_()
    return sorted({1, 5, Rw, Rw + 1, 2 * Rw + 3})


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("D", [8, 384, 2048])
@pytest.mark.parametrize("rows", norm_rows())
def test_norm_slabs_widths_and_forms(ops, rows, D, mode):
    """the four forms residual x prenorm of every (rows, D, dtypes).  Observed worst: fp32 tensors 2.1e-7 (dweight) [3e-5], bf16-stored
    3.7e-3 (dx) [7.8e-3]"""
    bf, res_bf = MODES[mode]
    for residual in (False, True):
        for prenorm in (False, True):
            c, g64, dev32 = norm_case(rows, D, residual, prenorm, bf, res_bf)
            g, got = run_norm(ops, c, bf, res_bf)
            assert (g.dresidual_in is not None) == residual
            assert got["x"].dtype == (BF if bf else F32) and got["weight"].dtype == F32
            if residual:
                assert got["residual"].dtype == (BF if res_bf else F32)
            stored = (("x",) if bf else ()) + (("residual",) if res_bf else ())
            hold(f"norm rows={rows} D={D} {mode} res={residual} prenorm={prenorm}", got, g64, dev32, stored)


@pytest.mark.parametrize("mode", list(MODES))
def test_norm_reproducible_complete_in_bounds(ops, mode):
    bf, res_bf = MODES[mode]
    c, _, _ = norm_case(2 * Rw_() + 3, 384, True, True, bf, res_bf)
    _, a = run_norm(ops, c, bf, res_bf)
    _, b = run_norm(ops, c, bf, res_bf)
    gp, p = run_norm(ops, c, bf, res_bf, poison=True)
    for name in a:
        assert torch.equal(a[name], b[name]), name
        assert not torch.isnan(p[name]).any(), name
        assert torch.equal(a[name], p[name]), name
    assert gp.guards_ok


@pytest.mark.parametrize("mode", list(MODES))
def test_norm_autograd_surface(ops, mode):
    """ops.rms_norm_fn on non-contiguous (B, L, D) leaves (a transposed buffer), weight in the model dtype, prenorm with both outputs
    used and without: .grad in each input's shape and dtype.  Observed worst: fp32 tensors 1.5e-7 (dx) [3e-5], bf16-stored 3.1e-3 (dx)
    [7.8e-3]"""
    bf, res_bf = MODES[mode]
    dt = BF if bf else F32
    Bsz, L, D = 3, Rw_() - 3, 384
    for prenorm in (True, False):
        key = ("norm_autograd", mode, prenorm)
        c, g64, dev32 = BB.reference(key, lambda: {k: (R.bf16(v) if bf and k == "weight" else v)
                                                   for k, v in BB.norm_inputs(11, Bsz * L, D, True, prenorm, bf, res_bf).items()}, BB.norm_grads)
        lay = lambda t, ty: t.view(Bsz, L, D).transpose(0, 1).contiguous().transpose(0, 1).to(DEV).to(ty)      # (B, L, D), strides of (L, B, D)
        x = lay(c["x"], dt).requires_grad_(True)
        # the residual stream arrives in its own dtype: fp32 with residual_in_fp32, else the model's
        res = lay(c["residual"], BF if res_bf else F32).requires_grad_(True)
        w = c["weight"].to(DEV).to(dt).requires_grad_(True)
        assert not x.is_contiguous()
        out = ops.rms_norm_fn(x, w, None, res, c["eps"], prenorm=prenorm, residual_in_fp32=not res_bf)
        y, r = out if prenorm else (out, None)
        assert y.grad_fn is not None and y.dtype == dt and y.shape == x.shape
        loss = (y.float() * lay(c["dy"], F32)).sum()
        if prenorm:
            assert r.dtype == (BF if res_bf else F32)
            loss = loss + (r.float() * lay(c["dres_out"], F32)).sum()
        loss.backward()
        for t in (x, res, w):
            assert t.grad.shape == t.shape and t.grad.dtype == t.dtype
        stored = (("x", "weight") if bf else ()) + (("residual",) if res_bf else ())
        hold(f"norm autograd {mode} prenorm={prenorm}", dict(x=x.grad.reshape(-1, D), residual=res.grad.reshape(-1, D), weight=w.grad),
             g64, dev32, stored)
        plain = ops.rms_norm_fn(x.detach(), w.detach(), None, res.detach(), c["eps"], prenorm=prenorm, residual_in_fp32=not res_bf)
        py, pr = plain if prenorm else (plain, None)
        assert py.grad_fn is None and not py.requires_grad and torch.equal(py, y.detach())
        if prenorm:
            assert pr.grad_fn is None and torch.equal(pr, r.detach())
    # without a residual: None comes back for it, the prenorm output is x's own gradient path
    c, g64, dev32 = norm_case(5, 384, False, True, bf, res_bf)
    x = c["x"].to(DEV).to(dt).requires_grad_(True)
    y, r = ops.rms_norm_fn(x, c["weight"].to(DEV), None, None, c["eps"], prenorm=True, residual_in_fp32=not res_bf)
    ((y.float() * c["dy"].to(DEV)).sum() + (r.float() * c["dres_out"].to(DEV)).sum()).backward()
    hold(f"norm autograd {mode} no residual", dict(x=x.grad), g64, dev32, ("x",) if bf else ())


# ---- mamba_inner_fn and one block -----------------------------------------------------------------------------------------------------
DM, E_, RK, BSZ = 64, 128, 8, 2
MAMBA_GRADS = ("xz",) + BB.MAMBA_PARAMS
BF_STORED_PARAMS = ("xz", "x_proj", "dt_proj", "out_proj")        # what a bf16 model holds in bf16; conv taps, A, D and biases stay fp32


def mamba_inputs(bf):
    L = G_() + 5
    g = torch.Generator().manual_seed(L)
    c = BB.mamba_params(DM + RK, DM, E_, RK)
    c["xz"] = torch.randn(BSZ, 2 * E_, L, generator=g)
    c["dout"] = torch.randn(BSZ, L, DM, generator=g)
    if bf:
        for k in BF_STORED_PARAMS + ("dout",):
            c[k] = R.bf16(c[k])
    return c


def mamba_reference(reverse, bf):
    return BB.graph_reference(("mamba_inner", reverse, bf), lambda: mamba_inputs(bf),
                              lambda K, lv: (K.mamba_inner(lv["xz"], lv, reverse) * lv["dout"].detach()).sum())


def mamba_gpu(ops, c, reverse, dt):
    lv = {k: c[k].to(DEV).to(dt if k in BF_STORED_PARAMS else F32).requires_grad_(True) for k in MAMBA_GRADS}
    out = BB.GpuOps(ops).mamba_inner(lv["xz"], lv, reverse)
    return lv, out


@pytest.mark.parametrize("dtype", [F32, BF])
def test_mamba_inner_grad_path_forward_is_the_operator(ops, dtype):
    """the composed path's value against the oracle's mamba_inner, and the reverse twin against the flipped call, at
    test_mamba_inner_fn's bars: 3e-5 (fp32), 2^-7 (bf16, the oracle rounding where upstream stores bf16).  Observed: fp32 2.8e-7 / 2.4e-7
    (reverse), 8e-8 / 9e-8 from the fused inference path; bf16 0 / 1.5e-3, the fused path's bits"""
    bf = dtype == BF
    c = mamba_inputs(bf)
    p = O.MambaParams(in_proj=c["in_proj"], conv_w=c["conv_w"], conv_b=c["conv_b"], x_proj=c["x_proj"], dt_proj_w=c["dt_proj"],
                      dt_proj_b=c["delta_bias"], A_log=c["A_log"], D=c["D"], out_proj=c["out_proj"])
    rnd = O.round_bf16 if bf else (lambda t: t)
    tol = 2.0 ** -7 if bf else 3e-5
    for reverse in (False, True):
        lv, out = mamba_gpu(ops, c, reverse, dtype)
        assert out.grad_fn is not None and out.dtype == dtype and out.shape == c["dout"].shape
        ref = O.mamba_inner(c["xz"].flip(-1), p, rnd).flip(1) if reverse else O.mamba_inner(c["xz"], p, rnd)
        e = SB.metric(out, ref)
        with torch.no_grad():
            fused = BB.GpuOps(ops).mamba_inner(lv["xz"], lv, reverse)
        assert fused.grad_fn is None
        print(f"mamba_inner grad path {dtype} rev={reverse}: {e:.2e}[{tol:.1e}]; against the fused inference path {SB.metric(out, fused):.2e}")
        assert e < tol


@pytest.mark.parametrize("reverse", [False, True])
def test_mamba_inner_gradients_fp32(ops, reverse):
    """xz and every parameter against the all-float64 CPU graph of the restatements, at the fp32 bar.  Observed worst: 1.3e-6
    (delta_bias) [3e-5]; the others 1.5e-7 .. 8.1e-7"""
    c, g64, dev32 = mamba_reference(reverse, False)
    lv, out = mamba_gpu(ops, c, reverse, F32)
    out.backward(c["dout"].to(DEV))
    torch.cuda.synchronize()
    for k in MAMBA_GRADS:
        assert lv[k].grad.shape == c[k].shape and lv[k].grad.dtype == F32, k
    hold(f"mamba_inner fp32 rev={reverse}", {k: lv[k].grad for k in MAMBA_GRADS}, g64, dev32)


@pytest.mark.parametrize("reverse", [False, True])
def test_mamba_inner_gradients_bf16_finite(ops, reverse):
    """bf16: finite gradients of the right shapes and dtypes; the figures against the float64 graph of the rounded operands are printed,
    not asserted - xc, x_dbl, delta and y are each rounded to bf16 on the way and nothing here derives a bar for their compound
    (observed: bf16-stored gradients 4.1e-3 .. 4.9e-3, the fp32 parameters' 1.8e-3 .. 1.0e-2 (delta_bias); per tensor in DESIGN.md §4m)"""
    c, g64, dev32 = mamba_reference(reverse, True)
    lv, out = mamba_gpu(ops, c, reverse, BF)
    out.backward(c["dout"].to(DEV).to(BF))
    torch.cuda.synchronize()
    for k in MAMBA_GRADS:
        gr = lv[k].grad
        assert gr.shape == c[k].shape and gr.dtype == (BF if k in BF_STORED_PARAMS else F32), k
        assert torch.isfinite(gr).all(), k
    hold(f"mamba_inner bf16 rev={reverse} (not asserted)", {k: lv[k].grad for k in MAMBA_GRADS}, g64, dev32, BF_STORED_PARAMS, check=False)


def test_one_block_composed_by_autograd(ops):
    """rms_norm_fn(prenorm, fp32 residual) -> in_proj -> mamba_inner_fn + its reverse twin on shared weights, the residual stream handed
    on: every parameter's and both inputs' gradients against the float64 CPU graph at twice the fp32 bar (two directions are summed).  Observed worst: 6.8e-7 (dt_proj) [6e-5]"""
    L = G_() + 5
    names = ("hidden", "residual", "norm_w", "in_proj") + BB.MAMBA_PARAMS

    def make():
        g = torch.Generator().manual_seed(21)
        c = BB.mamba_params(31, DM, E_, RK)
        c.update(hidden=torch.randn(BSZ, L, DM, generator=g), residual=torch.randn(BSZ, L, DM, generator=g) * 2.0,
                 dout=torch.randn(BSZ, L, DM, generator=g), dres=torch.randn(BSZ, L, DM, generator=g))
        return c

    def run(K, lv):
        out, res = BB.block(K, lv, lv["hidden"], lv["residual"])
        return (out * lv["dout"].detach()).sum() + (res * lv["dres"].detach()).sum()
    c, g64, dev32 = BB.graph_reference("block", make, run)
    lv = {k: c[k].to(DEV).requires_grad_(True) for k in names}
    lv.update(dout=c["dout"].to(DEV), dres=c["dres"].to(DEV))
    out, res = BB.block(BB.GpuOps(ops), lv, lv["hidden"], lv["residual"])
    assert out.grad_fn is not None and res.grad_fn is not None and res.dtype == F32
    ((out * lv["dout"]).sum() + (res * lv["dres"]).sum()).backward()
    torch.cuda.synchronize()
    for k in names:
        assert lv[k].grad.shape == c[k].shape and lv[k].grad.dtype == F32, k
    hold("block", {k: lv[k].grad for k in names}, g64, dev32, factor=2.0)
