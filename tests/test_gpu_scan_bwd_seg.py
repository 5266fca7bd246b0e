"""-m gpu: the segmented backward of the selective scan (csrc/scan_bwd_seg.hip through pcad_selective_scan_bwd_seg and the `segments`
keyword of ops.selective_scan_bwd / selective_scan_fn) against the float64 CPU reference of tests/scan_bwd_ref.py.

Metric, bars, operands and the printing of every figure before its assertion are tests/test_gpu_scan_bwd.py's, imported from there
unchanged: max |got - ref| / max |ref| per gradient tensor against max(3e-5 fp32 / 2^-7 bf16-stored, 8 x fp32 CPU autograd's own
deviation).  References are shared with that file where the shapes coincide (scan_bwd_ref.reference caches per key).

Shapes, with T = ops.SCAN_BWD_CHUNK: the issue's - two segments the second of one step (L = T + 1), segments of one chunk with a part
chunk at the end (3T + 4 at G = 4: 8, 8, 8, 4), of two and three chunks (3T + 4 at G = 3; 8T + 1 at G = 2, 3, 8: 40 + 25, 24 + 24 + 17,
five of 16 with a last one of one step), so that with three and more effective segments a missing P_g in the combine would show; E = 192
(three waves' partials) and three strands (S G rows of dA / dD / dbias partials); one effective segment bit-equal to
pcad_selective_scan_bwd; and one strand length past 2 SCAN_BWD_SEG_MIN_STEPS, where "auto" picks more than one segment.

Observed on an MI355X, worst over the cases of each group [bar]: fp32 tensors 8e-8 .. 9.6e-7 [3e-5] (dA at 8T + 1 in two segments the
largest), bf16-stored tensors 1.0e-3 .. 2.7e-3 [2^-7]: the figures of the unsegmented entry on the same inputs."""
import pytest
import torch

import scan_bwd_ref as SB
import test_gpu_scan_bwd as GS

pytestmark = pytest.mark.gpu

DEV = GS.DEV


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def run_seg(ops, x, reverse, bf, segments, poison=False, seg_entry=False):
    d = GS.to_dev(x, bf)
    g = ops.selective_scan_bwd(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["delta_bias"], d["dout"], reverse=reverse,
                               poison=poison, segments=segments, seg_entry=seg_entry)
    torch.cuda.synchronize()
    return g, dict(u=g.du, delta=g.ddelta, A=g.dA, B=g.dB, C=g.dC, D=g.dD, z=g.dz, delta_bias=g.ddelta_bias)


def handover_cases():
    T = GS.T_()
    return [(T + 1, 4), (3 * T + 4, 4), (3 * T + 4, 3), (8 * T + 1, 2), (8 * T + 1, 3), (8 * T + 1, 8)]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("LG", handover_cases())
def test_carry_handovers(ops, LG, reverse):
    L, G = LG
    steps = ops.scan_bwd_seg_steps(L, G)
    x, g64, dev32 = GS.case("chunks", 2, 128, L, reverse)
    _, got = run_seg(ops, x, reverse, False, G)
    GS.hold(f"L={L} G={G} ({-(-L // steps)} segments of {steps}) rev={reverse}", got, g64, dev32)


@pytest.mark.parametrize("bare", [False, True])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("form", ["short_strand", "one_segment"])
def test_one_effective_segment_is_the_unsegmented_call(ops, form, bf, bare):
    """L = T at segments = 4 (one segment of T steps) and L = 2T + 3 at segments = 1 straight through the new entry: the unsegmented
    kernel runs, every output has pcad_selective_scan_bwd's bits"""
    T = GS.T_()
    L, G = (T, 4) if form == "short_strand" else (2 * T + 3, 1)
    assert -(-L // ops.scan_bwd_seg_steps(L, G)) == 1
    x = SB.inputs(7 * L, 2, 128, L, bf)
    if bare:
        x["z"] = x["D"] = x["delta_bias"] = None
    _, ref = GS.run_raw(ops, x, True, bf)
    _, got = run_seg(ops, x, True, bf, G, seg_entry=True)
    for name in SB.NAMES:
        if name in ("z", "D", "delta_bias") and bare:
            assert (got[name] is None) == (ref[name] is None), name       # dz is None; dD / dbias are the zero operands' gradients
            if got[name] is None:
                continue
        assert got[name].dtype == ref[name].dtype and torch.equal(got[name], ref[name]), name


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", ["three_waves", "three_strands"])
def test_channel_strand_and_segment_partials(ops, shape, bf, reverse):
    T = GS.T_()
    Bsz, E, L, G = (2, 192, 3 * T + 4, 4) if shape == "three_waves" else (3, 64, 8 * T + 1, 3)
    x, g64, dev32 = GS.case("partials", Bsz, E, L, reverse, bf)
    _, got = run_seg(ops, x, reverse, bf, G)
    assert got["u"].dtype == (torch.bfloat16 if bf else torch.float32) and got["B"].dtype == torch.float32
    GS.hold(f"{shape} G={G} bf={bf} rev={reverse}", got, g64, dev32, GS.BF_STORED if bf else ())


@pytest.mark.parametrize("bf", [False, True])
def test_reproducible_complete_in_bounds(ops, bf):
    T = GS.T_()
    x, g64, dev32 = GS.case("partials", 2, 192, 3 * T + 4, True, bf)
    _, a = run_seg(ops, x, True, bf, 4)
    _, b = run_seg(ops, x, True, bf, 4)
    gp, p = run_seg(ops, x, True, bf, 4, poison=True)
    for name in SB.NAMES:
        assert torch.equal(a[name], b[name]), name                       # the same call twice
        assert not torch.isnan(p[name]).any(), name                      # every element written, nothing read that was not written
        assert torch.equal(a[name], p[name]), name                       # ... and the scratch's prior content does not matter
    assert gp.guards_ok                                                  # one row before and after every output untouched


def _leaves(d):
    out = {}
    for k in SB.NAMES:
        t = d[k]
        out[k] = (t.transpose(1, 2).contiguous().transpose(1, 2) if t.dim() == 3 else t.clone()).requires_grad_(True)
    return out


@pytest.mark.parametrize("bf", [False, True])
def test_autograd_surface(ops, bf):
    """ops.selective_scan_fn(..., segments=4) on non-contiguous leaves at L = 2T + 1 (three segments of T, T, 1): the output has
    segments=1's bits - the forward is the same call -, .backward() fills .grad in each input's shape and dtype within the bars"""
    T = GS.T_()
    Bsz, E, L = 2, 128, 2 * T + 1
    x, g64, dev32 = GS.case("chunks", Bsz, E, L, False, bf)
    d = GS.to_dev(x, bf)
    leaves, plain = _leaves(d), _leaves(d)
    assert not leaves["u"].is_contiguous() and not leaves["B"].is_contiguous()
    call = lambda lv, **kw: ops.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], z=lv["z"],
                                                  delta_bias=lv["delta_bias"], delta_softplus=True, **kw)
    out, ref = call(leaves, segments=4), call(plain)
    assert out.grad_fn is not None and torch.equal(out, ref)
    out.backward(d["dout"].transpose(1, 2).contiguous().transpose(1, 2))
    for k in SB.NAMES:
        assert leaves[k].grad.shape == leaves[k].shape and leaves[k].grad.dtype == leaves[k].dtype, k
    GS.hold(f"autograd segments=4 bf={bf}", {k: leaves[k].grad for k in SB.NAMES}, g64, dev32, ("u", "delta", "z", "B", "C") if bf else ())
    with pytest.raises(NotImplementedError):
        call(leaves, segments=4, accumulate_into=ref.detach())
    with pytest.raises(ValueError):
        call(leaves, segments=65)


def test_auto_resolves_and_runs(ops):
    """a strand of 2 SCAN_BWD_SEG_MIN_STEPS + 5 steps, two strands of two waves: "auto" cuts it (far below the device's wave slots) into
    as many segments as the minimum length allows; the gradients are those of that explicit count, bit for bit, and hold the bars"""
    L = 2 * ops.SCAN_BWD_SEG_MIN_STEPS + 5
    with torch.cuda.device(DEV):
        G = ops.scan_bwd_auto_segments(2, L, 128)
    assert G >= 2 and ops.scan_bwd_seg_steps(L, G) >= ops.SCAN_BWD_SEG_MIN_STEPS
    x, g64, dev32 = GS.case("auto", 2, 128, L, False)
    d = GS.to_dev(x, False)
    res = {}
    for segments in ("auto", G):
        lv = {k: d[k].clone().requires_grad_(True) for k in SB.NAMES}
        out = ops.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], z=lv["z"], delta_bias=lv["delta_bias"],
                                    delta_softplus=True, segments=segments)
        out.backward(d["dout"])
        res[segments] = {k: lv[k].grad for k in SB.NAMES}
    for k in SB.NAMES:
        assert torch.equal(res["auto"][k], res[G][k]), k
    GS.hold(f"auto -> {G} segments at L={L}", res["auto"], g64, dev32)
