"""-m gpu: the segmented training forward of the selective scan (csrc/scan_fwd_seg.hip through pcad_selective_scan_fwd_seg,
ops.selective_scan_fwd_seg and the `fwd_segments` keyword of ops.selective_scan_fn) against the float64 CPU recurrence of
tests/scan_bwd_ref.py (`forward`).

Operands, `to_dev` and the metric - max |got - ref| / max |ref| over the output - are tests/test_gpu_scan_bwd.py's and scan_bwd_ref's; the
bars are the project's BAR_SCAN, 3e-5 for fp32 and 2^-7 for a bf16-stored output.  Every figure is printed before its assertion.  The
float64 outputs are computed once per case and shared (scan_ref.cached).

Shapes, with T = ops.SCAN_BWD_CHUNK: the backward file's hand-overs - two segments the second of one step (L = T + 1), segments of one
chunk with a part chunk at the end (3T + 4 at G = 4), of two and three chunks (3T + 4 at G = 3; 8T + 1 at G = 2, 3, 8), so that with three
and more effective segments a missing P_g in the carry would show (tests/test_scan_fwd_seg.py shows that it would, by > 1e-4) -, E = 192
(three waves) and three strands in both dtypes, the bare form, one effective segment (today's call bit for bit through
selective_scan_fn), and one strand length past 2 SCAN_BWD_SEG_MIN_STEPS, where "auto" picks more than one segment."""
import pytest
import torch

import scan_bwd_ref as SB
import scan_ref as R
import test_gpu_scan_bwd as GS

pytestmark = pytest.mark.gpu

DEV = GS.DEV


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def out64(key, Bsz, E, L, reverse, bf=False, bare=False):
    """(the inputs of test_gpu_scan_bwd.case - shared with its gradient references -, the float64 output), computed once"""
    x = GS.case(key, Bsz, E, L, reverse, bf, bare)[0]
    return x, R.cached(("scan_fwd_seg", key, Bsz, E, L, bf, bare, reverse), lambda: SB.forward(x, reverse))


def run_seg(ops, x, reverse, bf, segments, poison=False):
    d = GS.to_dev(x, bf)
    r = ops.selective_scan_fwd_seg(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], d["z"], d["delta_bias"], reverse=reverse,
                                   segments=segments, poison=poison)
    torch.cuda.synchronize()
    return r


def run_fn(ops, x, reverse, bf, **kw):
    d = GS.to_dev(x, bf)
    y = ops.selective_scan_fn(d["u"], d["delta"], d["A"], d["B"], d["C"], d["D"], z=d["z"], delta_bias=d["delta_bias"], delta_softplus=True,
                              reverse=reverse, **kw)
    torch.cuda.synchronize()
    return y


def hold(tag, got, ref, bf):
    m, bar = SB.metric(got, ref), R.BAR_SCAN[bool(bf)]
    print(f"{tag}: {m:.2e} [{bar:.1e}]")
    assert m <= bar, (tag, m, bar)
    return m


def handover_cases():
    T = GS.T_()
    return [(T + 1, 4), (3 * T + 4, 4), (3 * T + 4, 3), (8 * T + 1, 2), (8 * T + 1, 3), (8 * T + 1, 8)]


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("LG", handover_cases())
def test_carry_handovers(ops, LG, reverse):
    L, G = LG
    steps = ops.scan_bwd_seg_steps(L, G)
    x, ref = out64("chunks", 2, 128, L, reverse)
    r = run_seg(ops, x, reverse, False, G)
    assert r.segments == G and r.out.shape == ref.shape and r.out.dtype == torch.float32
    tag = f"L={L} G={G} ({-(-L // steps)} segments of {steps}) rev={reverse}"
    plain = run_fn(ops, x, reverse, False)
    print(f"{tag}: from the plain call {SB.metric(r.out, plain):.2e} (printed only)")
    hold(tag, r.out, ref, False)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("shape", ["three_waves", "three_strands"])
def test_channels_strands_and_dtypes(ops, shape, bf, reverse):
    T = GS.T_()
    Bsz, E, L, G = (2, 192, 3 * T + 4, 4) if shape == "three_waves" else (3, 64, 8 * T + 1, 3)
    x, ref = out64("partials", Bsz, E, L, reverse, bf)
    r = run_seg(ops, x, reverse, bf, G)
    assert r.out.dtype == (torch.bfloat16 if bf else torch.float32)
    hold(f"{shape} G={G} bf={bf} rev={reverse}", r.out, ref, bf)


@pytest.mark.parametrize("reverse", [False, True])
def test_ungated_without_skip_and_bias(ops, reverse):
    """z = None, D = None, delta_bias = None at L = 2T + 1 in three segments: the ungated kernel"""
    L = 2 * GS.T_() + 1
    x, ref = out64("bare", 2, 128, L, reverse, bare=True)
    r = run_seg(ops, x, reverse, False, 4)
    hold(f"bare rev={reverse}", r.out, ref, False)


@pytest.mark.parametrize("bf", [False, True])
@pytest.mark.parametrize("form", ["default", "short_strand"])
def test_one_effective_segment_is_todays_call(ops, form, bf):
    """fwd_segments=1, and fwd_segments=4 at L = T (one segment of T steps), through selective_scan_fn: pcad_selective_scan runs and
    the output has the bits of the call without the keyword"""
    T = GS.T_()
    L, G = (2 * T + 3, 1) if form == "default" else (T, 4)
    assert -(-L // ops.scan_bwd_seg_steps(L, G)) == 1
    x = SB.inputs(7 * L, 2, 128, L, bf)
    for reverse in (False, True):
        ref = run_fn(ops, x, reverse, bf)
        got = run_fn(ops, x, reverse, bf, fwd_segments=G)
        assert got.dtype == ref.dtype and torch.equal(got, ref), reverse


@pytest.mark.parametrize("bf", [False, True])
def test_reproducible_complete_in_bounds(ops, bf):
    T = GS.T_()
    x, ref = out64("partials", 2, 192, 3 * T + 4, True, bf)
    a = run_seg(ops, x, True, bf, 4)
    b = run_seg(ops, x, True, bf, 4)
    p = run_seg(ops, x, True, bf, 4, poison=True)
    assert torch.equal(a.out, b.out)                                     # the same call twice
    assert not torch.isnan(p.out).any()                                  # every element written, nothing read that was not written
    assert torch.equal(a.out, p.out)                                     # ... and the scratch's prior content does not matter
    assert p.guards_ok                                                   # one row before and after the output untouched
    hold(f"poisoned bf={bf}", p.out, ref, bf)


def _leaves(d):
    out = {}
    for k in SB.NAMES:
        t = d[k]
        out[k] = (t.transpose(1, 2).contiguous().transpose(1, 2) if t.dim() == 3 else t.clone()).requires_grad_(True)
    return out


@pytest.mark.parametrize("bf", [False, True])
def test_autograd_surface(ops, bf):
    """ops.selective_scan_fn(..., fwd_segments=4, segments=4) on non-contiguous leaves at L = 2T + 1 (three segments of T, T, 1): the
    output holds the bar, .backward() fills .grad in each input's shape and dtype within test_gpu_scan_bwd's bars (the backward reads
    only the saved inputs, so it is the one of fwd_segments=1)"""
    T = GS.T_()
    Bsz, E, L = 2, 128, 2 * T + 1
    x, g64, dev32 = GS.case("chunks", Bsz, E, L, False, bf)
    _, ref = out64("chunks", Bsz, E, L, False, bf)
    d = GS.to_dev(x, bf)
    leaves = _leaves(d)
    assert not leaves["u"].is_contiguous() and not leaves["B"].is_contiguous()
    call = lambda lv, **kw: ops.selective_scan_fn(lv["u"], lv["delta"], lv["A"], lv["B"], lv["C"], lv["D"], z=lv["z"],
                                                  delta_bias=lv["delta_bias"], delta_softplus=True, **kw)
    out = call(leaves, fwd_segments=4, segments=4)
    assert out.grad_fn is not None and out.shape == leaves["u"].shape and out.dtype == leaves["u"].dtype
    hold(f"autograd fwd_segments=4 bf={bf} output", out, ref, bf)
    with torch.no_grad():
        assert torch.equal(call(leaves, fwd_segments=4), out)            # without grad: the same entry, the same bits
    out.backward(d["dout"].transpose(1, 2).contiguous().transpose(1, 2))
    for k in SB.NAMES:
        assert leaves[k].grad.shape == leaves[k].shape and leaves[k].grad.dtype == leaves[k].dtype, k
    GS.hold(f"autograd fwd_segments=4 segments=4 bf={bf}", {k: leaves[k].grad for k in SB.NAMES}, g64, dev32,
            ("u", "delta", "z", "B", "C") if bf else ())
    with pytest.raises(NotImplementedError):
        call(leaves, fwd_segments=4, accumulate_into=out.detach())
    with torch.no_grad(), pytest.raises(NotImplementedError):
        call(leaves, fwd_segments=4, accumulate_into=out.detach())
    with pytest.raises(ValueError):
        call(leaves, fwd_segments=65)


def test_auto_resolves_and_runs(ops):
    """a strand of 2 SCAN_BWD_SEG_MIN_STEPS + 5 steps, two strands of two waves: "auto" cuts it (far below the device's wave slots) into
    as many segments as the minimum length allows; the output is that explicit count's, bit for bit, and holds the bar"""
    L = 2 * ops.SCAN_BWD_SEG_MIN_STEPS + 5
    with torch.cuda.device(DEV):
        G = ops.scan_fwd_auto_segments(2, L, 128)
        assert G == ops.scan_bwd_auto_segments(2, L, 128)                # four waves: far from the shapes the forward's policy cuts back
    assert G >= 2 and ops.scan_bwd_seg_steps(L, G) >= ops.SCAN_BWD_SEG_MIN_STEPS
    x, ref = out64("auto", 2, 128, L, False)
    auto, explicit = run_fn(ops, x, False, False, fwd_segments="auto"), run_fn(ops, x, False, False, fwd_segments=G)
    assert torch.equal(auto, explicit)
    assert run_seg(ops, x, False, False, "auto").segments == G
    hold(f"auto -> {G} segments at L={L}", auto, ref, False)
