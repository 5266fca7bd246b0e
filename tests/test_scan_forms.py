"""CPU checks behind tests/test_gpu_engine_forms.py: the float64 reference of tests/scan_ref.py agrees with the fp32 oracle, the
segment carry identity holds in it, its inputs would show a lost carry, and the shapes of the GPU cases give the launch forms the
GPU file names (tests/launch_forms.py, the restatement of csrc/kernels.hpp / csrc/convx.hip that tests/test_launch_forms.py pins
to the library).

Sensitivity, measured here (the least change, among the 32 rows after any one boundary of either direction, that dropping the
carried state in float64 makes to the gate-once and gate-each outputs, per-row metric; needed: 100 x the bar of the case):
    fp32  segmented 1.67 .. 1.88, pair seam 1.79 .. 2.01 = 1 400 .. 29 000 x the bar of the sums (6e-5, or 8 x the oracle's row)
    bf16  segmented 1.67 .. 1.88, pair seam 1.80 .. 2.00 = 107 .. 128 x the 2^-6 the sums are held to
A change above 1 - needed for bf16, where 100 x 2^-6 = 1.56 - takes channels whose own output is smaller than what their carried
state contributes to it: the latched channels of scan_ref.make_direction, whose skip term D u opposes <h, C_t> inside one
direction's fp32 arithmetic (so no bf16 rounding is amplified by the cancellation)."""
import pytest
import torch

import scan_ref as R
from launch_forms import convx_ksplit, scan_pair_wanted, scan_segments
from oracle import caduceus_oracle as O


def relerr(a, b):
    return ((a.double() - b.double()).abs().max() / b.double().abs().max()).item()


@pytest.mark.parametrize("bf", [False, True])
def test_reference_scan_agrees_with_the_fp32_oracle(bf):
    """float64 reference cast to fp32 vs oracle.selective_scan_fn on the same inputs, each direction gated, at test_gpu_ops.py's bars
    (test_selective_scan_fp32 2e-5; bf16 2^-7 with the same rounding points)"""
    S, L, E, Rp = 2, 70, 128, 64
    case, yf, yr = R.walks_for(S, L, E, Rp, bf)
    rnd, ornd = (R.bf16, O.round_bf16) if bf else (R.ident, O._ident)
    outs = R.combine(yf, yr, case["z"], "strict", rnd)
    for d, rev, ref in ((case["fwd"], False, outs[0]), (case["rev"], True, outs[1])):
        f = (lambda t: t.flip(1)) if rev else R.ident
        delta = ornd(torch.einsum("slr,er->sle", d["dt_low"], d["Wdt"]))
        y = O.selective_scan_fn(f(d["u"]).transpose(1, 2), f(delta).transpose(1, 2), d["A"], f(d["B"]).transpose(1, 2),
                                f(d["C"]).transpose(1, 2), d["D"], z=f(case["z"]).transpose(1, 2), delta_bias=d["dbias"],
                                delta_softplus=True, rnd=ornd)
        assert relerr(ref.float(), f(y.transpose(1, 2))) < (2.0 ** -7 if bf else 2e-5)


def test_reference_conv_xproj_agrees_with_the_fp32_oracle():
    g = torch.Generator().manual_seed(5)
    S, L, E, Rr = 2, 45, 128, 24
    x = torch.randn(S, L, E, generator=g)
    wf, wr = (torch.randn(E, 4, generator=g) * 0.5 for _ in range(2))
    bf_, br = (torch.randn(E, generator=g) * 0.5 for _ in range(2))
    xpf, xpr = (torch.randn(Rr + 32, E, generator=g) * E ** -0.5 for _ in range(2))
    xcf, xcr, df, dr = R.conv_xproj(x, wf, bf_, wr, br, xpf, xpr)
    of = O.causal_conv1d_fn(x.transpose(1, 2), wf, bf_, activation="silu").transpose(1, 2)
    orv = O.causal_conv1d_fn(x.transpose(1, 2).flip(-1), wr, br, activation="silu").flip(-1).transpose(1, 2)
    assert relerr(xcf.float(), of) < 1e-5 and relerr(xcr.float(), orv) < 1e-5
    assert relerr(df.float(), torch.einsum("sle,re->slr", of, xpf)) < 3e-5
    assert relerr(dr.float(), torch.einsum("sle,re->slr", orv, xpr)) < 3e-5


def test_split_hi_lo():
    v = torch.randn(4096, generator=torch.Generator().manual_seed(2)) * torch.logspace(-6, 6, 4096)
    hi, lo = R.split_hi_lo(v)
    assert hi.dtype == lo.dtype == torch.bfloat16 and torch.equal(hi, v.bfloat16())
    assert torch.equal(lo, (v - hi.float()).bfloat16())
    assert ((hi.double() + lo.double() - v.double()).abs() <= v.double().abs() * 2.0 ** -16).all()
    ok = (hi.float() + lo.float()).bfloat16() == hi
    assert R.hi_rounds_sum(hi, lo).all() and ok.float().mean() > 0.99         # all but the exact ties (scan_ref.hi_rounds_sum)


def test_inputs_cover_the_softplus_regimes():
    case = R.case_for(2, 64, 128, 64, False)
    for d in (case["fwd"], case["rev"]):
        raw = torch.einsum("slr,er->sle", d["dt_low"].double(), d["Wdt"].double()) + d["dbias"].double()
        assert (raw[..., list(R.HOT)] > 20).all() and (raw[..., list(R.COLD)] < -10).all() and (raw[..., list(R.COLD)] > -14).all()
        sp = torch.nn.functional.softplus(d["dbias"][max(R.COLD) + 1:].double())
        assert sp.min() >= 1e-3 * 0.999 and sp.max() <= 0.1 * 1.001 and sp.max() / sp.min() > 30


@pytest.mark.parametrize("shape", list(R.SEG_SHAPES))
def test_segment_carry_identity(shape):
    """the strand cut at the kernels' segment boundaries and recombined with h0[g] = exp(A sum delta) (.) h0[g-1] + h_end[g-1] equals
    the uncut walk to 1e-12, both directions"""
    S, L, E = shape
    G, sb = R.SEG_SHAPES[shape]
    case, yf, yr = R.walks_for(S, L, E, 64, False)
    bounds = R.segment_bounds(L, G, sb)
    assert len(bounds) == G and bounds[-1][1] == L and all(b[0] < b[1] for b in bounds)
    for d, rev, y in ((case["fwd"], False, yf), (case["rev"], True, yr)):
        cut = R.walk_cut(d, bounds, rev)
        assert not torch.isnan(cut).any()
        assert relerr(cut, y) < 1e-12


def _sensitivity(S, L, E, bf, boundaries):
    """-> (worst change, worst change / bar): over the boundaries (walk steps) of both directions and the 32 rows after each, the
    change a dropped carry makes to the gate-once and the gate-each output, in the per-row metric.  Only the 32 rows are walked
    again, from a zero state; every other row of the reference is unchanged by the drop."""
    case, yf, yr = R.walks_for(S, L, E, 64, bf)
    rnd = R.bf16 if bf else R.ident
    worst, ratio = float("inf"), float("inf")
    for s0 in boundaries:
        n = min(32, L - s0)
        for d, rev in (("fwd", False), ("rev", True)):
            rows = slice(L - s0 - n, L - s0) if rev else slice(s0, s0 + n)
            dropped = R.walk(case[d], rev, rnd, steps=(s0, s0 + n))[0][:, rows]
            f, r, z = yf[:, rows], yr[:, rows], case["z"][:, rows]
            for mode in ("gate_once", "gate_each"):
                got = R.combine(f, dropped, z, mode) if rev else R.combine(dropped, r, z, mode)
                e = R.row_err(got, R.combine(f, r, z, mode)).min().item()
                worst, ratio = min(worst, e), min(ratio, e / R.scan_bar(S, L, E, 64, bf, mode))
    return worst, ratio


@pytest.mark.parametrize("bf", [False, True], ids=["fp32", "bf16"])
def test_a_dropped_carry_shows(bf):
    """A condition on the inputs: for every segmented and pair case of the GPU file, the carried state dropped at any one boundary
    (each segment start; the L / 2 seam of a pair walk) changes each of the 32 rows after it by at least 100 x the bar the case is
    tested at (scan_ref.scan_bar: sums of two directions, so twice the single-direction bar).  Figures: module docstring."""
    rows = []
    for (S, L, E), (G, sb) in R.SEG_SHAPES.items():
        rows.append((f"segmented S={S} L={L} E={E}",) + _sensitivity(S, L, E, bf, [b[0] for b in R.segment_bounds(L, G, sb)[1:]]))
    for (S, L, E) in R.PAIR_SHAPES:
        rows.append((f"pair S={S} L={L} E={E}",) + _sensitivity(S, L, E, bf, [L // 2]))
    for name, w, ratio in rows:
        print(f"sensitivity {'bf16' if bf else 'fp32'} {name}: worst row changes by {w:.3e} = {ratio:.0f} x its bar (needed: 100 x)")
    assert all(ratio >= 100 for _, _, ratio in rows), [r for r in rows if r[2] < 100]


def test_shapes_give_the_stated_forms():
    for (S, L, E), want in R.SEG_SHAPES.items():
        assert scan_segments(S, L, E) == want, (S, L, E, scan_segments(S, L, E))
    # the notes of the table: block counts per segment and the steps of the last block
    blocks = lambda L, G, sb: [-(-(min(L, (g + 1) * sb * 32) - g * sb * 32) // 32) for g in range(G)]
    assert blocks(256, 8, 1) == [1] * 8
    assert blocks(296, 10, 1) == [1] * 10 and 296 - 9 * 32 == 8
    assert blocks(300, 10, 1) == [1] * 10 and 300 - 9 * 32 == 12 and 300 % 8
    assert blocks(544, 9, 2) == [2] * 8 + [1]
    assert blocks(2072, 4, 17) == [17, 17, 17, 14] and 2072 - 64 * 32 == 24
    # policy_S: strand 0 launched alone under policy_S = 2 takes the S = 2 launch's form
    for (S, L, E) in R.SEG_SHAPES:
        if S == 2:
            assert scan_segments(1, L, E)[0] > 1
    # pair: what the kernel needs of L, and a call size at which the engine's policy picks the pair form at this L and E
    for (S, L, E) in R.PAIR_SHAPES:
        assert L % 64 == 0 and L >= 128 and scan_pair_wanted(520, L, E)
    # plain walks never segment without scratch; L = 44 is the one length off the 8-row groups
    assert [L % 8 for L in R.PLAIN_L] == [0, 0, 4, 0, 0]
    for (E, bf), ks in R.CONVX_KS.items():
        for L in R.CONVX_L:
            assert convx_ksplit(2, L, E, bf) == ks, (E, bf, L)
            assert convx_ksplit(1, L, E, bf) >= ks          # policy_S = 2 on one strand: the policy, not the launch, picks ks
