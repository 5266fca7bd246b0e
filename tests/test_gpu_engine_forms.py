"""-m gpu: the scan and conv + x_proj kernels in the instantiations and launch forms the ENGINE runs (csrc/forward.hip), through the
operator entries pcad_selective_scan_engine / pcad_selective_scan_pair / pcad_conv_xproj_bidir_engine, against the float64
reference of tests/scan_ref.py.

Metric: per row (strand, t) max_c |got - ref| / max_c |ref| over the row's own channels, worst row (scan_ref.row_err) - an error on a
few rows is not diluted by the tensor's maximum.  Bars: the project's own (tests/test_gpu_ops.py), for fp32 raised to 8 x the fp32
CPU oracle's worst row against the same reference where that is larger (scan_ref.scan_bar); sums of two directions twice the
single-direction bar.  Every case prints its worst row.

Which instantiation each group runs (csrc/scan.hip launch_scan / launch_scan_pair, csrc/convx.hip launch_convx):
  plain, L % 8 == 0   scan_kernel<bf16, ., ., ., FUSED, PRE 64 | 96, BLK8, SEG 0, ZB>  /  <float, ., ., ., FUSED, 0, BLK8, 0, ZB>
                      (launch_scan_t<bf16_t, true, 64 | 96, true, true>, <float, true, 0, true, true>) in the four (REV, ACC, HASZ)
                      combinations (0, 0, 0), (1, 2, 1), (1, 1, 1) after (0, 0, 1), and (1, 0, 1)
  plain, L = 44       launch_scan_t<bf16_t, true, 64> / <bf16_t, true> (Rp 96) / <float, true>: run-time layouts (uyb, zblk as arguments)
  segmented           the BLK8 instantiations with SEG 1 (pass A), scan_carry_kernel, SEG 2 (pass B); L = 300: the run-time-layout ones
  pair                scan_pair_kernel<T, ACC 0, HASZ gate_each, PRE, PHASE 3> then <T, ACC 2 | 1, true, PRE, 4> (scan_body SEG 3 / 4)
  walk_len            the plain BLK8 instantiations with Lw < L
  dt_split            <float, ...> with dts = 1: DeltaTileSplit::run64 (Rp 64) and ::run (Rp 96), plain and pair
  ysplit              scan_kernel<float, true, 2 | 1, true, true, 0, true, 0, true, SPLITY> and scan_pair_kernel<float, ., ., 0, 4, SPLITY>
  conv + x_proj       convx_kernel<T, ZFILL, NJ 6 | 8> on a dim3(tiles, ks) grid + convx_reduce_kernel<T>; dtl_split + w_split:
                      convx_kernel<float, ZFILL, 6, XS = true>, alone and on the K-split grid

hi == bf16(hi + lo) holds for every element but the exact ties the definition itself produces (scan_ref.hi_rounds_sum); beside it
the tests assert the stronger statement that (hi, lo) is, bit for bit, split_hi_lo of the fp32 y the same launch writes without ysplit.

Worst rows observed on an MI355X: the maximum over the shapes and outputs of each group [the bar; for fp32 the largest of the
group].  The latched channels of scan_ref.make_direction put out 0.4 of what their state contributes, so fp32 rounding shows ~2.5 x
larger on them than on ordinary channels - in the kernels and in the fp32 CPU oracle alike, which is where the fp32 bars above the
project's 3e-5 / 6e-5 come from (8 x the oracle's own worst row, scan_ref.scan_bar).  A bf16 row is off by one bf16 step of its
largest channel at most (a rounding that falls the other way), which is below 2^-7 of the row's maximum.
  plain      bf16 Rp 64   one direction 7.0e-3 [2^-7 = 7.8e-3]   sums 7.0e-3 [2^-6 = 1.6e-2]
             bf16 Rp 96   one direction 4.6e-3 [7.8e-3]           sums 6.6e-3 [1.6e-2]
             fp32         one direction 2.2e-5, sums 2.2e-5 [1.2e-4]
  segmented  bf16         one direction 7.7e-3 [7.8e-3]           sums 7.6e-3 [1.6e-2]
             fp32         one direction 7.1e-5 [5.4e-4 .. 1.2e-3], sums 7.1e-5 [1.2e-3]
             fp32 against the same launch unsegmented: 1.1e-4 [twice the above: 1.1e-3 .. 2.4e-3]
  pair       bf16 Rp 64   7.0e-3   bf16 Rp 96   7.3e-3   [1.6e-2], gate once and gate each alike
             fp32         1.9e-5 (rows next to the seam 8.7e-6) [1.6e-4]
  dt_split   Rp 64 / 96   plain: one direction 2.8e-6 [3e-5 .. 3.4e-5], sums 2.8e-6 [6e-5];  pair 9.4e-6 (seam 3.5e-6) [6.2e-5 .. 7.3e-5]
  ysplit     hi + lo: plain 7.4e-6 [6e-5], pair 1.5e-5 [6.2e-5]
  conv + x_proj K-split   bf16: xc 8.0e-4, x_dbl 4.4e-3 [7.8e-3];  fp32: xc 2.1e-7 [1e-5], x_dbl 4.6e-7 [3e-5], x_dbl against the
             unsplit call 1.3e-6 [6e-5]
  dtl_split + w_split     xc 2.4e-7 [1e-5], x_dbl 1.2e-5 [2e-5], the same alone and on the K-split grid
"""
import pytest
import torch

import scan_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
LOG2E = 1.4426950408889634
VARIANTS = [(True, 64), (True, 96), (False, 64)]                 # (bf16, Rp): bf16 PRE 64, bf16 PRE 96, fp32
VID = ["bf16-Rp64", "bf16-Rp96", "fp32"]


@pytest.fixture(scope="module")
def ops():
    from plantcaduceus_amd import ops as _ops
    return _ops


def tdtype(bf):
    return torch.bfloat16 if bf else torch.float32


def gpu_dir(d, Rp, bf, dt_split=False):
    """one direction of a scan_ref case -> the operands ops.selective_scan_engine takes, on the GPU"""
    dt = tdtype(bf)
    S, L, Rr = d["dt_low"].shape
    dl = torch.zeros(S, L, Rp)
    dl[..., :Rr] = d["dt_low"]
    W = torch.zeros(d["Wdt"].shape[0], Rp)
    W[:, :Rr] = d["Wdt"]
    if dt_split:                                                  # [hi | lo] operands (scan_ref.split_hi_lo)
        dl, W = (torch.cat(R.split_hi_lo(t), dim=-1) for t in (dl, W))
    else:
        dl, W = dl.to(dt), W.to(dt)
    return dict(u=d["u"].to(dt).to(DEV), dt_low=dl.to(DEV), Wdt=W.to(DEV), bc=torch.cat([d["B"], d["C"]], -1).to(DEV),
                A2=(d["A"] * LOG2E).to(DEV), D=d["D"].to(DEV), delta_bias=d["dbias"].to(DEV))


def scan(ops, g, Rp, **kw):
    return ops.selective_scan_engine(g["u"], g["dt_low"], g["Wdt"], Rp, g["bc"], g["A2"], g["D"], g["delta_bias"], **kw)


def worst(got, ref):
    assert not torch.isnan(got).any(), "a row the kernel must write was left NaN"
    return R.row_err(got, ref).max().item()


def check(name, got, ref, bar, seam=None):
    e = worst(got, ref)
    extra = ""
    if seam is not None:
        extra = f", rows next to the L/2 seam {R.row_err(got, ref)[:, seam - 2:seam + 2].max().item():.2e}"
    print(f"{name}: worst row {e:.2e} (bar {bar:.2e}){extra}")
    assert e < bar, f"{name}: worst row {e:.3e} >= bar {bar:.3e}"
    return e


def both_directions(ops, S, L, E, Rp, bf, segmented=False, dt_split=False):
    """The launches the engine issues for one layer, on the case of the shape.
    -> dict: fwd (ungated), once (reverse accumulate 2 on fwd), fwd_g (forward gated), each (reverse accumulate 1 on fwd_g),
    rev_g (reverse gated, accumulate 0), case, refs (float64, rounded where the launches round), names -> bars"""
    case, yf, yr = R.walks_for(S, L, E, Rp, bf)
    rnd = R.bf16 if bf else R.ident
    gf, gr = gpu_dir(case["fwd"], Rp, bf, dt_split), gpu_dir(case["rev"], Rp, bf, dt_split)
    z = case["z"].to(tdtype(bf)).to(DEV)
    kw = dict(segmented=segmented, dt_split=dt_split)
    o = dict(case=case, gf=gf, gr=gr, z=z)
    o["fwd"] = scan(ops, gf, Rp, **kw)
    o["once"] = scan(ops, gr, Rp, z=z, y_prior=o["fwd"].y, reverse=True, accumulate=2, **kw)
    o["fwd_g"] = scan(ops, gf, Rp, z=z, **kw)
    o["each"] = scan(ops, gr, Rp, z=z, y_prior=o["fwd_g"].y, reverse=True, accumulate=1, **kw)
    o["rev_g"] = scan(ops, gr, Rp, z=z, reverse=True, **kw)
    sf, sr = R.combine(yf, yr, case["z"], "strict", rnd)
    o["refs"] = dict(fwd=rnd(yf), once=R.combine(yf, yr, case["z"], "gate_once", rnd), fwd_g=sf,
                     each=R.combine(yf, yr, case["z"], "gate_each", rnd), rev_g=sr)
    o["bars"] = dict(fwd=R.scan_bar(S, L, E, Rp, bf, "fwd"), once=R.scan_bar(S, L, E, Rp, bf, "gate_once"),
                     fwd_g=R.scan_bar(S, L, E, Rp, bf, "strict"), each=R.scan_bar(S, L, E, Rp, bf, "gate_each"),
                     rev_g=R.scan_bar(S, L, E, Rp, bf, "strict"))
    return o


OUTS = ("fwd", "once", "fwd_g", "each", "rev_g")


# ---- plain walks in the engine's layouts ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", R.PLAIN_L)
@pytest.mark.parametrize("bf,Rp", VARIANTS, ids=VID)
def test_scan_plain(ops, bf, Rp, L):
    S, E = 2, 128
    o = both_directions(ops, S, L, E, Rp, bf)
    for k in OUTS:
        check(f"plain {VID[VARIANTS.index((bf, Rp))]} L={L} {k}", o[k].y, o["refs"][k], o["bars"][k])
        assert o[k].pad.numel() == 0                         # 2 L rows: whole 8-row groups at every L here
    if L == 44:
        # S L % 8 != 0: strand 0 alone leaves 4 padding rows in the blocked y, which are not the kernel's to write
        g0 = {k: (v[:1] if v.dim() == 3 else v) for k, v in o["gf"].items()}
        one = scan(ops, g0, Rp, z=o["z"][:1])
        assert one.pad.shape[0] == 4 and torch.isnan(one.pad).all()
        assert torch.equal(one.y, o["fwd_g"].y[:1])


# ---- segmented: pass A, carry, pass B ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", list(R.SEG_SHAPES), ids=lambda s: "S%d-L%d-E%d" % s)
@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp32"])
def test_scan_segmented(ops, bf, shape):
    S, L, E = shape
    G, _ = R.SEG_SHAPES[shape]
    Rp = 64
    o = both_directions(ops, S, L, E, Rp, bf, segmented=True)
    assert o["fwd"].seg_bytes == S * G * E * 17 * 4          # the scratch of G segments: the form ran
    p = both_directions(ops, S, L, E, Rp, bf)                # the same launches, seg_ws = NULL
    for k in OUTS:
        name = f"segmented {'bf16' if bf else 'fp32'} S={S} L={L} G={G} {k}"
        check(name, o[k].y, o["refs"][k], o["bars"][k])
        if not bf:
            check(name + " vs unsegmented", o[k].y, p[k].y, 2 * o["bars"][k])
    if S == 2:                                               # policy_S: strand 0 alone runs the S = 2 launch's form, bit for bit
        g0 = {k: (v[:1] if v.dim() == 3 else v) for k, v in o["gf"].items()}
        g1 = {k: (v[:1] if v.dim() == 3 else v) for k, v in o["gr"].items()}
        f0 = scan(ops, g0, Rp, segmented=True, policy_S=2)
        assert f0.seg_bytes == G * E * 17 * 4
        assert torch.equal(f0.y, o["fwd"].y[:1])
        r0 = scan(ops, g1, Rp, z=o["z"][:1], y_prior=f0.y, reverse=True, accumulate=2, segmented=True, policy_S=2)
        assert torch.equal(r0.y, o["once"].y[:1])


# ---- pair walks -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("gate_each", [0, 1])
@pytest.mark.parametrize("shape", R.PAIR_SHAPES, ids=lambda s: "S%d-L%d-E%d" % s)
@pytest.mark.parametrize("bf,Rp", VARIANTS, ids=VID)
def test_scan_pair(ops, bf, Rp, shape, gate_each):
    S, L, E = shape
    case, yf, yr = R.walks_for(S, L, E, Rp, bf)
    rnd = R.bf16 if bf else R.ident
    gf, gr = gpu_dir(case["fwd"], Rp, bf), gpu_dir(case["rev"], Rp, bf)
    z = case["z"].to(tdtype(bf)).to(DEV)
    mode = "gate_each" if gate_each else "gate_once"
    ref = R.combine(yf, yr, case["z"], mode, rnd, pair=True)
    two = ops.selective_scan_pair(gf, gr, z, Rp, gate_each=gate_each, phases=(1, 2))      # as the engine issues them
    one = ops.selective_scan_pair(gf, gr, z, Rp, gate_each=gate_each, phases=(3,))
    name = f"pair {VID[VARIANTS.index((bf, Rp))]} S={S} L={L} {mode}"
    check(name, two.y, ref, R.scan_bar(S, L, E, Rp, bf, mode), seam=L // 2)               # worst() also: every row written
    assert torch.equal(one.y, two.y)
    if gate_each:        # "the same two rounded addends" as two plain accumulate 1 launches
        f = scan(ops, gf, Rp, z=z)
        r = scan(ops, gr, Rp, z=z, y_prior=f.y, reverse=True, accumulate=1)
        assert torch.equal(two.y, r.y)


# ---- shortened walks ("last_layer_shortcut") ----------------------------------------------------------------------------------------
def same_bits(a, b):
    it = torch.int16 if a.dtype == torch.bfloat16 else torch.int32
    return torch.equal(a.contiguous().view(it), b.contiguous().view(it))


@pytest.mark.parametrize("w", [8, 24, 32, 40, 56])
@pytest.mark.parametrize("bf,Rp", [(True, 64), (False, 64)], ids=["bf16", "fp32"])
def test_scan_walk_len(ops, bf, Rp, w):
    S, L, E = 2, 64, 128
    o = both_directions(ops, S, L, E, Rp, bf)
    prior = torch.randn(S, L, E, generator=torch.Generator().manual_seed(w)).to(tdtype(bf)).to(DEV)
    f = scan(ops, o["gf"], Rp, y_prior=prior, walk_len=w)
    assert same_bits(f.y[:, :w], o["fwd"].y[:, :w]) and same_bits(f.y[:, w:], prior[:, w:])
    # the reverse gating launch adds to what y held: hand it the full forward output, so the walked rows must equal the full walk's
    r = scan(ops, o["gr"], Rp, z=o["z"], y_prior=o["fwd"].y, reverse=True, accumulate=2, walk_len=w)
    assert same_bits(r.y[:, L - w:], o["once"].y[:, L - w:]) and same_bits(r.y[:, :L - w], o["fwd"].y[:, :L - w])
    with pytest.raises(RuntimeError, match=r"\(-1\)"):
        scan(ops, o["gf"], Rp, walk_len=w + 4)                 # not a whole 8-step group


@pytest.mark.parametrize("bf", [True, False], ids=["bf16", "fp32"])
def test_scan_walk_len_is_ignored_when_segmented(ops, bf):
    S, L, E, Rp = 2, 256, 128, 64
    case, _, _ = R.walks_for(S, L, E, Rp, bf)
    gf = gpu_dir(case["fwd"], Rp, bf)
    a, b = scan(ops, gf, Rp, segmented=True), scan(ops, gf, Rp, segmented=True, walk_len=64)
    assert not torch.isnan(b.y).any() and same_bits(a.y, b.y)


# ---- fp32 model under "f32_gemm_split": split dt_proj, split output ------------------------------------------------------------------
@pytest.mark.parametrize("Rp", [64, 96])
def test_scan_dt_split(ops, Rp):
    """dt_low and Wdt as [hi | lo]: three bf16 products per fp32 product; the reference is computed from the unsplit fp32 operands"""
    S, L, E = 2, 64, 128
    o = both_directions(ops, S, L, E, Rp, False, dt_split=True)
    for k in OUTS:
        check(f"dt_split Rp={Rp} plain L={L} {k}", o[k].y, o["refs"][k], o["bars"][k])
    S, L = 1, 128
    case, yf, yr = R.walks_for(S, L, E, Rp, False)
    gf, gr = gpu_dir(case["fwd"], Rp, False, True), gpu_dir(case["rev"], Rp, False, True)
    for ge, mode in ((0, "gate_once"), (1, "gate_each")):
        got = ops.selective_scan_pair(gf, gr, case["z"].to(DEV), Rp, gate_each=ge, phases=(1, 2), dt_split=True)
        check(f"dt_split Rp={Rp} pair L={L} {mode}", got.y, R.combine(yf, yr, case["z"], mode, pair=True), R.scan_bar(S, L, E, Rp, False, mode),
              seam=L // 2)


def check_ysplit(name, res, y_before, plain_y, ref, bar):
    """hi + lo against the reference; (hi, lo) = split_hi_lo of the y the launch writes without ysplit, bit for bit; hi = bf16(hi + lo)
    (scan_ref.hi_rounds_sum: all but exact ties); the plain y buffer keeps the bytes it had (the other direction's output where the
    launch reads it, NaN elsewhere)"""
    assert same_bits(res.y, y_before), "ysplit: the plain y buffer was written"
    hi, lo = res.hi.cpu(), res.lo.cpu()
    check(name, hi.float() + lo.float(), ref, bar)
    assert R.hi_rounds_sum(hi, lo).all()
    whi, wlo = R.split_hi_lo(plain_y.cpu())
    assert same_bits(hi, whi) and same_bits(lo, wlo)


def test_scan_ysplit(ops):
    S, L, E, Rp = 2, 64, 128, 64
    o = both_directions(ops, S, L, E, Rp, False)
    for acc, prior, k in ((2, "fwd", "once"), (1, "fwd_g", "each")):
        res = scan(ops, o["gr"], Rp, z=o["z"], y_prior=o[prior].y, reverse=True, accumulate=acc, ysplit=True)
        check_ysplit(f"ysplit plain accumulate {acc}", res, o[prior].y, o[k].y, o["refs"][k], o["bars"][k])
    S, L = 1, 128
    case, yf, yr = R.walks_for(S, L, E, Rp, False)
    gf, gr = gpu_dir(case["fwd"], Rp, False), gpu_dir(case["rev"], Rp, False)
    z = case["z"].to(DEV)
    for ge, mode in ((0, "gate_once"), (1, "gate_each")):
        plain = ops.selective_scan_pair(gf, gr, z, Rp, gate_each=ge, phases=(1, 2))
        first = ops.selective_scan_pair(gf, gr, z, Rp, gate_each=ge, phases=(1,))          # what phase 1 leaves in y; NaN elsewhere
        res = ops.selective_scan_pair(gf, gr, z, Rp, gate_each=ge, phases=(1, 2), ysplit=True)
        check_ysplit(f"ysplit pair {mode}", res, first.y, plain.y, R.combine(yf, yr, case["z"], mode, pair=True),
                     R.scan_bar(S, L, E, Rp, False, mode))


def test_scan_ysplit_rejects_what_it_cannot_do(ops):
    """PCAD_ERR_INVALID on the host, before any launch"""
    S, E, Rp = 2, 128, 64

    def operands(L, bf):
        case, _, _ = R.walks_for(S, L, E, Rp, bf)
        return gpu_dir(case["fwd"], Rp, bf), gpu_dir(case["rev"], Rp, bf), case["z"].to(tdtype(bf)).to(DEV)
    gf, gr, z = operands(64, False)
    prior = torch.zeros(S, 64, E, device=DEV)
    ok = dict(z=z, y_prior=prior, reverse=True, accumulate=2, ysplit=True)
    scan(ops, gr, Rp, **ok)                                                        # the valid form
    for why, g, kw in (("forward launch", gf, dict(ok, reverse=False)), ("walk_len < L", gr, dict(ok, walk_len=32)),
                       ("no gate", gr, dict(ok, z=None, accumulate=1))):
        with pytest.raises(RuntimeError, match=r"\(-1\)"):
            scan(ops, g, Rp, **kw)
    _, grb, zb = operands(64, True)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):                            # bf16
        scan(ops, grb, Rp, z=zb, y_prior=prior.bfloat16(), reverse=True, accumulate=2, ysplit=True)
    _, grs, zs = operands(256, False)
    with pytest.raises(RuntimeError, match=r"\(-1\)"):                            # segmented
        scan(ops, grs, Rp, z=zs, y_prior=torch.zeros(S, 256, E, device=DEV), reverse=True, accumulate=2, ysplit=True, segmented=True)


# ---- conv + x_proj: K-split grid, split-bf16 x_proj -----------------------------------------------------------------------------------
def conv_case(S, L, E, Rr, bf):
    def make():
        g = torch.Generator().manual_seed(S * 1000 + L + E + Rr)
        x = torch.randn(S, L, E, generator=g)
        wf, wr = (torch.randn(E, 4, generator=g) * 0.5 for _ in range(2))
        b_f, b_r = (torch.randn(E, generator=g) * 0.5 for _ in range(2))
        xpf, xpr = (torch.randn(Rr + 32, E, generator=g) * E ** -0.5 for _ in range(2))
        if bf:
            x, xpf, xpr = (t.bfloat16().float() for t in (x, xpf, xpr))
        return x, wf, b_f, wr, b_r, xpf, xpr
    return R.cached(("conv", S, L, E, Rr, bf), make)


def conv_bars(S, L, E, Rr, bf, c):
    """(conv bar, x_dbl bar): fp32 raised to 8 x the fp32 CPU oracle's worst row against the float64 reference"""
    if bf:
        return R.BAR_CONV[True], R.BAR_XDBL[True]

    def make():
        from oracle import caduceus_oracle as O
        x, wf, b_f, wr, b_r, xpf, xpr = c
        ref = R.conv_xproj(*c)
        of = O.causal_conv1d_fn(x.transpose(1, 2), wf, b_f, activation="silu").transpose(1, 2)
        orv = O.causal_conv1d_fn(x.transpose(1, 2).flip(-1), wr, b_r, activation="silu").flip(-1).transpose(1, 2)
        dc = max(R.row_err(of, ref[0]).max().item(), R.row_err(orv, ref[1]).max().item())
        dx = max(R.row_err(torch.einsum("sle,re->slr", of, xpf), ref[2]).max().item(),
                 R.row_err(torch.einsum("sle,re->slr", orv, xpr), ref[3]).max().item())
        return max(R.BAR_CONV[False], R.ORACLE_FACTOR * dc), max(R.BAR_XDBL[False], R.ORACLE_FACTOR * dx)
    return R.cached(("convbar", S, L, E, Rr), make)


def run_conv(ops, c, bf, **kw):
    dt = tdtype(bf)
    x, wf, b_f, wr, b_r, xpf, xpr = c
    return ops.conv_xproj_bidir_engine(x.to(dt).to(DEV), wf.to(DEV), b_f.to(DEV), wr.to(DEV), b_r.to(DEV), xpf.to(dt).to(DEV), xpr.to(dt).to(DEV), **kw)


def x_dbl(res, d, S, L, split=False):
    """[S, L, R + 32] float64 of direction d: the dt columns (split: hi + lo) and B | C; the padding columns [R, Rp) must be zero"""
    dtl = res.dtl[d].cpu()
    if split:
        hi, lo = dtl[:, :res.Rp], dtl[:, res.Rp:]
        assert R.hi_rounds_sum(hi, lo).all()
        dtl = hi.double() + lo.double()
    assert not torch.isnan(dtl.float()).any() and (dtl[:, res.R:].float() == 0).all()
    return torch.cat([dtl[:, :res.R].double(), res.bc[d].cpu().double()], dim=1).view(S, L, res.R + 32)


@pytest.mark.parametrize("L", R.CONVX_L)
@pytest.mark.parametrize("E,bf,Rp", [(E, bf, 64) for (E, bf) in R.CONVX_KS] + [(256, True, 96), (256, False, 96)],
                         ids=lambda v: str(v))
def test_conv_xproj_ksplit(ops, E, bf, Rp, L):
    S, Rr = 2, R.R_OF[Rp]
    ks = R.CONVX_KS[(E, bf)]
    c = conv_case(S, L, E, Rr, bf)
    rnd = R.bf16 if bf else R.ident
    res = run_conv(ops, c, bf)
    assert res.part_bytes == ks * 2 * S * L * (Rp + 32) * 4       # ks partial x_dbl tensors: the K-split grid ran
    whole = run_conv(ops, c, bf, ksplit=False)                     # the same call without part_ws
    ref = R.conv_xproj(*c, rnd=rnd)
    bar_c, bar_x = conv_bars(S, L, E, Rr, bf, c)
    name = f"conv+x_proj K-split {'bf16' if bf else 'fp32'} E={E} ks={ks} Rp={Rp} L={L}"
    for d in range(2):
        check(f"{name} xc[{d}]", res.xc[d], ref[d], bar_c)
        if bf:
            assert same_bits(res.xc[d], whole.xc[d])               # the conv is not split
            # x_dbl against the product of the kernel's OWN bf16 xc (tests/test_gpu_ops.py test_conv_xproj_fused: isolates the GEMM)
            want = rnd(torch.einsum("sle,re->slr", res.xc[d].double().cpu(), c[5 + d].double()))
        else:
            want = ref[2 + d]
            check(f"{name} x_dbl[{d}] vs unsplit", x_dbl(res, d, S, L), x_dbl(whole, d, S, L), 2 * bar_x)
        check(f"{name} x_dbl[{d}]", x_dbl(res, d, S, L), want, bar_x)
    # policy_S: strand 0 alone under policy_S = 2 runs the S = 2 launch's split, bit for bit
    c0 = (c[0][:1],) + c[1:]
    r0 = run_conv(ops, c0, bf, policy_S=2)
    assert r0.part_bytes == ks * 2 * 1 * L * (Rp + 32) * 4
    for d in range(2):
        assert same_bits(r0.xc[d], res.xc[d][:1]) and same_bits(r0.dtl[d], res.dtl[d][:L]) and same_bits(r0.bc[d], res.bc[d][:L])


@pytest.mark.parametrize("ksplit", [False, True], ids=["alone", "with-K-split"])
@pytest.mark.parametrize("L", [5, 128])
def test_conv_xproj_dtl_split_w_split(ops, L, ksplit):
    """the fp32 model's "f32_gemm_split" form: x_proj as three bf16 products per fp32 product, dt_low written as [hi | lo]"""
    S, E, Rp, Rr = 2, 256, 64, 24
    c = conv_case(S, L, E, Rr, False)
    res = run_conv(ops, c, False, ksplit=ksplit, split=True)
    assert res.part_bytes == 4 * 2 * S * L * (Rp + 32) * 4 and res.dtl[0].dtype == torch.bfloat16
    ref = R.conv_xproj(*c)
    bar_c, _ = conv_bars(S, L, E, Rr, False, c)
    for d in range(2):
        name = f"conv+x_proj dtl_split + w_split {'K-split' if ksplit else 'one block per tile'} L={L}"
        check(f"{name} xc[{d}]", res.xc[d], ref[d], bar_c)
        check(f"{name} x_dbl[{d}]", x_dbl(res, d, S, L, split=True), ref[2 + d], R.BAR_SPLIT)
