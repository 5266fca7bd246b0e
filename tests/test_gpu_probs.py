"""Nucleotide-probability head on the MI355X (csrc/probs.hip): as an operator (pcad_probs_head against
pcad_final_head and float64), inside the forward (pcad_forward_probs / CaduceusForMaskedLM.nucleotide_probs against the live torch
oracle) and under sv_effect."""
import ctypes as C
import math

import numpy as np
import pytest
import torch

from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine, ops
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
from plantcaduceus_amd.ops import to_res_fragment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMP = [0, 1, 2, 6, 5, 4, 3, 7]
COLS = (6, 3, 5, 4)              # a permuted order: a column mix-up shows
ULP = 2.0 ** -23


def rnd(x, dtype):
    return x.to(dtype).float()


def i32(v):
    return (C.c_int32 * len(v))(*[int(x) for x in v])


class HeadInputs:
    """One (B, L, D) problem on the device: h, res (plain or fragment layout), norm weight, embedding."""

    def __init__(self, B, L, D, dtype, res_dtype, frag, scale, g):
        rows = 2 * B * L
        self.B, self.L, self.D, self.dt, self.rdt, self.frag = B, L, D, engine._DT[dtype], engine._DT[res_dtype], frag
        self.h = torch.randn(rows, D, generator=g).to(dtype).to(DEV)
        res = (torch.randn(rows, D, generator=g) * 0.5 + 0.25).to(res_dtype)
        self.res = (to_res_fragment(res) if frag else res).to(DEV).contiguous()
        self.w = (torch.rand(D, generator=g) + 0.5).to(DEV)
        self.emb = rnd(torch.randn(8, D, generator=g) * (scale / math.sqrt(D)), dtype).to(DEV)
        self.comp = torch.tensor(COMP, dtype=torch.int32, device=DEV)
        self.lib = engine.load_library()

    def final(self, positions=None, per_seq=None, h=None, compact=False):
        P = len(positions) if positions is not None else 0
        Q = 1 if per_seq is not None else (P or self.L)
        lg = torch.full((self.B, Q, 8), float("nan"), device=DEV)
        rc = self.lib.pcad_final_head((self.h if h is None else h).data_ptr(), self.res.data_ptr(), self.w.data_ptr(), self.emb.data_ptr(),
                                      self.comp.data_ptr(), None, lg.data_ptr(), self.B, self.L, self.D, C.c_float(1e-5),
                                      i32(positions) if P else None, P, per_seq.data_ptr() if per_seq is not None else None,
                                      int(compact), None, None, self.dt, self.rdt, int(self.frag), engine._stream_ptr())
        assert rc == 0, self.lib.pcad_last_error()
        torch.cuda.synchronize()
        return lg.cpu()

    def probs(self, positions=None, ppw=None, cols=COLS, h=None, compact=False, want_logits=True, ids=None, status=None):
        P = ppw.shape[1] if ppw is not None else (len(positions) if positions is not None else 0)
        Q = P or self.L
        pr = torch.full((self.B, Q, 4), float("nan"), device=DEV)
        lg = torch.full((self.B, Q, 8), float("nan"), device=DEV) if want_logits else None
        rc = self.lib.pcad_probs_head((self.h if h is None else h).data_ptr(), self.res.data_ptr(), self.w.data_ptr(), self.emb.data_ptr(),
                                      self.comp.data_ptr(), i32(cols), pr.data_ptr(), lg.data_ptr() if lg is not None else None,
                                      self.B, self.L, self.D, C.c_float(1e-5), i32(positions) if positions is not None else None, P,
                                      ppw.data_ptr() if ppw is not None else None, int(compact),
                                      ids.data_ptr() if ids is not None else None, status.data_ptr() if status is not None else None,
                                      self.dt, self.rdt, int(self.frag), engine._stream_ptr())
        assert rc == 0, self.lib.pcad_last_error()
        torch.cuda.synchronize()
        return pr.cpu(), (lg.cpu() if lg is not None else None)


def softmax_check(pr, lg, cols, case):
    """check 2: |probs - float64 softmax of the kernel's own logits| <= max(4 x torch's float32 error on them, 2^-23); rows sum to 1
    within 4 * 2^-24.  -> (error, torch's float32 error, largest top margin among the four columns)"""
    x = lg[..., list(cols)]
    want = torch.softmax(x.double(), dim=-1)
    t32 = (torch.softmax(x.float(), dim=-1).double() - want).abs().max().item()
    err = (pr.double() - want).abs().max().item()
    bar = max(4 * t32, ULP)
    top = torch.sort(x, dim=-1).values
    margin = (top[..., 3] - top[..., 2]).max().item()
    rowsum = (pr.double().sum(-1) - 1).abs().max().item()
    print(f"probs head {case}: max |p - f64| {err:.3e}, torch fp32 {t32:.3e}, bar {bar:.3e}, |sum - 1| {rowsum:.3e}, top margin {margin:.1f}")
    assert err <= bar, case
    assert rowsum <= 4 * 2.0 ** -24, case
    return err, t32, margin


def positions_for(L, P, g):
    """P distinct positions including 0 and L - 1 (the reverse-complement strand's rows L - 1 and 0), unsorted"""
    if P == 1:
        return [L - 1]
    mid = (torch.randperm(L - 2, generator=g)[: P - 2] + 1).tolist()
    return [L - 1] + mid + [0]


# ---- 1 + 2: the head alone ---------------------------------------------------------------------------------------------------
# D: 64 (nchunk 8: most lanes idle), 384 (no multiple of 256), 1024, 2048 (the largest head_row's MAXC = 4 instantiation takes)
SHAPES = [(D, L, B) for D in (64, 384, 1024, 2048) for L in (24, 65, 128) for B in (1, 3)]


@pytest.mark.parametrize("dtype,res_dtype", [(torch.float32, torch.float32), (torch.bfloat16, torch.float32),
                                             (torch.bfloat16, torch.bfloat16)])
def test_probs_head_operator(dtype, res_dtype):
    """pcad_probs_head's logits are pcad_final_head's, bit for bit, in all three position forms (and with h_compact); form 2 = rows of
    form 1; form 3 with one list for every window = form 2; the probabilities pass the softmax check on those logits; the
    probabilities do not depend on whether the logits are also written.  Logit scale alternates between a few units and ~100, so
    that rows whose top margin exceeds 80 occur (the max subtraction)."""
    g = torch.Generator().manual_seed(17)
    worst, worst_t32, margin = 0.0, 0.0, 0.0
    for n, (D, L, B) in enumerate(SHAPES):
        x = HeadInputs(B, L, D, dtype, res_dtype, False, (3.0, 60.0)[n % 2], g)
        case = (str(dtype), str(res_dtype), D, L, B)
        # form 1: all positions
        ref1 = x.final()
        p1, l1 = x.probs()
        assert torch.equal(l1, ref1), case
        e, t, m = softmax_check(p1, l1, COLS, case + ("all",))
        worst, worst_t32, margin = max(worst, e), max(worst_t32, t), max(margin, m)
        assert torch.equal(x.probs(want_logits=False)[0], p1), case
        for P in (1, 16):
            pos = positions_for(L, P, g)
            # form 2: a shared host list
            p2, l2 = x.probs(positions=pos)
            assert torch.equal(l2, x.final(positions=pos)), case + (P,)
            assert torch.equal(l2, l1[:, pos]) and torch.equal(p2, p1[:, pos]), case + (P,)
            # ... and on the gathered rows of h (the last-layer shortcut's input)
            hc = ops.gather_rows(x.h, B, L, pos)
            p2c, l2c = x.probs(positions=pos, h=hc, compact=True)
            assert torch.equal(l2c, l2) and torch.equal(p2c, p2), case + (P, "compact")
            # form 3: every window the same list = form 2
            same = torch.tensor([pos] * B, dtype=torch.int32, device=DEV)
            p3, l3 = x.probs(ppw=same)
            assert torch.equal(l3, l2) and torch.equal(p3, p2), case + (P, "per-window, same list")
            # form 3: every window its own list, 0 and L - 1 included
            own = torch.stack([torch.tensor(positions_for(L, P, g)) for _ in range(B)]).to(torch.int32)
            p3, l3 = x.probs(ppw=own.to(DEV))
            idx = own.long()[:, :, None]
            assert torch.equal(l3, torch.gather(l1, 1, idx.expand(-1, -1, 8))), case + (P, "per-window")
            assert torch.equal(p3, torch.gather(p1, 1, idx.expand(-1, -1, 4))), case + (P, "per-window")
            if P == 1:
                assert torch.equal(l3, x.final(per_seq=own[:, 0].contiguous().to(DEV))), case + ("pos_per_seq",)
        # another column order: the same logits, the probabilities permuted
        pn, _ = x.probs(cols=(3, 4, 5, 6))
        inv = [(3, 4, 5, 6).index(c) for c in COLS]
        # the sum is formed in another order: <= 3 roundings of 2^-24 (relative) each way and one division rounding each, 7 * 2^-24
        assert (pn[..., inv] - p1).abs().max().item() <= 4 * ULP, case
    print(f"probs head {dtype} / res {res_dtype}: worst |p - f64| {worst:.3e} (torch fp32 {worst_t32:.3e}), largest top margin {margin:.1f}")
    assert margin > 80, "no row exercised the max subtraction"


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_probs_head_fragment_layout(dtype):
    """fp32 residual in the norm-folded GEMM's fragment layout (B = 1, L = 128, D = 256): the plain-row results, bit for bit, and
    pcad_final_head's logits on the same layout."""
    g = torch.Generator().manual_seed(3)
    B, L, D = 1, 128, 256
    plain = HeadInputs(B, L, D, dtype, torch.float32, False, 60.0, g)
    frag = HeadInputs(B, L, D, dtype, torch.float32, False, 60.0, g)
    frag.h, frag.w, frag.emb = plain.h, plain.w, plain.emb
    frag.res, frag.frag = to_res_fragment(plain.res.cpu()).to(DEV).contiguous(), True
    own = torch.tensor([positions_for(L, 16, g)], dtype=torch.int32, device=DEV)
    for kw in ({}, {"positions": positions_for(L, 16, g)}, {"ppw": own}):
        pp, lp = plain.probs(**kw)
        pf, lf = frag.probs(**kw)
        assert torch.equal(lf, lp) and torch.equal(pf, pp), (str(dtype), list(kw))
    assert torch.equal(frag.probs()[1], frag.final())
    softmax_check(*frag.probs(), COLS, (str(dtype), "fragment"))


def test_probs_head_validation():
    """Per-window positions L and -1: PCAD_STATUS_BAD_POSITION, the row of the clamped position, the other windows untouched.  The
    token-id check of final_head_kernel is kept.  Bad cols: PCAD_ERR_INVALID, nothing launched (outputs untouched)."""
    g = torch.Generator().manual_seed(5)
    B, L, D = 3, 65, 64
    x = HeadInputs(B, L, D, torch.float32, torch.float32, False, 3.0, g)
    ids = torch.full((B, L), 3, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    good = torch.tensor([[4, 9], [L - 1, 0], [7, 30]], dtype=torch.int32)
    bad = good.clone()
    bad[1, 0], bad[1, 1] = L, -1
    pg, lg_ = x.probs(ppw=good.to(DEV), ids=ids, status=status)
    assert int(status.item()) == 0
    pb, lb = x.probs(ppw=bad.to(DEV), ids=ids, status=status)
    assert int(status.item()) == engine.STATUS_BAD_POSITION
    assert torch.equal(pb, pg) and torch.equal(lb, lg_)          # L -> L - 1, -1 -> 0: the clamped rows; windows 0 and 2 unaffected
    status.zero_()
    ids[2, 64] = 9
    x.probs(ppw=good.to(DEV), ids=ids, status=status)
    assert int(status.item()) == engine.STATUS_BAD_TOKEN
    out = torch.full((B, L, 4), 7.0, device=DEV)
    rc = x.lib.pcad_probs_head(x.h.data_ptr(), x.res.data_ptr(), x.w.data_ptr(), x.emb.data_ptr(), x.comp.data_ptr(), i32((3, 4, 5, 8)),
                               out.data_ptr(), None, B, L, D, C.c_float(1e-5), None, 0, None, 0, None, None, x.dt, x.rdt, 0,
                               engine._stream_ptr())
    torch.cuda.synchronize()
    assert rc == -1 and (out == 7.0).all()                       # PCAD_ERR_INVALID


# ---- 3: the forward against the oracle ---------------------------------------------------------------------------------------
def mlm(cfg, sd, dtype, **options):
    cfg.engine_options = dict(options)
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dtype).to(DEV).eval()


def rand_ids(B, L, seed):
    return torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("mode", ["fp32", "fp32_split", "bf16"])
def test_model_probs_vs_oracle(mode):
    """nucleotide_probs in the three position forms against softmax (float64) of the live oracle's logits.  A softmax does not
    amplify, |dp|inf <= |dlogit|inf, so the bar is tests/test_gpu_model.py's logit bar as an absolute number: tol max|oracle logit|,
    tol = 1e-4 (fp32, fp32 + f32_gemm_split) / 3e-2 (bf16 against the bf16-emulating oracle), and never above 1.  The logits
    handed back are the plain forward's: form 1 = forward(ids), form 2 = forward(ids, positions=list) (last-layer shortcut), form 3
    with P = 1 = pcad_forward_at."""
    bf16 = mode == "bf16"
    dtype = torch.bfloat16 if bf16 else torch.float32
    tol = 3e-2 if bf16 else 1e-4
    g = torch.Generator().manual_seed(13)
    for L, B in ((45, 3), (128, 2)):
        cfg = make_config("tiny", d_model=128, n_layer=2)
        sd = synthetic_state_dict(cfg, seed=11)
        ids = rand_ids(B, L, L)
        if bf16:
            ref = O.forward_strands(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16)["logits"]
        else:
            ref = O.forward_strands(ids, O.params_from_state_dict(sd, cfg))["logits"]
        ref = torch.as_tensor(ref).float()
        bar = min(tol * ref.abs().max().item(), 1.0)
        want = torch.softmax(ref[..., list(COLS)].double(), dim=-1)
        m = mlm(make_config("tiny", d_model=128, n_layer=2), sd, dtype, **({"f32_gemm_split": 1} if mode == "fp32_split" else {}))
        eng = m._engine()
        d = ids.to(DEV)
        p1, l1 = m.nucleotide_probs(d, COLS, return_logits=True)
        assert p1.shape == (B, L, 4) and p1.dtype == torch.float32 and l1.shape == (B, L, 8)
        assert torch.equal(l1.cpu(), m(input_ids=d).logits.cpu())
        pos = positions_for(L, 16, g)
        p2, l2 = m.nucleotide_probs(d, COLS, positions=pos, return_logits=True)
        assert torch.equal(l2.cpu(), m(input_ids=d, positions=pos).logits.cpu())
        own = torch.stack([torch.tensor(positions_for(L, 16, g)) for _ in range(B)])
        p3 = m.nucleotide_probs(d, COLS, positions_per_window=own.to(DEV))
        one = own[:, :1].contiguous()
        p4, l4 = m.nucleotide_probs(d, COLS, positions_per_window=one.to(DEV), return_logits=True)
        assert torch.equal(l4.cpu(), eng.forward(d, positions=one[:, 0].to(DEV))[0].cpu())          # pcad_forward_at
        # the full last layer (forms 1 and 3) gives one set of rows
        idx = own.long()[:, :, None].expand(-1, -1, 4)
        assert torch.equal(p3.cpu(), torch.gather(p1.cpu(), 1, idx))
        assert torch.equal(p4.cpu(), torch.gather(p1.cpu(), 1, one.long()[:, :, None].expand(-1, -1, 4)))
        errs = dict(all=(p1.cpu().double() - want).abs().max().item(),
                    shared=(p2.cpu().double() - want[:, pos]).abs().max().item(),
                    per_window=(p3.cpu().double() - torch.gather(want, 1, idx)).abs().max().item())
        print(f"{mode} L={L}: |dp| {errs}, bar {bar:.3e} (max |logit| {ref.abs().max().item():.2f})")
        assert max(errs.values()) <= bar, (mode, L, errs)
        m.check_status()
        del m


# ---- 4: batch and chunk independence -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_and_chunk_independence(dtype):
    """"scan_segments" 0: a window's probabilities (all positions, and ten positions of its own) are bit-identical alone, at batch 37,
    under "chunk_seqs" 5 and with "poison_workspace" 1."""
    cfg = make_config("tiny", d_model=128, n_layer=2)
    m = mlm(cfg, synthetic_state_dict(cfg, seed=6), dtype, scan_segments=0)
    eng = m._engine()
    B, L = 37, 200
    ids = rand_ids(B, L, 2).to(DEV)
    own = torch.stack([torch.randperm(L, generator=torch.Generator().manual_seed(b))[:10] for b in range(B)]).to(DEV)

    def run(sl=slice(None)):
        return eng.forward_probs(ids[sl], COLS).cpu(), eng.forward_probs(ids[sl], COLS, positions_per_window=own[sl]).cpu()

    alone = run(slice(5, 6))
    batch = run()
    eng.set_option("chunk_seqs", 5)
    chunked = run()
    eng.set_option("poison_workspace", 1)
    poisoned = run()
    eng.set_option("poison_workspace", 0)
    eng.set_option("chunk_seqs", 0)
    for k in range(2):
        assert torch.equal(alone[k][0], batch[k][5])
        assert torch.equal(chunked[k], batch[k]) and torch.equal(poisoned[k], batch[k])
        assert torch.isfinite(poisoned[k]).all()
    assert torch.equal(batch[1], torch.gather(batch[0], 1, own.cpu()[:, :, None].expand(-1, -1, 4)))
    m.check_status()


# ---- 5: validation through the model -----------------------------------------------------------------------------------------
def test_model_validation():
    cfg = make_config("tiny", d_model=128, n_layer=1)
    m = mlm(cfg, synthetic_state_dict(cfg, seed=8), torch.float32)
    B, L = 3, 65
    ids = rand_ids(B, L, 9).to(DEV)
    good = torch.tensor([[4, 9], [L - 1, 0], [7, 30]])
    bad = good.clone()
    bad[1, 0], bad[1, 1] = L, -1
    pg = m.nucleotide_probs(ids, COLS, positions_per_window=good.to(DEV)).cpu()
    m.check_status()
    pb = m.nucleotide_probs(ids, COLS, positions_per_window=bad.to(DEV)).cpu()
    assert m.status_bits() == engine.STATUS_BAD_POSITION
    with pytest.raises(IndexError, match="position"):
        m.check_status()
    assert torch.equal(pb, pg)
    with pytest.raises(RuntimeError, match="cols"):
        m.nucleotide_probs(ids, (3, 4, 5, 8))
    with pytest.raises(ValueError):
        m.nucleotide_probs(ids, COLS, positions=[1], positions_per_window=good.to(DEV))
    with pytest.raises(ValueError):
        m.nucleotide_probs(ids, COLS, positions_per_window=torch.zeros(B, 17, dtype=torch.long, device=DEV))
    m.check_status()


# ---- 6: workspace ------------------------------------------------------------------------------------------------------------
def test_workspace_bytes_unchanged_on_device():
    from test_mlm_eval import WORKSPACE_BYTES, _handle
    lib = engine.load_library()
    for (D, dt, split, B, L), want in WORKSPACE_BYTES.items():
        h = _handle(lib, D, dt, split)
        got = lib.pcad_workspace_bytes(h, B, L)
        lib.pcad_destroy(h)
        assert got == want, (D, dt, split, B, L, got)


# ---- 7: sv_effect on the engine ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_sv_effect_sparse_equals_dense_on_the_engine(dtype, tmp_path):
    """6 synthetic SVs of 512-bp windows, PlantCAD2 Small's width, 2 layers: sv_effect's sparse path (boundary_probs: ten rows per
    window) against the dense one (unmasked_probs + sv_llr_boundary).  Rows within 2^-23 (the floor of check 2's bar; both come from
    the same head on the same full last layer), scores within what that allows - |d log p| <= dp / p at every read position - and
    identical AUROC / AUPRC."""
    import pandas as pd
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    cfg = make_config("tiny", d_model=768, n_layer=2)
    m = mlm(cfg, synthetic_state_dict(cfg, seed=5), dtype)
    tok = CaduceusTokenizer()
    rng = np.random.default_rng(4)
    n, L, F = 6, 512, 5
    mk = lambda: "".join(rng.choice(list("ACGTN"), size=L, p=[.24, .24, .24, .24, .04]))
    left, right = rng.integers(F + 1, 200, size=n), rng.integers(300, L - F, size=n)
    left[0], right[0] = F + 1, L - F                             # rows 0 and L - 1
    df = pd.DataFrame({"RefSeq": [mk() for _ in range(n)], "MutSeq": [mk() for _ in range(n)], "left": left, "right": right,
                       "label": [0, 1, 0, 1, 1, 0]})
    out = tmp_path / "sv.tsv"
    res = pe.sv_effect(df, m, tok, DEV, batch_size=4, flanking=F, output=str(out))
    got = pd.read_csv(out, sep="\t")["score"].to_numpy().astype(np.float32)       # the float32 scores' shortest decimal form reads back exactly
    ref_p = pe.unmasked_probs(df["RefSeq"], tok, m, DEV, 4)
    mut_p = pe.unmasked_probs(df["MutSeq"], tok, m, DEV, 4)
    dense = pe.sv_llr_boundary(df["left"], df["right"], df["MutSeq"], ref_p, mut_p, F)
    ref_pos, mut_pos = pe._sv_positions(df["left"], df["right"], L, F)
    rows = np.arange(n)[:, None]
    r_rows = pe.boundary_probs(df["RefSeq"], ref_pos, tok, m, DEV, 4)
    m_rows = pe.boundary_probs(df["MutSeq"], np.broadcast_to(mut_pos, (n, 2 * F)), tok, m, DEV, 4)
    dr = np.abs(r_rows - ref_p[rows, ref_pos]).max()
    dm = np.abs(m_rows - mut_p[rows, mut_pos[None, :]]).max()
    allow = (ULP / np.maximum(ref_p[rows, ref_pos], 1e-12).min(-1) + ULP / np.maximum(mut_p[rows, mut_pos[None, :]], 1e-12).min(-1)).mean(1)
    print(f"sv_effect {dtype}: rows |dp| ref {dr:.3e} mut {dm:.3e}; scores |d| {np.abs(got - dense).max():.3e}, allowed {allow.max():.3e}")
    assert dr <= ULP and dm <= ULP
    assert (np.abs(got - dense) <= allow).all()
    assert res["AUPRC"] == pe.average_precision(df["label"], dense)
    assert pe.auroc(df["label"], got) == pe.auroc(df["label"], dense)
    m.check_status()
