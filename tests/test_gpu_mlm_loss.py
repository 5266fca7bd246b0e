"""Masked-LM loss on the MI355X: the fused loss head (csrc/loss.hip) as an operator, inside the forward (pcad_forward_loss /
CaduceusForMaskedLM with labels) and the mlm_eval command.  The float64 restatement of the loss is tests/mlm_ref.py."""
import ctypes as C
import json
import math
import os

import numpy as np
import pytest
import torch
from torch.nn import functional as F

import mlm_ref
from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
from plantcaduceus_amd.ops import to_res_fragment

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
COMP = [0, 1, 2, 6, 5, 4, 3, 7]


def rnd(x, dtype):
    return x.to(dtype).float()


def rand_labels(B, L, frac, g):
    """labels in 0..7 on about `frac` of the positions, -100 elsewhere"""
    lab = torch.randint(0, 8, (B, L), generator=g)
    keep = torch.rand(B, L, generator=g) < frac
    return torch.where(keep, lab, torch.full_like(lab, -100)).to(torch.int32)


def rand_weights(B, L, g):
    return torch.tensor([0.0, 0.1, 1.0])[torch.randint(0, 3, (B, L), generator=g)]


def run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, dt, frag, ignore_index=-100, want_logits=True, status=None,
                  ids=None, res_dt=engine.PCAD_F32):
    comp = torch.tensor(COMP, dtype=torch.int32, device=DEV)
    res_dev = (to_res_fragment(res) if frag else res).to(DEV).contiguous()
    hd, wd, ed = h.to(DEV), w.to(DEV), emb.to(DEV)
    lab = labels.to(DEV).contiguous()
    wt = weights.to(DEV).float().contiguous() if weights is not None else None
    sums = torch.full((B, 4), float("nan"), device=DEV)
    nll = torch.full((B, L), float("nan"), device=DEV)
    lg = torch.full((B, L, 8), float("nan"), device=DEV) if want_logits else None
    nb = lib.pcad_loss_head_scratch_bytes(B, L)
    scratch = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    sp = (scratch.data_ptr() + 255) // 256 * 256
    rc = lib.pcad_loss_head(hd.data_ptr(), res_dev.data_ptr(), wd.data_ptr(), ed.data_ptr(), comp.data_ptr(), lab.data_ptr(),
                            wt.data_ptr() if wt is not None else None, ignore_index, sums.data_ptr(), nll.data_ptr(),
                            lg.data_ptr() if lg is not None else None, B, L, D, C.c_float(1e-5),
                            ids.data_ptr() if ids is not None else None, status.data_ptr() if status is not None else None,
                            dt, res_dt, int(frag), sp, nb, engine._stream_ptr())
    assert rc == 0, lib.pcad_last_error()
    torch.cuda.synchronize()
    return sums.cpu(), nll.cpu(), (lg.cpu() if lg is not None else None)


def run_final_head(lib, h, res, w, emb, B, L, D, dt, frag):
    comp = torch.tensor(COMP, dtype=torch.int32, device=DEV)
    res_dev = (to_res_fragment(res) if frag else res).to(DEV).contiguous()
    hd, wd, ed = h.to(DEV), w.to(DEV), emb.to(DEV)
    lg = torch.empty(B, L, 8, device=DEV)
    rc = lib.pcad_final_head(hd.data_ptr(), res_dev.data_ptr(), wd.data_ptr(), ed.data_ptr(), comp.data_ptr(), None, lg.data_ptr(),
                             B, L, D, C.c_float(1e-5), None, 0, None, 0, None, None, dt, engine.PCAD_F32, int(frag),
                             engine._stream_ptr())
    assert rc == 0, lib.pcad_last_error()
    torch.cuda.synchronize()
    return lg.cpu()


# ---- 1 + 2: the head alone -----------------------------------------------------------------------------------------------
# (D, L, fragment layout, B): B chosen so that 2 B L is a multiple of 256 where the fragment layout is used (which also needs D % 256 == 0)
HEAD_CASES = [(D, L, frag, B) for D in (384, 512, 768, 1024, 1536)
              for L, frag, B in ((24, False, 3), (512, False, 2), (600, False, 2), (24, True, 16), (512, True, 2), (600, True, 16))
              if not (frag and D % 256)]


@pytest.mark.parametrize("dtype", [torch.bfloat16, torch.float32])
def test_loss_head_operator(dtype):
    """pcad_loss_head against mlm_ref (float64) on pcad_final_head's logits of the same inputs.  The logits are the same numbers
    (asserted bit-equal), so the difference is exp / log alone: the bar is 4x the error of torch's own float32
    F.cross_entropy(reduction="none") against the float64 value on those logits.  Counts exact.  Window sums: within
    L 2^-24 sum|w nll| of the float64 sum of the kernel's own nll x w (fp32 summation in a fixed order)."""
    lib = engine.load_library()
    g = torch.Generator().manual_seed(7)
    dt = engine._DT[dtype]
    worst = 0.0
    for D, L, frag, B in HEAD_CASES:
        rows = 2 * B * L
        h = torch.randn(rows, D, generator=g).to(dtype)
        res = torch.randn(rows, D, generator=g) * 0.5 + 0.25
        w = torch.rand(D, generator=g) + 0.5
        emb = rnd(torch.randn(8, D, generator=g) * (3.0 / math.sqrt(D)), dtype)      # logits of a few units
        labels = rand_labels(B, L, 0.5, g)
        weights = rand_weights(B, L, g)
        ref_lg = run_final_head(lib, h, res, w, emb, B, L, D, dt, frag)
        sums, nll, lg = run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, dt, frag)
        case = (str(dtype), D, L, frag)
        assert torch.equal(lg, ref_lg), case
        want = mlm_ref.token_nll(ref_lg, labels)
        m = mlm_ref.labelled_mask(labels)
        t32 = F.cross_entropy(ref_lg.view(-1, 8), labels.view(-1).long(), reduction="none", ignore_index=-100).view(B, L)
        bar = 4 * (t32.double() - want).abs().max().item()
        err = (nll.double() - want).abs().max().item()
        worst = max(worst, err)
        print(f"loss head {case}: max |nll - f64| {err:.3e}, torch fp32 {bar / 4:.3e}, bar {bar:.3e}")
        assert err <= bar, case
        assert (nll[~m] == 0).all(), case
        wsum = mlm_ref.window_sums(ref_lg, labels, weights)
        assert torch.equal(sums[:, 2:].double(), wsum[:, 2:]), case                  # labelled, arg-max hits: exact
        # sums without logits_out (only labelled rows are read): the same bits
        sums2, nll2, _ = run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, dt, frag, want_logits=False)
        assert torch.equal(sums2, sums) and torch.equal(nll2, nll), case
        wm = torch.where(m, weights.double(), torch.zeros(B, L, dtype=torch.float64))
        prod = wm * nll.double()
        assert ((sums[:, 0].double() - prod.sum(1)).abs() <= L * 2.0 ** -24 * prod.abs().sum(1)).all(), case
        assert ((sums[:, 1].double() - wm.sum(1)).abs() <= L * 2.0 ** -24 * wm.abs().sum(1)).all(), case
        # no weights: w = 1
        sums3, _, _ = run_loss_head(lib, h, res, w, emb, labels, None, B, L, D, dt, frag, want_logits=False)
        assert torch.equal(sums3[:, 1], sums3[:, 2]), case
        assert ((sums3[:, 0].double() - nll.double().sum(1)).abs() <= L * 2.0 ** -24 * nll.double().abs().sum(1)).all(), case
    print(f"loss head {dtype}: worst |nll - f64| {worst:.3e}")


@pytest.mark.parametrize("D", [384, 1024, 1536])
def test_loss_head_bf16_residual(D):
    """The <bf16, bf16> pair (a bf16 model with residual_in_fp32 = False) at each width class: bf16 h and a bf16 residual against the
    same call with that residual widened to fp32.  The head only reads the residual and adds it to h in fp32 (csrc/head_row.hpp), and
    a bf16 value is exact in fp32, so sums, nll and logits are bit-equal; the outputs start as NaN, so an unwritten row shows."""
    lib = engine.load_library()
    g = torch.Generator().manual_seed(D)
    B, L = 3, 24
    h = torch.randn(2 * B * L, D, generator=g).to(torch.bfloat16)
    res = (torch.randn(2 * B * L, D, generator=g) * 0.5 + 0.25).to(torch.bfloat16)
    w = torch.rand(D, generator=g) + 0.5
    emb = rnd(torch.randn(8, D, generator=g) * (3.0 / math.sqrt(D)), torch.bfloat16)
    labels = rand_labels(B, L, 0.5, g)
    weights = rand_weights(B, L, g)
    got = run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, engine.PCAD_BF16, False, res_dt=engine.PCAD_BF16)
    want = run_loss_head(lib, h, res.float(), w, emb, labels, weights, B, L, D, engine.PCAD_BF16, False)
    for name, a, b in zip(("sums", "nll", "logits"), got, want):
        assert not torch.isnan(b).any(), name
        assert torch.equal(a, b), name


def test_loss_head_label_semantics():
    """-100, any negative label and a custom ignore_index are skipped; a label of 9 sets PCAD_STATUS_BAD_LABEL and is skipped; the
    token-id check is kept; weights at ignored positions do not count."""
    lib = engine.load_library()
    g = torch.Generator().manual_seed(1)
    B, L, D = 2, 70, 64
    h = torch.randn(2 * B * L, D, generator=g)
    res = torch.randn(2 * B * L, D, generator=g)
    w = torch.ones(D)
    emb = torch.randn(8, D, generator=g) * 0.3
    labels = torch.randint(0, 8, (B, L), generator=g).to(torch.int32)
    labels[0, 3], labels[0, 4], labels[1, 69], labels[1, 0] = -100, -7, 5, 9
    weights = torch.full((B, L), 0.5)
    weights[0, 3] = 1e6
    ids = torch.full((B, L), 3, dtype=torch.int32, device=DEV)
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    sums, nll, lg = run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, 0, False, ignore_index=5, status=status, ids=ids)
    assert int(status.item()) == engine.STATUS_BAD_LABEL
    skipped = (labels == 5) | (labels < 0) | (labels == 9)
    assert skipped[0, 3] and skipped[0, 4] and skipped[1, 69] and skipped[1, 0]
    assert (nll[skipped] == 0).all() and (nll[~skipped] > 0).all()
    lab_ref = torch.where(skipped, torch.full_like(labels, -100), labels)
    want = mlm_ref.window_sums(lg, lab_ref, weights)
    assert torch.equal(sums[:, 2:].double(), want[:, 2:])
    # 70 positive fp32 terms: summation error <= 70 * 2^-24 = 4.2e-6 relative, plus ~1e-7 from exp / log
    torch.testing.assert_close(sums[:, :2].double(), want[:, :2], rtol=1e-5, atol=0)
    ids[1, 7] = 11
    status.zero_()
    labels[1, 0] = 2
    run_loss_head(lib, h, res, w, emb, labels, weights, B, L, D, 0, False, status=status, ids=ids)
    assert int(status.item()) == engine.STATUS_BAD_TOKEN


# ---- 3: model vs oracle --------------------------------------------------------------------------------------------------
def mlm(cfg, sd, dtype, **options):
    cfg.engine_options = dict(options)
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dtype).to(DEV).eval()


def rand_ids(B, L, seed):
    return torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(seed))


@pytest.mark.parametrize("mode", ["fp32", "fp32_split", "bf16"])
def test_model_loss_vs_oracle(mode):
    """model(ids, labels, loss_weights).loss and the token nll against mlm_ref on the CPU oracle's logits.  |d logsumexp| <= max |d logit|,
    so per-token |d nll| <= 2 max |d logit|: the bar is twice the logit tolerance tests/test_gpu_model.py applies to the same
    configuration (relative to the logit range): 2 tol max|oracle logit|, tol = 1e-4 (fp32, fp32 + f32_gemm_split) / 3e-2 (bf16
    against the bf16-emulating oracle).  The batch loss is a convex combination of the nll: the same bar."""
    bf16 = mode == "bf16"
    dtype = torch.bfloat16 if bf16 else torch.float32
    tol = 3e-2 if bf16 else 1e-4
    g = torch.Generator().manual_seed(11)
    for L, B in ((45, 3), (600, 3)):
        cfg = make_config("tiny", d_model=128, n_layer=2)
        sd = synthetic_state_dict(cfg, seed=11)
        ids = rand_ids(B, L, L)
        if bf16:
            ref = O.forward_strands(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16)["logits"]
        else:
            ref = O.forward_strands(ids, O.params_from_state_dict(sd, cfg))["logits"]
        ref = torch.as_tensor(ref).float()
        bar = 2 * tol * ref.abs().max().item()
        m = mlm(make_config("tiny", d_model=128, n_layer=2), sd, dtype, **({"f32_gemm_split": 1} if mode == "fp32_split" else {}))
        labels = rand_labels(B, L, 0.15, g)
        for weights in (None, rand_weights(B, L, g)):
            out = m(input_ids=ids.to(DEV), labels=labels.to(DEV), loss_weights=None if weights is None else weights.to(DEV),
                    return_token_nll=True, return_window_sums=True)
            assert out.logits.shape == (B, L, 8) and out.logits.dtype == torch.float32
            assert torch.equal(out.logits.cpu(), m(input_ids=ids.to(DEV)).logits.cpu())
            nll = out["token_nll"].cpu().double()
            want_nll = mlm_ref.token_nll(ref, labels)
            want = mlm_ref.loss(ref, labels, weights)
            e_tok = (nll - want_nll).abs().max().item()
            e_loss = abs(out.loss.item() - want.item())
            print(f"{mode} L={L} weights={weights is not None}: |d nll| {e_tok:.3e}, |d loss| {e_loss:.3e}, bar {bar:.3e}")
            assert e_tok <= bar and e_loss <= bar, (mode, L)
            ws = mlm_ref.window_sums(out.logits.cpu(), labels, weights)
            assert torch.equal(out["window_sums"].cpu()[:, 2:].double(), ws[:, 2:])
        m.check_status()
        del m


@pytest.mark.parametrize("size", ["l20", "l32"])
def test_full_depth_nll_vs_committed_oracle(size):
    """Full depth: tests/golden/census_<size>.npz holds the oracle's fp32 logits at the masked position 255 of its windows
    (oracle/gen_census_golden.py).  Label position 255 only, with a seeded base id in 3..6: nll[:, 255] against mlm_ref on the fixture
    logits, under twice tests/test_gpu_fulldepth.py's fp32 bar (1e-4 of max |logit|)."""
    import hashlib
    from oracle.gen_census_golden import census_windows
    n = 16
    fx = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", f"census_{size}.npz"))
    ids = census_windows(int(fx["meta"][0]), int(fx["meta"][1]))
    assert hashlib.sha1(ids.tobytes()).digest() == fx["ids_sha1"].tobytes()
    ids = torch.from_numpy(ids[:n].astype(np.int64))
    ref = torch.from_numpy(fx["logits_f32"][:n].astype(np.float32))          # [n, 8] at position 255
    cfg = make_config(size)
    sd = synthetic_state_dict(cfg, seed=1234, stress=False)
    m = mlm(cfg, sd, torch.float32)
    labels = torch.full((n, 512), -100, dtype=torch.int32)
    labels[:, 255] = torch.randint(3, 7, (n,), generator=torch.Generator().manual_seed(3)).to(torch.int32)
    out = m(input_ids=ids.to(DEV), labels=labels.to(DEV), output_logits=False, return_token_nll=True)
    assert out.logits is None
    nll = out["token_nll"].cpu().double()
    want = mlm_ref.token_nll(ref.unsqueeze(1), labels[:, 255:256])[:, 0]
    bar = 2 * 1e-4 * ref.abs().max().item()
    err = (nll[:, 255] - want).abs().max().item()
    print(f"{size} full depth: |d nll| {err:.3e}, bar {bar:.3e}")
    assert err <= bar
    assert (nll[:, :255] == 0).all() and (nll[:, 256:] == 0).all()
    assert abs(out.loss.item() - want.mean().item()) <= bar


# ---- 4: determinism / batch independence ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_batch_and_chunk_independence(dtype):
    """"scan_segments" 0: a window's sums row and nll row are bit-identical alone, at batch 37 and under "chunk_seqs" 5; repeated calls
    are bit-identical; "poison_workspace" 1 leaves the results unchanged and finite."""
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=6)
    m = mlm(cfg, sd, dtype, scan_segments=0)
    eng = m._engine()
    g = torch.Generator().manual_seed(2)
    B, L = 37, 600
    ids = rand_ids(B, L, 2).to(DEV)
    labels = rand_labels(B, L, 0.15, g).to(DEV)
    weights = rand_weights(B, L, g).to(DEV)

    def run(sl=slice(None)):
        s, n, _ = eng.forward_loss(ids[sl], labels[sl], weights[sl], want_nll=True)
        return s.cpu(), n.cpu()

    alone = run(slice(5, 6))
    batch = run()
    again = run()
    eng.set_option("chunk_seqs", 5)
    chunked = run()
    eng.set_option("poison_workspace", 1)
    poisoned = run()
    eng.set_option("poison_workspace", 0)
    eng.set_option("chunk_seqs", 0)
    assert torch.equal(alone[0][0], batch[0][5]) and torch.equal(alone[1][0], batch[1][5])
    for other in (again, chunked, poisoned):
        assert torch.equal(other[0], batch[0]) and torch.equal(other[1], batch[1])
    assert torch.isfinite(poisoned[0]).all() and torch.isfinite(poisoned[1]).all()


# ---- 5: semantics through the model ----------------------------------------------------------------------------------------
def test_model_semantics():
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=8)
    m = mlm(cfg, sd, torch.float32)
    g = torch.Generator().manual_seed(4)
    B, L = 4, 96
    ids = rand_ids(B, L, 9).to(DEV)
    before = m(input_ids=ids)
    lg0, = (before.logits.cpu(),)
    labels = rand_labels(B, L, 0.3, g)
    weights = rand_weights(B, L, g)
    out = m(input_ids=ids, labels=labels.to(DEV), loss_weights=weights.to(DEV), return_window_sums=True)
    lean = m(input_ids=ids, labels=labels.to(DEV), loss_weights=weights.to(DEV), output_logits=False, return_window_sums=True)
    assert lean.logits is None and torch.equal(lean.loss.cpu(), out.loss.cpu())          # the same loss bit for bit
    assert torch.equal(lean["window_sums"].cpu(), out["window_sums"].cpu())
    # pcad_forward's outputs on the same ids are unchanged by a preceding forward_loss call
    assert torch.equal(m(input_ids=ids).logits.cpu(), lg0)
    # negative labels and a custom ignore_index
    lab2 = labels.clone()
    lab2[labels == -100] = -3
    assert torch.equal(m(input_ids=ids, labels=lab2.to(DEV), loss_weights=weights.to(DEV)).loss.cpu(), out.loss.cpu())
    lab3 = labels.clone()
    lab3[labels == -100] = 77
    assert torch.equal(m(input_ids=ids, labels=lab3.to(DEV), loss_weights=weights.to(DEV), ignore_index=77).loss.cpu(), out.loss.cpu())
    m.check_status()
    # weights at ignored positions do not count
    w2 = weights.clone()
    w2[labels == -100] = 1e9
    assert torch.equal(m(input_ids=ids, labels=labels.to(DEV), loss_weights=w2.to(DEV)).loss.cpu(), out.loss.cpu())
    # unweighted: the mean over labelled positions = F.cross_entropy on the model's own logits (to fp32 rounding)
    plain = m(input_ids=ids, labels=labels.to(DEV).long())
    want = mlm_ref.loss(plain.logits.cpu(), labels)
    assert abs(plain.loss.item() - want.item()) <= 1e-5 * abs(want.item())
    # an all-ignored batch: nan loss, sums all 0
    none = m(input_ids=ids, labels=torch.full((B, L), -100, device=DEV), return_window_sums=True)
    assert math.isnan(none.loss.item()) and (none["window_sums"].cpu() == 0).all()
    with pytest.raises(ValueError):
        m(input_ids=ids, labels=labels.to(DEV), positions=[3])
    # a label of 9: reported, skipped
    lab9 = labels.clone()
    lab9[2, 5] = 9
    lab9_ref = labels.clone()
    lab9_ref[2, 5] = -100
    b = m(input_ids=ids, labels=lab9_ref.to(DEV), loss_weights=weights.to(DEV))
    m.check_status()
    a = m(input_ids=ids, labels=lab9.to(DEV), loss_weights=weights.to(DEV))
    assert m.status_bits() == engine.STATUS_BAD_LABEL
    with pytest.raises(IndexError, match="labels"):
        m.check_status()
    assert torch.equal(a.loss.cpu(), b.loss.cpu())


def test_auto_model_both_dtypes(tmp_path):
    from transformers import AutoModelForMaskedLM
    import plantcaduceus_amd
    plantcaduceus_amd.register()
    cfg = make_config("tiny", d_model=128, n_layer=2)
    path = str(tmp_path / "snap")
    save_checkpoint(path, cfg, synthetic_state_dict(cfg, seed=9))
    g = torch.Generator().manual_seed(0)
    ids = rand_ids(2, 64, 1).to(DEV)
    labels = rand_labels(2, 64, 0.15, g).to(DEV)
    w = rand_weights(2, 64, g).to(DEV)
    for dtype in (torch.float32, torch.bfloat16):
        m = AutoModelForMaskedLM.from_pretrained(path, trust_remote_code=True).to(dtype).to(DEV).eval()
        out = m(input_ids=ids, labels=labels, loss_weights=w)
        assert out.loss.dim() == 0 and math.isfinite(out.loss.item()) and out.logits.shape == (2, 64, 8)
        m.check_status()


# ---- 6: workspace ----------------------------------------------------------------------------------------------------------
def test_workspace_bytes_unchanged_on_device():
    from test_mlm_eval import WORKSPACE_BYTES, _handle
    lib = engine.load_library()
    for (D, dt, split, B, L), want in WORKSPACE_BYTES.items():
        h = _handle(lib, D, dt, split)
        got = lib.pcad_workspace_bytes(h, B, L)
        lib.pcad_destroy(h)
        assert got == want, (D, dt, split, B, L, got)


# ---- 7: the command --------------------------------------------------------------------------------------------------------
def test_mlm_eval_command(tmp_path):
    """mlm_eval --do_eval on a 64-window synthetic dataset reproduces eval_loss computed by mlm_ref from model(ids).logits with the
    same masks, within bar 3's tolerance (fp32 + f32_gemm_split: 2e-4 of max |logit|); perplexity == exp(eval_loss)."""
    import pandas as pd
    from transformers import set_seed
    from plantcaduceus_amd import mlm_eval
    cfg = make_config("tiny", d_model=128, n_layer=2)
    snap = str(tmp_path / "snap")
    save_checkpoint(snap, cfg, synthetic_state_dict(cfg, seed=9))
    rng = np.random.default_rng(0)
    seqs = ["".join(rng.choice(list("ACGTacgtN"), size=200)) for _ in range(64)]
    data = tmp_path / "data"
    os.makedirs(data)
    pd.DataFrame({"seq": seqs}).to_parquet(data / "validation.parquet")
    out = str(tmp_path / "out")
    nllf = str(tmp_path / "nll.npy")
    mlm_eval.main(["--model_name_or_path", snap, "--dataset_name", str(data), "--do_eval", "--output_dir", out,
                   "--per_device_eval_batch_size", "7", "--soft_masked_loss_weights_evaluation", "0.1", "--engine_batch_size", "24",
                   "--token-nll-out", nllf])
    res = json.load(open(os.path.join(out, "eval_results.json")))
    assert res["eval_samples"] == 64 and res["perplexity"] == math.exp(res["eval_loss"])
    model, tok = mlm_eval.load_model_and_tokenizer(snap, None, DEV)
    ids, special, w = mlm_eval.tokenize_windows(tok, seqs, 0.1)
    set_seed(42)
    masked, labels = mlm_eval.mask_windows(mlm_eval.make_collator(tok, 0.15), ids, special, 7)
    lg = torch.cat([model(input_ids=torch.from_numpy(masked[i:i + 16]).to(DEV)).logits.cpu() for i in range(0, 64, 16)])
    want = mlm_ref.trainer_eval_loss(lg, torch.from_numpy(labels), torch.from_numpy(w), 7)
    bar = 2 * 1e-4 * lg.abs().max().item()
    print(f"mlm_eval: eval_loss {res['eval_loss']:.6f}, from logits {want:.6f}, bar {bar:.3e}")
    assert abs(res["eval_loss"] - want) <= bar
    nll = np.load(nllf)
    assert nll.shape == (64, 200) and (nll[labels < 0] == 0).all()
    assert np.abs(nll - mlm_ref.token_nll(lg, torch.from_numpy(labels)).numpy()).max() <= bar
    ws = mlm_ref.window_sums(lg, torch.from_numpy(labels), torch.from_numpy(w))
    assert res["eval_token_accuracy"] == pytest.approx(float(ws[:, 3].sum() / ws[:, 2].sum()), abs=1e-12)
    assert res["eval_loss_token_mean"] == pytest.approx(float(ws[:, 0].sum() / ws[:, 1].sum()), abs=bar)
