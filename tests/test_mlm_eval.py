"""Masked-LM evaluation without a GPU: the loss restatement (tests/mlm_ref.py), the host regrouping of per-window sums into loss
batches, the collator glue, the mlm_eval command on a stand-in model (alone and under a 2-rank gloo group) and the C ABI's argument
checks and sizing."""
import ctypes as C
import json
import math
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp
from torch.nn import functional as F

import mlm_ref
from plantcaduceus_amd import engine, mlm_eval
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer


def _case(n, L, frac, seed):
    g = torch.Generator().manual_seed(seed)
    logits = torch.randn(n, L, 8, generator=g) * 3
    labels = torch.randint(0, 8, (n, L), generator=g)
    labels[torch.rand(n, L, generator=g) >= frac] = -100
    weights = torch.tensor([0.0, 0.1, 1.0])[torch.randint(0, 3, (n, L), generator=g)]
    return logits, labels, weights


# ---- the restatement itself ------------------------------------------------------------------------------------------------
def test_ref_matches_torch_cross_entropy():
    logits, labels, weights = _case(5, 40, 0.3, 0)
    want = F.cross_entropy(logits.double().view(-1, 8), labels.view(-1), ignore_index=-100)
    assert mlm_ref.loss(logits, labels).item() == pytest.approx(want.item(), rel=1e-12)
    tok = F.cross_entropy(logits.double().view(-1, 8), labels.view(-1), ignore_index=-100, reduction="none").view(5, 40)
    assert torch.allclose(mlm_ref.token_nll(logits, labels), tok, rtol=1e-12, atol=0)
    w = torch.where(labels >= 0, weights.double(), torch.zeros(5, 40, dtype=torch.float64))
    assert mlm_ref.loss(logits, labels, weights).item() == pytest.approx(((w * tok).sum() / w.sum()).item(), rel=1e-12)
    # negative labels and a custom ignore_index are ignored
    lab2 = labels.clone()
    lab2[labels == -100] = -5
    assert torch.equal(mlm_ref.token_nll(logits, lab2), mlm_ref.token_nll(logits, labels))
    lab3 = labels.clone()
    lab3[labels == -100] = 6
    lab3[labels == 6] = -100
    assert mlm_ref.loss(logits, lab3, ignore_index=6).item() == pytest.approx(mlm_ref.loss(logits, labels.masked_fill(labels == 6, -100)).item())
    # nothing labelled: nan, as F.cross_entropy
    none = torch.full((5, 40), -100)
    assert math.isnan(mlm_ref.loss(logits, none).item()) and math.isnan(mlm_ref.loss(logits, none, weights).item())
    assert math.isnan(F.cross_entropy(logits.view(-1, 8), none.view(-1)).item())
    s = mlm_ref.window_sums(logits, labels, weights)
    assert s.shape == (5, 4) and torch.equal(s[:, 2], (labels >= 0).sum(1).double())
    assert torch.equal(s[:, 3], ((logits.argmax(-1) == labels) & (labels >= 0)).sum(1).double())


# ---- host regrouping ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,bs", [(19, 8), (16, 8), (5, 8), (7, 1)])
def test_regrouping_matches_per_batch_losses(n, bs):
    """per-window sums -> per-loss-batch losses -> Trainer's eval_loss: equal to computing every batch's loss from its logits (short
    last batch included)"""
    logits, labels, weights = _case(n, 33, 0.2, n)
    sums = mlm_ref.window_sums(logits, labels, weights).numpy()
    losses, counts = mlm_eval.regroup_losses(sums, bs)
    assert counts.tolist() == [min(bs, n - b0) for b0 in range(0, n, bs)]
    for i, b0 in enumerate(range(0, n, bs)):
        want = mlm_ref.loss(logits[b0:b0 + bs], labels[b0:b0 + bs], weights[b0:b0 + bs]).item()
        assert losses[i] == pytest.approx(want, rel=1e-12)
    assert mlm_eval.trainer_eval_loss(sums, bs) == pytest.approx(mlm_ref.trainer_eval_loss(logits, labels, weights, bs), rel=1e-12)
    m = mlm_eval.metrics_from_sums(sums, bs, "eval")
    assert m["perplexity"] == math.exp(m["eval_loss"]) and m["eval_samples"] == n
    assert m["eval_loss_token_mean"] == pytest.approx(mlm_ref.loss(logits, labels, weights).item(), rel=1e-12)
    assert set(m) >= {"eval_loss", "perplexity", "eval_samples", "eval_token_accuracy", "eval_loss_token_mean"}


def test_regrouping_zero_weight_batch_is_nan():
    logits, labels, weights = _case(10, 20, 0.3, 3)
    weights[4:8] = 0
    sums = mlm_ref.window_sums(logits, labels, weights).numpy()
    losses, _ = mlm_eval.regroup_losses(sums, 4)
    assert np.isfinite(losses[0]) and math.isnan(losses[1]) and np.isfinite(losses[2])
    assert math.isnan(mlm_ref.loss(logits[4:8], labels[4:8], weights[4:8]).item())
    assert math.isnan(mlm_eval.trainer_eval_loss(sums, 4)) and math.isnan(mlm_ref.trainer_eval_loss(logits, labels, weights, 4))
    assert math.isnan(mlm_eval.trainer_eval_loss(np.zeros((0, 4)), 4))


# ---- collator glue ------------------------------------------------------------------------------------------------------
def _seqs(n, L, seed, alphabet="ACGTacgtN"):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list(alphabet), size=L)) for _ in range(n)]


def test_collator_glue():
    from transformers import set_seed
    tok = CaduceusTokenizer()
    seqs = _seqs(11, 50, 0)
    ids, special, w = mlm_eval.tokenize_windows(tok, seqs, 0.25)
    assert ids.shape == (11, 50) and np.array_equal(ids, tok.encode_batch(seqs))
    lower = np.array([[c.islower() for c in s] for s in seqs])
    assert np.array_equal(w, np.where(lower, np.float32(0.25), np.float32(1.0)))          # lower-case -> the soft-mask weight
    assert np.array_equal(special, np.array([[c in "Nn" for c in s] for s in seqs]))      # N -> [UNK]: never masked
    coll = mlm_eval.make_collator(tok, 0.15)
    set_seed(7)
    masked, labels = mlm_eval.mask_windows(coll, ids, special, 4)
    set_seed(7)
    masked2, labels2 = mlm_eval.mask_windows(coll, ids, special, 4)
    assert np.array_equal(masked, masked2) and np.array_equal(labels, labels2)            # same seed -> same masks
    # = calling torch_mask_tokens directly, once per loss batch in dataset order
    set_seed(7)
    for b0 in range(0, 11, 4):
        x, y = coll.torch_mask_tokens(torch.from_numpy(ids[b0:b0 + 4].copy()),
                                      special_tokens_mask=torch.from_numpy(special[b0:b0 + 4].copy()))
        assert np.array_equal(masked[b0:b0 + 4], x.numpy()) and np.array_equal(labels[b0:b0 + 4], y.numpy())
    on = labels != -100
    assert 0 < on.sum() < on.size and not (on & special).any()
    assert np.array_equal(labels[on], ids[on])                                           # labels: the original token on the masked set,
    assert (labels[~on] == -100).all() and np.array_equal(masked[~on], ids[~on])          # -100 and an untouched input off it
    assert (masked[on] == tok.mask_token_id).mean() > 0.5
    assert masked.dtype == np.int32 and labels.dtype == np.int32 and masked.min() >= 0 and masked.max() < 8
    set_seed(8)
    assert not np.array_equal(mlm_eval.mask_windows(coll, ids, special, 4)[1], labels)
    with pytest.raises(ValueError, match="unequal length"):
        mlm_eval.tokenize_windows(tok, ["ACGT", "ACG"], 1.0)


# ---- the command on a stand-in model ---------------------------------------------------------------------------------------
class _OracleLossModel:
    """Stand-in for CaduceusForMaskedLM on the CPU: the oracle's logits, the loss head restated by mlm_ref (fp32 outputs as the
    engine gives them)."""

    def __init__(self):
        from oracle import caduceus_oracle as O
        from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
        cfg = make_config("x", d_model=32, n_layer=1)
        self.inner = O.OracleForMaskedLM(O.params_from_state_dict(synthetic_state_dict(cfg, seed=2), cfg))
        self.config = cfg
        self.calls = []

    def __call__(self, input_ids, labels, loss_weights, output_logits=True, return_window_sums=False, return_token_nll=False):
        self.calls.append(int(input_ids.shape[0]))
        lg = self.inner(input_ids=input_ids).logits.float()
        out = {"window_sums": mlm_ref.window_sums(lg, labels, loss_weights).float()}
        if return_token_nll:
            out["token_nll"] = mlm_ref.token_nll(lg, labels).float()
        return out


def _dataset(path, n=13, L=24):
    import pandas as pd
    os.makedirs(path, exist_ok=True)
    pd.DataFrame({"seq": _seqs(n, L, 1), "chrom": ["1"] * n}).to_parquet(os.path.join(path, "validation.parquet"))
    pd.DataFrame({"seq": _seqs(n - 3, L, 2)}).to_csv(os.path.join(path, "test.tsv"), sep="\t", index=False)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _cli(data, out, extra=()):
    model = _OracleLossModel()
    real = mlm_eval.load_model_and_tokenizer
    mlm_eval.load_model_and_tokenizer = lambda *a, **k: (model, CaduceusTokenizer())
    try:
        res = mlm_eval.main(["--model_name_or_path", "unused", "--dataset_name", data, "--do_eval", "--do_test", "--output_dir", out,
                             "--per_device_eval_batch_size", "4", "--soft_masked_loss_weights_evaluation", "0.0", "--device", "cpu",
                             "--engine_batch_size", "5", "--seed", "3", "--token-nll-out", os.path.join(out, "nll.npy"), *extra])
    finally:
        mlm_eval.load_model_and_tokenizer = real
    return model, res


def _cli_worker(rank, ws, port, data, out):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(ws), LOCAL_RANK=str(rank))
    torch.set_num_threads(2)
    _cli(data, out)
    assert not dist.is_initialized()
    open(os.path.join(out, f"done_{rank}"), "w").close()


def test_cli_world_1_and_gloo_world_2(tmp_path):
    from transformers import set_seed
    data = str(tmp_path / "data")
    _dataset(data)
    one = str(tmp_path / "one")
    os.makedirs(one)
    model, res = _cli(data, one)
    assert model.calls == [5, 5, 3, 5, 5]                      # the engine batch is free of the loss batch
    ev = json.load(open(os.path.join(one, "eval_results.json")))
    te = json.load(open(os.path.join(one, "test_results.json")))
    assert ev == json.loads(json.dumps(res["eval"])) and ev["eval_samples"] == 13 and te["test_samples"] == 10
    assert ev["perplexity"] == math.exp(ev["eval_loss"]) and te["perplexity"] == math.exp(te["test_loss"])
    # the same numbers from the pieces: masks per loss batch of 4 after set_seed(3), weight 0 at lower-case bases
    import pandas as pd
    tok = CaduceusTokenizer()
    seqs = list(pd.read_parquet(os.path.join(data, "validation.parquet"))["seq"])
    ids, special, w = mlm_eval.tokenize_windows(tok, seqs, 0.0)
    set_seed(3)
    masked, labels = mlm_eval.mask_windows(mlm_eval.make_collator(tok, 0.15), ids, special, 4)
    lg = model.inner(input_ids=torch.from_numpy(masked).long()).logits.float()
    want = mlm_ref.trainer_eval_loss(lg, torch.from_numpy(labels), torch.from_numpy(w), 4)
    assert ev["eval_loss"] == pytest.approx(want, rel=1e-5) or (math.isnan(want) and math.isnan(ev["eval_loss"]))
    nll = np.load(os.path.join(one, "nll.eval.npy"))
    assert nll.shape == (13, 24) and (nll[labels < 0] == 0).all()
    assert np.load(os.path.join(one, "nll.test.npy")).shape == (10, 24)
    # max_eval_samples
    cut = str(tmp_path / "cut")
    os.makedirs(cut)
    _, r3 = _cli(data, cut, ["--max_eval_samples", "6"])
    assert r3["eval"]["eval_samples"] == 6 and r3["test"]["test_samples"] == 10
    # two ranks over gloo: the same JSON, written by rank 0
    two = str(tmp_path / "two")
    os.makedirs(two)
    mp.spawn(_cli_worker, args=(2, _free_port(), data, two), nprocs=2, join=True)
    assert all(os.path.exists(os.path.join(two, f"done_{r}")) for r in range(2))
    for f in ("eval_results.json", "test_results.json"):
        assert open(os.path.join(two, f)).read() == open(os.path.join(one, f)).read()
    assert np.array_equal(np.load(os.path.join(two, "nll.eval.npy")), nll)


def test_cli_refuses_training_and_unequal_windows(tmp_path, monkeypatch):
    import pandas as pd
    monkeypatch.setattr(mlm_eval, "load_model_and_tokenizer", lambda *a, **k: (_OracleLossModel(), CaduceusTokenizer()))
    with pytest.raises(SystemExit, match="do_train"):
        mlm_eval.main(["--model_name_or_path", "u", "--dataset_name", "d", "--do_train", "--output_dir", str(tmp_path)])
    with pytest.raises(SystemExit, match="nothing to do"):
        mlm_eval.main(["--model_name_or_path", "u", "--dataset_name", "d", "--output_dir", str(tmp_path)])
    f = str(tmp_path / "v.tsv")
    pd.DataFrame({"seq": ["ACGT", "ACGTA"]}).to_csv(f, sep="\t", index=False)
    with pytest.raises(ValueError, match="unequal length"):
        mlm_eval.main(["--model_name_or_path", "u", "--dataset_name", f, "--do_eval", "--output_dir", str(tmp_path), "--device", "cpu"])
    pd.DataFrame({"sequence": ["ACGT"]}).to_csv(f, sep="\t", index=False)
    with pytest.raises(KeyError, match="seq"):
        mlm_eval.main(["--model_name_or_path", "u", "--dataset_name", f, "--do_eval", "--output_dir", str(tmp_path), "--device", "cpu"])


def test_model_refuses_labels_with_positions():
    from plantcaduceus_amd.checkpoint import make_config
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    m = CaduceusForMaskedLM(make_config("x", d_model=32, n_layer=1))
    ids = torch.zeros(1, 8, dtype=torch.long)
    with pytest.raises(ValueError, match="positions"):
        m(input_ids=ids, labels=ids, positions=[1])
    with pytest.raises(ValueError, match="loss_weights need labels"):
        m(input_ids=ids, loss_weights=torch.ones(1, 8))
    with pytest.raises(RuntimeError, match="ROCm device"):          # no CPU fallback
        m(input_ids=ids, labels=ids)


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _handle(lib, D, dtype, split=False):
    c = engine.PcadConfig(d_model=D, n_layer=2, d_state=16, d_conv=4, expand=2, dt_rank=(D + 15) // 16, vocab=8, eps=1e-5,
                          dtype=dtype, residual_in_fp32=1, complement=(C.c_int32 * 8)(0, 1, 2, 6, 5, 4, 3, 7))
    h = C.c_void_p()
    assert lib.pcad_create(C.byref(c), C.byref(h)) == 0
    if split:
        assert lib.pcad_set_option(h, b"f32_gemm_split", 1) == 0
    return h


# pcad_workspace_bytes of the library before the loss head existed (the values tests/test_seqcls.py pins): the head's partials
# reuse buffers that are dead after the last out_proj, so the forward's workspace is unchanged
WORKSPACE_BYTES = {
    (768, 1, False, 40, 600): 1058112000, (768, 0, True, 4, 8192): 3078750208, (1024, 1, False, 32, 8192): 15353249792,
    (128, 0, False, 3, 45): 3124224,
}


def test_workspace_bytes_unchanged():
    lib = engine.load_library()
    for (D, dt, split, B, L), want in WORKSPACE_BYTES.items():
        h = _handle(lib, D, dt, split)
        got = lib.pcad_workspace_bytes(h, B, L)
        lib.pcad_destroy(h)
        assert got == want, (D, dt, split, B, L, got)


def test_loss_abi_validates_without_gpu():
    lib = engine.load_library()
    assert engine.STATUS_BAD_LABEL == 4
    h = _handle(lib, 128, 0)
    one = C.c_void_p(256)        # a non-null pointer that is never dereferenced: every call below is refused before any device work
    # unbound handle
    assert lib.pcad_forward_loss(h, one, one, None, -100, 1, 8, one, None, None, one, 1 << 20, None) == -2
    assert b"not bound" in lib.pcad_last_error()
    # bad arguments
    assert lib.pcad_forward_loss(None, one, one, None, -100, 1, 8, one, None, None, one, 1 << 20, None) == -1
    assert lib.pcad_forward_loss(h, one, None, None, -100, 1, 8, one, None, None, one, 1 << 20, None) == -1
    assert b"labels" in lib.pcad_last_error()
    assert lib.pcad_forward_loss(h, one, one, None, -100, 1, 8, None, None, None, one, 1 << 20, None) == -1
    assert lib.pcad_forward_loss(h, one, one, None, -100, 1, 0, one, None, None, one, 1 << 20, None) == -1
    assert lib.pcad_forward_loss(h, one, one, None, -100, -1, 8, one, None, None, one, 1 << 20, None) == -1
    lib.pcad_destroy(h)
    # sizing: one partial [4] fp32 per (window, 64-position segment), rounded up to 256 bytes; a function of B and L only
    assert lib.pcad_loss_head_scratch_bytes(3, 600) == 512 and lib.pcad_loss_head_scratch_bytes(32, 8192) == 32 * 128 * 16
    assert lib.pcad_loss_head_scratch_bytes(0, 600) == 0 and lib.pcad_loss_head_scratch_bytes(3, 0) == 0
    f = C.c_float(1e-5)
    assert lib.pcad_loss_head(None, None, None, None, None, None, None, -100, None, None, None, 1, 8, 64, f, None, None, 0, 0, 0,
                              None, 0, None) == -1
    assert lib.pcad_loss_head(one, one, one, one, one, one, None, -100, one, None, None, 1, 8, 60, f, None, None, 0, 0, 0, one, 256,
                              None) == -1                       # D % 8
    assert lib.pcad_loss_head(one, one, one, one, one, one, None, -100, one, None, None, 1, 8, 64, f, None, None, 0, 1, 0, one, 256,
                              None) == -1                       # fp32 model with a bf16 residual
    assert lib.pcad_loss_head(one, one, one, one, one, one, None, -100, one, None, None, 1, 8, 64, f, None, None, 0, 0, 1, one, 256,
                              None) == -1                       # fragment layout needs D % 256 == 0
    assert lib.pcad_loss_head(one, one, one, one, one, one, None, -100, one, None, None, 1, 8, 64, f, None, None, 0, 0, 0, one, 0,
                              None) == -3                       # scratch too small
