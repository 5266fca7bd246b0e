"""Sequence classification without a GPU: the PEFT adapter loader and its LoRA policy, tokenizer padding / truncation, the
`sampling_rate` selection, the host metrics of the predict / evaluate commands, the tokenize command and the C ABI's sizing."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

from plantcaduceus_amd import adapters, engine, lora_predict
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    cfg = make_config("tiny", d_model=128, n_layer=2)
    path = str(tmp_path_factory.mktemp("base"))
    save_checkpoint(path, cfg, synthetic_state_dict(cfg, seed=3))
    return cfg, path


# ---- adapters ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [dict(), dict(prefix=False), dict(default_infix=True), dict(bin_format=True)])
def test_adapter_round_trip(base, tmp_path, variant):
    cfg, bp = base
    sd = adapters.make_synthetic_adapter(str(tmp_path), cfg, 92, base_path=bp, seed=4, **variant)
    m = adapters.load_adapter(str(tmp_path), task_type="multi_label", num_labels=92)
    score = [v for k, v in sd.items() if ".score" in "." + k or k.startswith("score")]
    assert len(score) == 1
    assert torch.equal(m.score.weight, score[0])
    info = m.adapter_info
    assert info["r"] == 8 and info["lora_alpha"] == 32 and info["target_modules"] == ["in_proj", "out_proj", "x_proj"]
    assert info["lora_pairs"] == 2 * 3 * cfg.n_layer and info["nonzero_lora_B"] == []
    assert m.config.num_labels == 92 and m.config.problem_type == "multi_label_classification"
    assert m.score.weight.dtype == torch.float32 and m.pooling_strategy == "mean"


def test_adapter_task_shapes(base, tmp_path):
    cfg, bp = base
    adapters.make_synthetic_adapter(str(tmp_path / "c"), cfg, 2, base_path=bp)
    adapters.make_synthetic_adapter(str(tmp_path / "r"), cfg, 1, base_path=bp)
    mc = adapters.load_adapter(str(tmp_path / "c"), task_type="classification")
    mr = adapters.load_adapter(str(tmp_path / "r"), task_type="regression")
    assert mc.config.num_labels == 2 and mc.config.id2label == {0: "NEGATIVE", 1: "POSITIVE"}
    assert mr.config.num_labels == 1 and mr.config.problem_type == "regression"
    with pytest.raises(ValueError, match="num_labels"):
        adapters.load_adapter(str(tmp_path / "c"), task_type="classification".replace("classification", "regression"))
    with pytest.raises(ValueError, match="num_labels > 1"):
        adapters.load_adapter(str(tmp_path / "c"), task_type="multi_label")


def test_adapter_unknown_key_fails(base, tmp_path):
    from safetensors.torch import load_file, save_file
    cfg, bp = base
    adapters.make_synthetic_adapter(str(tmp_path), cfg, 2, base_path=bp)
    fn = os.path.join(str(tmp_path), "adapter_model.safetensors")
    sd = load_file(fn)
    sd["base_model.model.caduceus.backbone.layers.0.mixer.submodule.mamba_fwd.dt_proj.lora_A.weight"] = torch.zeros(8, 4)
    save_file(sd, fn)
    with pytest.raises(ValueError, match="unexpected tensor .*dt_proj"):
        adapters.load_adapter(str(tmp_path), task_type="classification")


def test_adapter_missing_score_fails(base, tmp_path):
    from safetensors.torch import load_file, save_file
    cfg, bp = base
    adapters.make_synthetic_adapter(str(tmp_path), cfg, 2, base_path=bp)
    fn = os.path.join(str(tmp_path), "adapter_model.safetensors")
    sd = {k: v for k, v in load_file(fn).items() if "score" not in k}
    save_file(sd, fn)
    with pytest.raises(ValueError, match="no score weight"):
        adapters.load_adapter(str(tmp_path), task_type="classification")


def test_lora_policy(base, tmp_path):
    cfg, bp = base
    adapters.make_synthetic_adapter(str(tmp_path / "zero"), cfg, 2, base_path=bp)
    assert adapters.load_adapter(str(tmp_path / "zero"), task_type="classification", lora_deltas="auto").adapter_info["nonzero_lora_B"] == []
    adapters.make_synthetic_adapter(str(tmp_path / "nz"), cfg, 2, base_path=bp, lora_b_scale=0.1)
    with pytest.raises(ValueError) as ei:
        adapters.load_adapter(str(tmp_path / "nz"), task_type="classification")
    msg = str(ei.value)
    assert "layers.0.mixer.submodule.mamba_fwd." in msg and "lora_B.weight" in msg and "lora_deltas='ignore'" in msg
    m = adapters.load_adapter(str(tmp_path / "nz"), task_type="classification", lora_deltas="ignore")
    assert len(m.adapter_info["nonzero_lora_B"]) == 2 * 3 * cfg.n_layer and m.adapter_info["max_abs_delta"] > 0
    with pytest.raises(ValueError):
        adapters.load_adapter(str(tmp_path / "zero"), task_type="classification", lora_deltas="merge")


def test_seqcls_from_pretrained_reports_missing_score(base, caplog):
    from plantcaduceus_amd.modeling_caduceus import CaduceusForSequenceClassification
    _, bp = base
    with caplog.at_level("WARNING"):
        a = CaduceusForSequenceClassification.from_pretrained(bp, num_labels=3, problem_type="multi_label_classification")
    assert "score.weight" in caplog.text
    b = CaduceusForSequenceClassification.from_pretrained(bp, num_labels=3)
    assert torch.equal(a.score.weight, b.score.weight) and a.score.weight.shape == (3, 128)     # deterministic initialisation
    with pytest.raises(NotImplementedError):
        CaduceusForSequenceClassification(a.config, conjoin_eval=True)


def test_auto_class_registered(base):
    import plantcaduceus_amd
    from transformers import AutoModelForSequenceClassification
    from plantcaduceus_amd.modeling_caduceus import CaduceusForSequenceClassification
    plantcaduceus_amd.register()
    _, bp = base
    m = AutoModelForSequenceClassification.from_pretrained(bp, trust_remote_code=True, num_labels=2)
    assert isinstance(m, CaduceusForSequenceClassification) and m.num_labels == 2


def test_loss_follows_hf_problem_types(base):
    from plantcaduceus_amd.modeling_caduceus import CaduceusForSequenceClassification
    from torch.nn import functional as F
    _, bp = base
    g = torch.Generator().manual_seed(0)
    lg = torch.randn(6, 2, generator=g)
    m = CaduceusForSequenceClassification.from_pretrained(bp, num_labels=2)
    lab = torch.tensor([0, 1, 1, 0, 1, 0])
    assert torch.equal(m.loss_from_logits(lg, lab), F.cross_entropy(lg, lab))
    m = CaduceusForSequenceClassification.from_pretrained(bp, num_labels=1, problem_type="regression")
    y = torch.randn(6, generator=g)
    assert torch.equal(m.loss_from_logits(lg[:, :1], y), F.mse_loss(lg[:, 0], y))
    m = CaduceusForSequenceClassification.from_pretrained(bp, num_labels=2, problem_type="multi_label_classification")
    yy = (torch.rand(6, 2, generator=g) > 0.5).float()
    assert torch.equal(m.loss_from_logits(lg, yy), F.binary_cross_entropy_with_logits(lg, yy))


# ---- tokenizer ---------------------------------------------------------------------------------------------------------
def test_tokenizer_padding_and_truncation():
    t = CaduceusTokenizer()
    assert t.padding_side == "left" and t.pad_token_id == 0
    out = t(["ACG", "acgtac", "", "n"], padding="max_length", truncation=True, max_length=4, add_special_tokens=False)
    assert out["input_ids"] == [[0, 3, 4, 5], [3, 4, 5, 6], [0, 0, 0, 0], [0, 0, 0, 2]]
    r = CaduceusTokenizer(padding_side="right")
    assert r(["acg", "acgtac"], padding="max_length", truncation=True, max_length=5)["input_ids"] == [[3, 4, 5, 0, 0], [3, 4, 5, 6, 3]]
    assert r(["acg", "ac"], padding=True)["input_ids"] == [[3, 4, 5], [3, 4, 0]]
    pt = t(["acgt", "gg"], padding="max_length", truncation=True, max_length=3, return_tensors="pt")["input_ids"]
    assert pt.dtype == torch.int64 and pt.tolist() == [[3, 4, 5], [0, 5, 5]]
    with pytest.raises(ValueError):
        t(["acgtac"], padding="max_length", truncation=False, max_length=3)
    # vectorised form = per-sequence form
    rng = np.random.default_rng(0)
    seqs = ["".join(rng.choice(list("ACGTNacgt"), size=int(rng.integers(0, 40)))) for _ in range(50)]
    arr = t.encode_batch_padded(seqs, max_length=24)
    for s, row in zip(seqs, arr):
        ids = t.encode(s)[:24]
        assert row.tolist() == [0] * (24 - len(ids)) + ids


def test_tokenizer_unpadded_path_unchanged():
    t = CaduceusTokenizer()
    assert t(["acg", "tta"], return_tensors="pt")["input_ids"].tolist() == [[3, 4, 5], [6, 6, 3]]
    assert t("acgN")["input_ids"] == [3, 4, 5, 2]
    with pytest.raises(ValueError, match="unequal length"):
        t(["acg", "ac"], return_tensors="pt")
    assert t.encode_batch(["acg", "gta"], mask_index=1).tolist() == [[3, 1, 5], [5, 1, 3]]


def test_tokenizer_padding_side_from_snapshot(tmp_path):
    import json
    CaduceusTokenizer(padding_side="right").save_pretrained(str(tmp_path))
    assert json.load(open(tmp_path / "tokenizer_config.json"))["padding_side"] == "right"
    assert CaduceusTokenizer.from_pretrained(str(tmp_path)).padding_side == "right"


# ---- sampling_rate -----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n,rate,seed", [(100, 0.3, 42), (7, 0.01, 1), (1000, 1.0, 5), (37, 0.5, 0)])
def test_sampling_rate_matches_datasets(n, rate, seed):
    datasets = pytest.importorskip("datasets")
    ds = datasets.Dataset.from_dict({"i": list(range(n))})
    k = max(min(int(rate * n), n), 1)
    want = ds.shuffle(seed=seed).select(range(k))["i"]
    assert lora_predict.sample_indices(n, rate, seed).tolist() == list(want)
    assert lora_predict.sample_indices(n, None, seed) is None
    with pytest.raises(ValueError):
        lora_predict.sample_indices(n, 1.5, seed)


# ---- metrics -----------------------------------------------------------------------------------------------------------
def test_metrics_match_sklearn_scipy():
    skm = pytest.importorskip("sklearn.metrics")
    stats = pytest.importorskip("scipy.stats")
    rng = np.random.default_rng(0)
    n = 257
    lg = rng.normal(size=(n, 2)).astype(np.float32)
    lg[::7] = lg[0]                                     # ties in the scores
    y = rng.integers(0, 2, n)
    got = lora_predict.metrics_classification(lg, y)
    probs = torch.softmax(torch.tensor(lg), 1)[:, 1].numpy()
    preds = lg.argmax(1)
    want = {"accuracy": skm.accuracy_score(y, preds), "f1": skm.f1_score(y, preds), "roc_auc": skm.roc_auc_score(y, probs),
            "average_precision": skm.average_precision_score(y, probs), "balance": y.sum() / n}
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-12), k
    assert list(got) == list(want)

    pr = rng.normal(size=(n, 1)).astype(np.float32)
    pr[::5] = pr[1]
    lab = (pr[:, 0] * 0.5 + rng.normal(size=n)).round(1)         # ties in the labels
    got = lora_predict.metrics_regression(pr, lab)
    p = pr.squeeze()
    mse = ((p - lab) ** 2).mean()
    want = {"mse": mse, "rmse": np.sqrt(mse), "mae": np.abs(p - lab).mean(),
            "r2": 1 - ((lab - p) ** 2).sum() / (((lab - lab.mean()) ** 2).sum() + 1e-8),
            "pearson_r": stats.pearsonr(p, lab)[0], "spearman_r": stats.spearmanr(p, lab)[0]}
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-6), k
    assert list(got) == list(want)

    NL = 92
    lgm = rng.normal(size=(n, NL)).astype(np.float32)
    lgm[:, 3] = 0.0                                     # ties
    ym = rng.integers(0, 2, (n, NL))
    ym[:50] = (lgm[:50] > 0).astype(int)                 # some exact-match rows
    got = lora_predict.metrics_multilabel(lgm, ym)
    pm = torch.sigmoid(torch.tensor(lgm)).numpy()
    pdm = (pm > 0.5).astype(int)
    want = {"accuracy": skm.accuracy_score(ym, pdm), "f1": skm.f1_score(ym, pdm, average="micro"),
            "roc_auc": skm.roc_auc_score(ym, pm, average="micro"),
            "average_precision": skm.average_precision_score(ym, pm, average="micro")}
    for k in want:
        assert got[k] == pytest.approx(want[k], rel=1e-9, abs=1e-12), k
    assert list(got) == list(want)


# ---- commands ----------------------------------------------------------------------------------------------------------
def test_tokenize_command_round_trip(base, tmp_path):
    import pandas as pd
    _, bp = base
    seqs = ["ACGTACGTAA", "acg", "TTTTTTTTTTTTTTTT", "NNACG"]
    tsv = tmp_path / "x.tsv"
    pd.DataFrame({"SEQUENCE": seqs, "label": ["0101", "1111", "0000", "1000"]}).to_csv(tsv, sep="\t", index=False)
    out = str(tmp_path / "x.parquet")
    lora_predict.main(["tokenize", "--data-dir", str(tsv), "--model_name", bp, "--sequence-length", "12", "--output_path", out,
                       "--task_type", "multi_label"])
    ids, labels, name = lora_predict.read_tokenized(out)
    t = CaduceusTokenizer()
    assert ids.dtype == np.int32 and ids.shape == (4, 12)
    assert np.array_equal(ids, t.encode_batch_padded(seqs, max_length=12))
    assert ids[1].tolist() == [0] * 9 + [3, 4, 5]           # left padding (the snapshot's tokenizer default)
    assert name == "labels" and labels.tolist() == [[0, 1, 0, 1], [1, 1, 1, 1], [0, 0, 0, 0], [1, 0, 0, 0]]
    tsv2 = tmp_path / "y.tsv"
    pd.DataFrame({"Sequence": seqs, "Label": [0, 1, 1, 0]}).to_csv(tsv2, sep="\t", index=False)
    out2 = lora_predict.tokenize(data_dir=str(tsv2), model_name=bp, sequence_length=8)
    assert out2 == str(tmp_path / "y.parquet")
    ids2, labels2, name2 = lora_predict.read_tokenized(out2)
    assert ids2.shape == (4, 8) and name2 == "label" and labels2.tolist() == [0, 1, 1, 0]


def test_cli_accepts_both_flag_spellings():
    p = lora_predict.build_parser()
    a = p.parse_args(["predict", "--checkpoint_dir", "a", "--data-dir", "b", "--task-type", "multi_label", "--num_labels", "92",
                      "--sampling-rate", "0.5", "--lora-deltas", "ignore", "--dtype", "bfloat16", "--pooling", "max"])
    b = p.parse_args(["predict", "--checkpoint-dir", "a", "--data_dir", "b", "--task_type", "multi_label", "--num-labels", "92",
                      "--sampling_rate", "0.5", "--lora_deltas", "ignore", "--dtype", "bfloat16", "--pooling", "max"])
    assert vars(a) == vars(b)
    assert a.checkpoint_dir == "a" and a.data_dir == "b" and a.num_labels == 92 and a.sampling_rate == 0.5
    e = p.parse_args(["evaluate", "--checkpoint_dir", "a", "--data_dir", "b"])
    assert e.dtype == "float32" and e.pooling == "mean" and e.lora_deltas == "auto" and e.batch_size == 32 and e.seed == 42
    t = p.parse_args(["tokenize", "--data_dir", "x", "--model-name", "m"])
    assert t.sequence_length == 8192 and t.model_name == "m"


# ---- C ABI -------------------------------------------------------------------------------------------------------------
def _handle(lib, D, dtype, split=False):
    c = engine.PcadConfig(d_model=D, n_layer=2, d_state=16, d_conv=4, expand=2, dt_rank=(D + 15) // 16, vocab=8, eps=1e-5,
                          dtype=dtype, residual_in_fp32=1, complement=(C.c_int32 * 8)(0, 1, 2, 6, 5, 4, 3, 7))
    h = C.c_void_p()
    assert lib.pcad_create(C.byref(c), C.byref(h)) == 0
    if split:
        assert lib.pcad_set_option(h, b"f32_gemm_split", 1) == 0
    return h


# pcad_workspace_bytes of the library before the pooled head existed (its partials reuse buffers that are dead after the last
# out_proj, so the forward's workspace is unchanged)
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


def test_pooled_abi_validates_without_gpu():
    lib = engine.load_library()
    h = _handle(lib, 128, 0)
    # unbound handle: refused before any device work
    assert lib.pcad_forward_pooled(h, None, 1, 8, 0, None, 2, None, None, None, 0, None) != 0
    assert lib.pcad_forward_pooled(h, None, 1, 8, 7, None, 2, None, None, None, 0, None) == -1
    assert b"pooling" in lib.pcad_last_error()
    assert lib.pcad_forward_pooled(h, None, 1, 8, 0, None, 257, None, None, None, 0, None) == -1
    lib.pcad_destroy(h)
    assert lib.pcad_pooled_head_scratch_bytes(3, 600, 768, 0) == 3 * 2 * 10 * 768 * 4
    assert lib.pcad_pooled_head_scratch_bytes(3, 600, 768, 2) == 3 * 2 * 768 * 4
    assert lib.pcad_pooled_head_scratch_bytes(3, 600, 768, 9) == 0
    assert lib.pcad_pooled_head(None, None, None, None, 2, None, None, 1, 8, 64, C.c_float(1e-5), 0, None, None, 0, 0, 0, None, 0,
                                None) == -1
