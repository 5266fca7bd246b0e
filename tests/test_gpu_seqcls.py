"""Sequence classification on the MI355X: the pooled head (csrc/pool.hip) as an operator, inside the forward
(pcad_forward_pooled / CaduceusForSequenceClassification), and the LoRA predict / evaluate commands end to end.

The head's CPU restatement lives in tests/seqcls_ref.py (head_ref): the recalled Caduceus remote code's
    hs = stack([H[..., :D], flip(H[..., D:], dims=[1, 2])], -1); pooled = pool(hs, 1); logits = (score(p0) + score(p1)) / 2
with the rounding points of DESIGN.md §4f, applied to hidden states (the oracle's, or this engine's own)."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pandas as pd
import pytest
import torch

from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine
from plantcaduceus_amd.adapters import make_synthetic_adapter
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM, CaduceusForSequenceClassification
from plantcaduceus_amd.ops import to_res_fragment
from seqcls_ref import head_ref, pool_strands, rnd, score_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
POOLINGS = ("mean", "max", "first", "last")


def dot_scale(pooled, W):
    """The size of the terms of the score products, max over (window, label) of sum_k |pooled_k| |W_nk| (both strands): the
    scale an fp32 dot product's rounding is relative to (a logit can be a cancelling sum, far below its terms)."""
    a = pooled.abs().double()
    w = W.float().abs().double().cpu()
    return torch.maximum(a[:, 0] @ w.T, a[:, 1] @ w.T).max().float()


def ulp_bf16(x):
    e = torch.floor(torch.log2(x.abs().clamp_min(1e-30)))
    return torch.pow(2.0, e - 7)


# ---- operator ------------------------------------------------------------------------------------------------------
OP_CASES = [  # (D, L, NL, B, frag)
    (64, 1, 2, 3, False), (64, 45, 92, 3, False), (768, 600, 1, 2, False), (768, 45, 2, 3, False),
    (1536, 600, 92, 2, False), (1536, 8192, 2, 1, False), (768, 8192, 92, 1, True), (1536, 64, 1, 2, True),
]


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
@pytest.mark.parametrize("pooling", POOLINGS)
def test_pooled_head_operator(dtype, pooling):
    lib = engine.load_library()
    g = torch.Generator().manual_seed(3)
    dt = engine._DT[dtype]
    for D, L, NL, B, frag in OP_CASES:
        rows = 2 * B * L
        h = (torch.randn(rows, D, generator=g)).to(dtype)
        res = torch.randn(rows, D, generator=g) * 0.5 + 1.0                  # fp32 residual stream, non-zero mean
        w = torch.rand(D, generator=g) + 0.5
        W = rnd(torch.randn(NL, D, generator=g) * 0.05, dtype)
        v = h.float() + res
        o = rnd(v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + 1e-5) * w, dtype)
        pooled_ref = pool_strands(o[:B * L].view(B, L, D), o[B * L:].view(B, L, D), pooling, dtype)
        lg_ref = score_ref(pooled_ref, W, dtype)
        res_dev = (to_res_fragment(res) if frag else res).to(DEV).contiguous()
        hd, wd, Wd = h.to(DEV), w.to(DEV), W.to(DEV)
        pooled = torch.empty(B, 2, D, device=DEV)
        lg = torch.empty(B, NL, device=DEV)
        pid = engine.POOLING[pooling]
        nb = lib.pcad_pooled_head_scratch_bytes(B, L, D, pid)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
        sp = (scratch.data_ptr() + 255) // 256 * 256
        rc = lib.pcad_pooled_head(hd.data_ptr(), res_dev.data_ptr(), wd.data_ptr(), Wd.data_ptr(), NL, pooled.data_ptr(),
                                  lg.data_ptr(), B, L, D, C.c_float(1e-5), pid, None, None, dt, engine.PCAD_F32, int(frag), sp, nb,
                                  engine._stream_ptr())
        assert rc == 0, lib.pcad_last_error()
        torch.cuda.synchronize()
        pooled, lg = pooled.cpu(), lg.cpu()
        case = (D, L, NL, B, frag)
        if dtype == torch.float32:
            assert ((pooled - pooled_ref).abs().max() / pooled_ref.abs().max()).item() <= 1e-6, case
            assert ((lg - lg_ref).abs().max() / dot_scale(pooled_ref, W)).item() <= 1e-6, case
        else:
            assert ((pooled - pooled_ref).abs() <= ulp_bf16(pooled_ref)).all(), case          # within 1 bf16 ulp
            assert ((lg - lg_ref).abs().max() / lg_ref.abs().max()).item() <= 2e-2, case
            if pooling != "mean":                                                          # no summation: exact
                assert torch.equal(pooled, pooled_ref), case


@pytest.mark.parametrize("pooling", ["mean", "max"])
@pytest.mark.parametrize("D", [384, 1024, 1536])
def test_pooled_head_bf16_residual(D, pooling):
    """The <bf16, bf16> pair (a bf16 model with residual_in_fp32 = False) at each width class: bf16 h and a bf16 residual against the
    same call with that residual widened to fp32.  pool_stage1_kernel only reads the residual and forms v = h + res in fp32, and a
    bf16 value is exact in fp32, so pooled and logits are bit-equal; the outputs start as NaN, so an unwritten row shows."""
    lib = engine.load_library()
    g = torch.Generator().manual_seed(D)
    B, L, NL = 3, 45, 2
    h = torch.randn(2 * B * L, D, generator=g).to(torch.bfloat16).to(DEV)
    res = (torch.randn(2 * B * L, D, generator=g) * 0.5 + 1.0).to(torch.bfloat16).to(DEV)
    w = (torch.rand(D, generator=g) + 0.5).to(DEV)
    W = rnd(torch.randn(NL, D, generator=g) * 0.05, torch.bfloat16).to(DEV)
    pid = engine.POOLING[pooling]
    nb = lib.pcad_pooled_head_scratch_bytes(B, L, D, pid)
    scratch = torch.empty(nb + 256, dtype=torch.uint8, device=DEV)
    sp = (scratch.data_ptr() + 255) // 256 * 256

    def run(r, res_dt):
        pooled = torch.full((B, 2, D), float("nan"), device=DEV)
        lg = torch.full((B, NL), float("nan"), device=DEV)
        rc = lib.pcad_pooled_head(h.data_ptr(), r.data_ptr(), w.data_ptr(), W.data_ptr(), NL, pooled.data_ptr(), lg.data_ptr(), B, L, D,
                                  C.c_float(1e-5), pid, None, None, engine.PCAD_BF16, res_dt, 0, sp, nb, engine._stream_ptr())
        assert rc == 0, lib.pcad_last_error()
        torch.cuda.synchronize()
        return pooled.cpu(), lg.cpu()

    got = run(res, engine.PCAD_BF16)
    want = run(res.float().contiguous(), engine.PCAD_F32)
    for name, a, b in zip(("pooled", "logits"), got, want):
        assert not torch.isnan(b).any(), name
        assert torch.equal(a, b), name


def test_pooled_head_reports_bad_tokens():
    lib = engine.load_library()
    B, L, D = 2, 45, 64
    h = torch.randn(2 * B * L, D, device=DEV)
    res = torch.randn(2 * B * L, D, device=DEV)
    w = torch.ones(D, device=DEV)
    W = torch.randn(2, D, device=DEV)
    ids = torch.full((B, L), 3, dtype=torch.int32, device=DEV)
    ids[1, 7] = 9
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    lg = torch.empty(B, 2, device=DEV)
    nb = lib.pcad_pooled_head_scratch_bytes(B, L, D, 0)
    scratch = torch.empty(nb, dtype=torch.uint8, device=DEV)
    assert lib.pcad_pooled_head(h.data_ptr(), res.data_ptr(), w.data_ptr(), W.data_ptr(), 2, None, lg.data_ptr(), B, L, D,
                                C.c_float(1e-5), 0, ids.data_ptr(), status.data_ptr(), 0, 0, 0, scratch.data_ptr(), nb,
                                engine._stream_ptr()) == 0
    torch.cuda.synchronize()
    assert int(status.item()) == 1


# ---- model -----------------------------------------------------------------------------------------------------------
def seqcls(cfg, sd, NL, dtype=torch.float32, pooling="mean", options=None, seed=5):
    if options:
        cfg.engine_options = dict(options)
    cfg.num_labels = NL
    m = CaduceusForSequenceClassification(cfg, pooling_strategy=pooling)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("caduceus.")}, strict=False)
    with torch.no_grad():
        m.score.weight.copy_(torch.randn(NL, cfg.d_model, generator=torch.Generator().manual_seed(seed)) * 0.05)
    return m.to(dtype).to(DEV).eval()


def rand_ids(B, L, seed):
    return torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(seed))


_ORACLE = {}


def oracle_hidden(cfg, sd, ids, bf16):
    key = (tuple(ids.shape), bf16)
    if key not in _ORACLE:
        if bf16:
            _ORACLE[key] = O.forward_strands(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16)["hidden"]
        else:
            _ORACLE[key] = O.forward_strands(ids, O.params_from_state_dict(sd, cfg))["hidden"]
    return _ORACLE[key]


@pytest.mark.parametrize("L", [45, 600])
@pytest.mark.parametrize("mode", ["fp32", "fp32_split", "bf16"])
def test_model_vs_oracle(L, mode):
    """fp32 and fp32 + f32_gemm_split: <= 1e-4 of max |logit| against the head restatement on the oracle's hidden states (the
    reference's parity budget), the predicted class identical where the oracle's margin exceeds that bar.  bf16 against the
    bf16-emulating oracle: 3e-2 of max |logit|, the bar of the bf16 hidden states / LM logits (tests/test_gpu_model.py)."""
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=11)
    ids = rand_ids(3, L, L)
    bf16 = mode == "bf16"
    H = oracle_hidden(cfg, sd, ids, bf16)
    dtype = torch.bfloat16 if bf16 else torch.float32
    bar = 3e-2 if bf16 else 1e-4
    for NL in (2, 1, 92):
        m = seqcls(make_config("tiny", d_model=128, n_layer=2), sd, NL, dtype,
                   options={"f32_gemm_split": 1} if mode == "fp32_split" else None)
        lg = m(input_ids=ids.to(DEV)).logits.cpu()
        assert lg.dtype == torch.float32 and lg.shape == (3, NL)
        ref, _ = head_ref(H, m.score.weight.detach().float(), "mean", dtype)
        scale = ref.abs().max()
        err = ((lg - ref).abs().max() / scale).item()
        print(f"{mode} L={L} NL={NL}: {err:.2e} of max |logit|")
        assert err <= bar, (mode, L, NL, err)
        if NL > 1:
            top2 = ref.topk(2, dim=-1).values
            sure = (top2[:, 0] - top2[:, 1]) > bar * scale
            assert torch.equal(lg.argmax(-1)[sure], ref.argmax(-1)[sure])


@pytest.mark.parametrize("dtype", [torch.float32, torch.bfloat16])
def test_engine_self_consistency_pc2_small(dtype):
    """PlantCAD2 Small width (d_model 768, 2 layers): forward_pooled equals the head restatement on this engine's own
    CaduceusForMaskedLM hidden_states[-1] (same weights, same options, same batch): fp32 1e-6 relative (pooled: of max |pooled|;
    logits: of the score products' terms, dot_scale - the head's fp32 dot products against float64), bf16 pooled vectors
    within one bf16 ulp (the head's fp32 mean in another summation order) and logits 1e-2 of max."""
    cfg = make_config("pc2-small", n_layer=2)
    sd = synthetic_state_dict(cfg, seed=2)
    mlm = CaduceusForMaskedLM(make_config("pc2-small", n_layer=2))
    mlm.load_state_dict(sd, strict=False)
    mlm.tie_weights()
    mlm = mlm.to(dtype).to(DEV).eval()
    for L, B in ((600, 40), (8192, 4)):
        ids = rand_ids(B, L, B)
        H = mlm(input_ids=ids.to(DEV), output_hidden_states=True).hidden_states[-1]
        for pooling, NL in (("mean", 2), ("max", 92), ("first", 1), ("last", 2)):
            m = seqcls(make_config("pc2-small", n_layer=2), sd, NL, dtype, pooling)
            out = m(input_ids=ids.to(DEV), pooled_out=True)
            lg, pooled = out.logits.cpu(), out["pooled"].cpu()
            ref, pref = head_ref(H, m.score.weight.detach().float(), pooling, dtype)
            if dtype == torch.float32:
                assert ((pooled - pref).abs().max() / pref.abs().max()).item() <= 1e-6, (L, pooling)
                assert ((lg - ref).abs().max() / dot_scale(pref, m.score.weight.detach())).item() <= 1e-6, (L, pooling)
            else:
                assert ((pooled - pref).abs() <= ulp_bf16(pref)).all(), (L, pooling)
                assert ((lg - ref).abs().max() / ref.abs().max()).item() <= 1e-2, (L, pooling)
            del m
    del mlm
    torch.cuda.empty_cache()


@pytest.mark.parametrize("pooling", POOLINGS)
def test_rc_invariance(pooling):
    """Classification logits of a batch equal those of its reverse complements (the head averages the two strands' scores):
    pins the head's strand wiring without any recalled code."""
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=4)
    m = seqcls(cfg, sd, 2, pooling=pooling)
    ids = rand_ids(5, 300, 1)
    comp = torch.tensor(cfg.complement_list()[:8])
    rc = comp[ids.flip(1)]
    a = m(input_ids=ids.to(DEV)).logits.cpu()
    b = m(input_ids=rc.to(DEV)).logits.cpu()
    if pooling in ("first", "last"):
        assert torch.equal(a, b)
    else:
        torch.testing.assert_close(a, b, rtol=1e-6, atol=1e-7)


def test_batch_and_chunk_independence():
    """fp32: one window's logits are bit-identical alone, inside a batch of 37 and with "chunk_seqs" cutting that batch into
    several chunks (the head's segmentation is a function of L only); "scan_segments" 0 keeps the batch-size-dependent small-launch
    forms of the scan / conv out of the comparison (include/pcad.h).  With "poison_workspace": no NaN, the same values."""
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=6)
    m = seqcls(cfg, sd, 3, options={"scan_segments": 0})
    eng = m._engine()
    ids = rand_ids(37, 600, 2)
    alone = m(input_ids=ids[5:6].to(DEV)).logits.cpu()
    batch = m(input_ids=ids.to(DEV)).logits.cpu()
    eng.set_option("chunk_seqs", 8)
    chunked = m(input_ids=ids.to(DEV)).logits.cpu()
    eng.set_option("poison_workspace", 1)
    poisoned = m(input_ids=ids.to(DEV)).logits.cpu()
    eng.set_option("poison_workspace", 0)
    eng.set_option("chunk_seqs", 0)
    assert torch.equal(alone[0], batch[5])
    assert torch.equal(batch, chunked)
    assert torch.isfinite(poisoned).all() and torch.equal(poisoned, chunked)


def test_forward_pooled_bad_token_raises():
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=6)
    m = seqcls(cfg, sd, 2)
    ids = rand_ids(2, 64, 3)
    ids[1, 10] = 11
    m(input_ids=ids.to(DEV))
    with pytest.raises(IndexError):
        m.check_status()


# ---- commands end to end ---------------------------------------------------------------------------------------------
def _snapshot(tmp_path):
    cfg = make_config("tiny", d_model=128, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=9)
    base = str(tmp_path / "base")
    save_checkpoint(base, cfg, sd)
    return cfg, base


def _tsv(path, n, L, task, NL, seed=0):
    rng = np.random.default_rng(seed)
    seqs = ["".join(rng.choice(list("ACGTN"), size=int(rng.integers(L - 20, L + 20)))) for _ in range(n)]
    if task == "classification":
        lab = rng.integers(0, 2, n)
    elif task == "regression":
        lab = rng.normal(size=n).round(4)
    else:
        lab = ["".join(str(x) for x in rng.integers(0, 2, NL)) for _ in range(n)]
    pd.DataFrame({"Sequence": seqs, "Label": lab}).to_csv(path, sep="\t", index=False)


@pytest.mark.parametrize("task,NL", [("classification", 2), ("regression", 1), ("multi_label", 92)])
def test_commands_end_to_end(tmp_path, task, NL):
    from plantcaduceus_amd import lora_predict
    from plantcaduceus_amd.adapters import load_adapter
    cfg, base = _snapshot(tmp_path)
    ad = str(tmp_path / "adapter")
    make_synthetic_adapter(ad, cfg, NL, base_path=base, seed=1)
    tsv, pq = str(tmp_path / "x.tsv"), str(tmp_path / "x.parquet")
    _tsv(tsv, 45, 256, task, NL)
    lora_predict.main(["tokenize", "--data_dir", tsv, "--model-name", base, "--sequence_length", "256", "--output_path", pq,
                       "--task_type", task])
    csv = str(tmp_path / "pred.csv")
    extra = ["--num_labels", str(NL)] if task == "multi_label" else []
    lora_predict.main(["predict", "--checkpoint_dir", ad, "--data_dir", pq, "--output_file", csv, "--task_type", task,
                       "--batch_size", "16"] + extra)
    df = pd.read_csv(csv)
    cols = {"classification": ["probability_positive"], "regression": ["predicted_value"],
            "multi_label": [f"class_{i}" for i in range(NL)]}[task]
    assert list(df.columns) == cols and len(df) == 45
    # the HF class on the same ids: the same values
    ids, labels, _ = lora_predict.read_tokenized(pq)
    m = load_adapter(ad, task_type=task, num_labels=NL if task == "multi_label" else None)
    m.config.engine_options = {"f32_gemm_split": 1}
    m = m.to(DEV).eval()
    lg = torch.cat([m(input_ids=torch.from_numpy(ids[i:i + 16]).to(DEV)).logits.cpu() for i in range(0, 45, 16)])
    if task == "classification":
        want = torch.softmax(lg, 1)[:, 1].numpy()[:, None]
    elif task == "regression":
        want = lg.numpy()
    else:
        want = torch.sigmoid(lg).numpy()
    np.testing.assert_allclose(df[cols].to_numpy(), want, rtol=1e-6, atol=1e-7)
    res = lora_predict.evaluate(ad, pq, task_type=task, num_labels=NL if task == "multi_label" else None, batch_size=16)
    keys = {"classification": ["accuracy", "f1", "roc_auc", "average_precision", "balance"],
            "regression": ["mse", "rmse", "mae", "r2", "pearson_r", "spearman_r"],
            "multi_label": ["accuracy", "f1", "roc_auc", "average_precision"]}[task]
    assert list(res) == ["eval_loss"] + ["eval_" + k for k in keys] + ["eval_runtime", "eval_samples_per_second",
                                                                      "eval_steps_per_second"]
    assert all(np.isfinite(res[k]) for k in res)
    if task == "multi_label":
        # the reference's documented command line, under a one-rank torchrun (process group over RCCL, rank 0 writes)
        csv2 = str(tmp_path / "pred2.csv")
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
        import socket
        s = socket.socket()
        s.bind(("127.0.0.1", 0))
        port = s.getsockname()[1]
        s.close()
        r = subprocess.run([sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=1", "--master-addr",
                            "127.0.0.1", "--master-port", str(port), "-m", "plantcaduceus_amd.lora_predict", "predict",
                            "--checkpoint-dir", ad, "--data-dir", pq, "--output-file", csv2, "--task-type", "multi_label",
                            "--num-labels", str(NL), "--batch-size", "16"], cwd=ROOT, env=env, capture_output=True, text=True,
                           timeout=300)
        assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
        pd.testing.assert_frame_equal(pd.read_csv(csv2), df)


def test_real_adapter():
    """Runs only when PLANTCAD2_ADAPTER_DIR names a released adapter directory (its base resolvable from its
    base_model_name_or_path, or PLANTCAD2_BASE_DIR): prints whether its lora_B are zero (LoRA policy) and runs
    predict on a few windows."""
    ad = os.environ.get("PLANTCAD2_ADAPTER_DIR")
    if not ad:
        pytest.skip("PLANTCAD2_ADAPTER_DIR not set (released PlantCAD2 adapters are not available offline)")
    from plantcaduceus_amd.adapters import load_adapter
    task = os.environ.get("PLANTCAD2_ADAPTER_TASK", "classification")
    nl = int(os.environ.get("PLANTCAD2_ADAPTER_LABELS", "0")) or None
    m = load_adapter(ad, task_type=task, num_labels=nl, lora_deltas="ignore", base=os.environ.get("PLANTCAD2_BASE_DIR"))
    print(json.dumps({k: v for k, v in m.adapter_info.items() if k != "nonzero_lora_B"}),
          "lora_B all zero:", not m.adapter_info["nonzero_lora_B"])
    m.config.engine_options = {"f32_gemm_split": 1}
    m = m.to(DEV).eval()
    lg = m(input_ids=rand_ids(4, 8192, 0).to(DEV)).logits
    assert torch.isfinite(lg).all()
