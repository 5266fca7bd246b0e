"""-m gpu: `lora_predict train --train_lora 0` with PCAD_TRAIN_FEATURES=cache on the data and geometry of
tests/test_gpu_lora_train.py, restated here: toy geometry (n_layer 2, d_model 64, d_inner 128, dt_rank 4), 16 training and 8 validation
windows of L = 69, label = G+C fraction above the training median, batch 4, fp32, lr 1e-3 constant, seed 42; 20 steps with an evaluation
every 5; PCAD_TRAIN_FEATURE_BATCH=3, so that the last block of either set is short (16 = 5 x 3 + 1, 8 = 2 x 3 + 2).

  cache       the run's two caches are `torch.equal` to CaduceusForSequenceClassification's engine (`forward_pooled(block, ...,
              want_pooled=True)`, "f32_gemm_split" 1 as `predict` sets it) on the same blocks of 3
  counter     the engine saw exactly 16 + 8 windows by the end of the run - 80 training samples and four evaluations later; one engine
  step 0      logits from features against the trainable model's forward(input_ids) on the same windows: |d| <= 2 x 1e-4 x max |logit|
              (each side is held to 1e-4 of the oracle by DESIGN.md §4f)
  trajectory  the 20 step losses against the float64 CPU restatement of head-only AdamW on the cached features
              (tests/pooled_logits_ref.head_only_adamw): max relative difference <= 1e-5.  The bar is reasoned, not observed: both sides
              start from the same fp32 features and weights; an fp32 dot product over D = 64 is off by at most 64 x 2^-24 = 3.8e-6 of its
              terms' magnitude, |d loss / d logit| <= 1 and the losses are 0.5 .. 0.7, so a step loss is within ~1e-5 before the optimizer's
              own fp32 roundings (a few 2^-24 per element and step over 20 steps) are counted.  last / first below 0.9,
              tests/test_gpu_lora_train.py's criterion for the GPU run.  The plain `--train_lora 0` run's final loss is printed beside it.
  output      every saved lora_B is exactly zero; `predict` loads output_dir under `auto` and its logits are within
              2 x 1e-4 x max |logit| of the run's last evaluation logits
  resume      --max_steps 6, and again from checkpoint-3: adapter_model.safetensors bit-equal, log entries equal from step 4 on
  world 2     accumulation 2 in one process against world 2 over gloo, accumulation 1 (tests/_feature_train_worker.py): adapters
              bit-equal, evaluation entries equal, only rank 0 wrote, and the two ranks' engines saw 24 windows between them
  bf16        --bf16 true, 6 steps: finite fp32 score, the adapter loads
  unset       without the variable `train` constructs no Engine
Every case prints its figures before it asserts.

Observed on an MI355X: see DESIGN.md §4x."""
import json
import os
import socket
import subprocess
import sys

import numpy as np
import pytest
import torch

import _feature_train_worker as W
import pooled_logits_ref as PL
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_feature_train_worker.py")
DEV = "cuda:0"
F32 = torch.float32
N_TRAIN, N_VALID, L, BATCH, LR, SEED, FB = 16, 8, 69, 4, 1e-3, 42, 3
A, C, G, T = 3, 4, 5, 6                # CaduceusTokenizer's ids of the four bases
ENV, FB_ENV = "PCAD_TRAIN_FEATURES", "PCAD_TRAIN_FEATURE_BATCH"


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def trunk_state():
    return synthetic_state_dict(toy_config(), seed=SEED, stress=False)


def windows():
    g = np.random.default_rng(11)

    def draw(n):
        gc = g.uniform(0.15, 0.85, size=n)
        is_gc = g.random((n, L)) < gc[:, None]
        first = g.random((n, L)) < 0.5
        return np.where(is_gc, np.where(first, C, G), np.where(first, A, T)).astype(np.int32)
    tr, va = draw(N_TRAIN), draw(N_VALID)
    frac = lambda x: ((x == C) | (x == G)).mean(1)
    cut = float(np.median(frac(tr)))
    return tr, (frac(tr) > cut).astype(np.int64), va, (frac(va) > cut).astype(np.int64)


def write_inputs(tmp):
    import pyarrow as pa
    import pyarrow.parquet as pq
    tr, ytr, va, yva = windows()
    for name, x, y in (("train", tr, ytr), ("valid", va, yva)):
        pq.write_table(pa.table({"input_ids": pa.array(list(x), type=pa.list_(pa.int32())), "label": pa.array(y)}), str(tmp / f"{name}.parquet"))
    save_checkpoint(str(tmp / "base"), toy_config(), trunk_state())


def arguments(tmp, out, *extra, steps=6, every=3, accumulation=1):
    return ["--train_dir", str(tmp / "train.parquet"), "--valid_dir", str(tmp / "valid.parquet"), "--model_name", str(tmp / "base"),
            "--output_dir", str(out), "--train_batch_size", str(BATCH), "--eval_batch_size", "4", "--gradient_accumulation_steps", str(accumulation),
            "--learning_rate", str(LR), "--lr_scheduler_type", "constant", "--warmup_steps", "0", "--max_steps", str(steps),
            "--logging_steps", "1", "--eval_steps", str(every), "--save_steps", str(every), "--seed", str(SEED), "--device", DEV,
            "--train_lora", "0", *extra]


def command(tmp, out, *extra, **kw):
    """the command in this process with the worker's counters around it -> the counts"""
    from plantcaduceus_amd import lora_predict
    counts = {"engines": 0, "windows": 0, "writes": 0}
    undo = W.counted(counts)
    try:
        lora_predict.main(["train"] + arguments(tmp, out, *extra, **kw))
    finally:
        undo()
    return counts


def history(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return json.load(f)["log_history"]


def losses(hist):
    return np.array([e["loss"] for e in hist if "loss" in e], dtype=np.float64)


def frozen_model(dtype=F32):
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    m = TrainableCaduceusForSequenceClassification(toy_config(), 2, "single_label_classification", device=DEV, seed=SEED, train_lora=False, dtype=dtype)
    m.load_trunk({k: v for k, v in trunk_state().items() if k.startswith("caduceus.")})
    return m


@pytest.fixture()
def cached(monkeypatch):
    monkeypatch.setenv(ENV, "cache")
    monkeypatch.setenv(FB_ENV, str(FB))


@pytest.fixture(scope="module")
def run20(tmp_path_factory):
    """the 20-step run on cached features, once: -> dict(tmp, out, counts, caches [train, valid], eval_logits [one per evaluation])"""
    from plantcaduceus_amd import lora_predict
    tmp = tmp_path_factory.mktemp("feature_train")
    write_inputs(tmp)
    caches, evals = [], []
    mp = pytest.MonkeyPatch()
    mp.setenv(ENV, "cache")
    mp.setenv(FB_ENV, str(FB))
    cache_features, eval_logits = lora_predict.cache_features, lora_predict.FeatureTrainer.eval_logits
    mp.setattr(lora_predict, "cache_features", lambda *a, **k: (caches.append(cache_features(*a, **k)), caches[-1])[1])
    mp.setattr(lora_predict.FeatureTrainer, "eval_logits", lambda self: (evals.append(eval_logits(self)), evals[-1])[1])
    try:
        counts = command(tmp, tmp / "run", steps=20, every=5)
    finally:
        mp.undo()
    return dict(tmp=tmp, out=tmp / "run", counts=counts, caches=caches, eval_logits=evals)


def test_cache_is_the_inference_engines_pooled_vectors(run20):
    from plantcaduceus_amd.modeling_caduceus import CaduceusForSequenceClassification
    tr, _, va, _ = windows()
    model = CaduceusForSequenceClassification.from_pretrained(str(run20["tmp"] / "base"), num_labels=2, problem_type="single_label_classification",
                                                              torch_dtype=F32)
    model.config.engine_options = {"f32_gemm_split": 1}
    eng = model.to(DEV).eval()._engine()
    assert len(run20["caches"]) == 2
    for name, ids, cache in (("train", tr, run20["caches"][0]), ("valid", va, run20["caches"][1])):
        t = torch.from_numpy(ids).to(DEV)
        want = torch.cat([eng.forward_pooled(t[b0:b0 + FB], "mean", model.score.weight, want_pooled=True)[1] for b0 in range(0, len(ids), FB)])
        print(f"{name} cache {tuple(cache.shape)} {cache.dtype} on {cache.device}: max |d| {(cache - want).abs().max().item():.3e}, "
              f"max |feature| {want.abs().max().item():.3f}")
        assert cache.shape == (len(ids), 2, 64) and cache.dtype == F32 and cache.is_cuda and torch.equal(cache, want)


def test_the_trunk_ran_once_per_window(run20):
    """80 training samples and four evaluations later the engine has seen 16 + 8 windows: without the feature this cannot hold"""
    with open(run20["out"] / "train_results.json") as f:
        res = json.load(f)
    hist = history(run20["out"])
    print(f"engine windows {run20['counts']['windows']}, engines {run20['counts']['engines']}; train_results feature_windows "
          f"{res.get('feature_windows')}, feature_pass_runtime {res.get('feature_pass_runtime')}")
    assert [e["step"] for e in hist if "eval_loss" in e] == [5, 10, 15, 20] and len(losses(hist)) == 20 and len(run20["eval_logits"]) == 4
    assert run20["counts"]["windows"] == N_TRAIN + N_VALID and run20["counts"]["engines"] == 1
    assert res["feature_windows"] == N_TRAIN + N_VALID and res["feature_pass_runtime"] > 0 and res["train_samples"] == N_TRAIN


def test_step0_logits_from_features_against_the_trainable_forward():
    tr, _, _, _ = windows()
    model = frozen_model()
    model.feature_engine({"f32_gemm_split": 1})
    ids = torch.from_numpy(tr).to(DEV)
    with torch.no_grad():
        plain = model(ids).logits
        feats = model.pooled_features(ids)
        got = model(pooled=feats).logits
    top, d = plain.abs().max().item(), (got - plain).abs().max().item()
    print(f"step-0 logits from features vs forward(input_ids): max |d logit| {d:.3e} [bar {2e-4 * top:.3e}, max |logit| {top:.3f}]")
    assert model.feature_windows == N_TRAIN and got.shape == plain.shape == (N_TRAIN, 2)
    assert d <= 2 * 1e-4 * top
    with pytest.raises(ValueError, match="exactly one"):
        model(ids, pooled=feats)
    with pytest.raises(ValueError, match="exactly one"):
        model()


def test_feature_engine_needs_frozen_factors():
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    m = TrainableCaduceusForSequenceClassification(toy_config(), 2, "single_label_classification", device=DEV, seed=SEED)
    with pytest.raises(ValueError, match="train_lora"):
        m.feature_engine()
    with pytest.raises(ValueError, match="train_lora"):
        m.pooled_features(torch.zeros((1, L), dtype=torch.int32, device=DEV))


def test_trajectory_against_float64_head_only_adamw(run20, monkeypatch):
    from plantcaduceus_amd import pretrain
    _, ytr, _, _ = windows()
    got = losses(history(run20["out"]))
    order = pretrain.WindowOrder(N_TRAIN, BATCH, 1, SEED)
    ref = np.array(PL.head_only_adamw(run20["caches"][0].cpu(), torch.from_numpy(ytr), [order.windows(s)[0] for s in range(20)],
                                      frozen_model().score.weight.detach().cpu(), LR))
    monkeypatch.delenv(ENV, raising=False)
    command(run20["tmp"], run20["tmp"] / "plain", steps=20, every=5)
    plain = losses(history(run20["tmp"] / "plain"))
    diff = float(np.max(np.abs(got - ref) / np.abs(ref)))
    print("cached  " + " ".join(f"{x:.6f}" for x in got))
    print("float64 " + " ".join(f"{x:.6f}" for x in ref))
    print("plain   " + " ".join(f"{x:.6f}" for x in plain))
    print(f"max relative difference cached vs float64 restatement {diff:.3e} [1e-5]; last / first cached {got[-1] / got[0]:.3f} [0.9], "
          f"float64 {ref[-1] / ref[0]:.3f}; final loss cached {got[-1]:.6f}, plain --train_lora 0 {plain[-1]:.6f} "
          f"(relative difference {abs(got[-1] - plain[-1]) / abs(plain[-1]):.3e}, recorded, not asserted)")
    assert len(got) == len(ref) == 20 and np.isfinite(got).all()
    assert diff <= 1e-5
    assert got[-1] < 0.9 * got[0]


def test_output_has_zero_factors_and_predict_loads_it(run20):
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict
    _, _, va, _ = windows()
    sd = load_file(str(run20["out"] / "adapter_model.safetensors"))
    assert sum(".lora_B." in k for k in sd) == 12 and all(not v.any() for k, v in sd.items() if ".lora_B." in k)
    eng = lora_predict.load_model(str(run20["out"]), "classification", None, None, DEV, "float32", "mean", "auto")
    got = lora_predict.predict_logits(eng, va, DEV, 4)
    want = run20["eval_logits"][-1]
    top, d = float(np.abs(want).max()), float(np.abs(got - want).max())
    print(f"predict (auto) vs the run's last evaluation logits: max |d logit| {d:.3e} [bar {2e-4 * top:.3e}, max |logit| {top:.3f}]")
    assert got.shape == want.shape == (N_VALID, 2) and d <= 2 * 1e-4 * top


def test_resume_from_checkpoint_is_bit_equal(tmp_path, cached):
    from safetensors.torch import load_file
    write_inputs(tmp_path)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    command(tmp_path, a)
    counts = command(tmp_path, b, "--resume_from_checkpoint", str(a / "checkpoint-3"))
    wa, wb = load_file(str(a / "adapter_model.safetensors")), load_file(str(b / "adapter_model.safetensors"))
    ha, hb = history(a), history(b)
    print(f"resume: losses straight {[round(x, 6) for x in losses(ha)]} resumed {[round(x, 6) for x in losses(hb)[3:]]}; the resumed run's "
          f"engine saw {counts['windows']} windows")
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    strip = lambda h: [{k: v for k, v in e.items() if k != "eval_runtime"} for e in h]
    at = next(i for i, e in enumerate(ha) if e["step"] == 4)
    assert [e["step"] for e in ha if "loss" in e] == [1, 2, 3, 4, 5, 6] and strip(ha[at:]) == strip(hb[at:])
    assert counts["windows"] == N_TRAIN + N_VALID               # the pass is run again: the cache is not persisted


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_gloo_against_accumulation_2(tmp_path, cached):
    from safetensors.torch import load_file
    write_inputs(tmp_path)
    one, two, side = tmp_path / "one", tmp_path / "two", tmp_path / "side"
    os.makedirs(side)
    command(tmp_path, one, steps=4, every=2, accumulation=2)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PCAD_DDP_BACKEND="gloo", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, str(side)] + arguments(tmp_path, two, steps=4, every=2, accumulation=1)
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [json.load(open(side / f"r{k}.json")) for k in range(2)]
    wa, wb = load_file(str(one / "adapter_model.safetensors")), load_file(str(two / "adapter_model.safetensors"))
    strip = lambda h: [{k: v for k, v in e.items() if k != "eval_runtime"} for e in h]
    ea, eb = [e for e in strip(history(one)) if "eval_loss" in e], [e for e in strip(history(two)) if "eval_loss" in e]
    print(f"world 2: per-rank counts {ranks}; losses one process {[round(x, 6) for x in losses(history(one))]} world 2 "
          f"{[round(x, 6) for x in losses(history(two))]}")
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert len(ea) == 2 and ea == eb
    assert ranks[0]["writes"] > 0 and ranks[1]["writes"] == 0
    # blocks of 3 dealt in contiguous runs: 6 + 3 blocks = rank 0 runs 3 + 2 blocks (9 + 6 windows), rank 1 the rest (7 + 2)
    assert [q["windows"] for q in ranks] == [15, 9] and all(q["engines"] == 1 for q in ranks)


def test_bf16(tmp_path, cached):
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict
    write_inputs(tmp_path)
    out = tmp_path / "bf16"
    counts = command(tmp_path, out, "--bf16", "true")
    sd = load_file(str(out / "adapter_model.safetensors"))
    h = losses(history(out))
    print(f"--bf16 true losses {[round(x, 5) for x in h]}")
    score = sd["base_model.model.score.weight"]
    assert score.dtype == F32 and bool(torch.isfinite(score).all()) and np.isfinite(h).all() and len(h) == 6
    assert counts["windows"] == N_TRAIN + N_VALID
    eng = lora_predict.load_model(str(out), "classification", None, None, DEV, "bfloat16", "mean", "auto")
    assert np.isfinite(lora_predict.predict_logits(eng, windows()[2], DEV, 4)).all()


def test_variable_unset_builds_no_engine(tmp_path, monkeypatch):
    monkeypatch.delenv(ENV, raising=False)
    write_inputs(tmp_path)
    out = tmp_path / "plain"
    counts = command(tmp_path, out, steps=3)
    with open(out / "train_results.json") as f:
        res = json.load(f)
    assert counts["engines"] == 0 and counts["windows"] == 0 and counts["writes"] > 0
    assert "feature_windows" not in res and "feature_pass_runtime" not in res and len(losses(history(out))) == 3


def test_budget_guard_and_refusals(tmp_path, cached):
    write_inputs(tmp_path)
    with pytest.raises(SystemExit, match=ENV) as e:                  # 1 step x 4 x 1 x 1 = 4 scheduled samples < 16 / 2
        command(tmp_path, tmp_path / "refused", steps=1)
    assert "4" in str(e.value) and "16" in str(e.value)
    counts = command(tmp_path, tmp_path / "boundary", steps=2, every=2)           # 8 = 16 / 2: runs
    assert counts["windows"] == N_TRAIN + N_VALID
    with pytest.raises(SystemExit, match="pooling"):
        command(tmp_path, tmp_path / "refused", "--pooling", "max")
