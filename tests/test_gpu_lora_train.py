"""-m gpu: the `lora_predict train` command on the toy geometry of tests/test_gpu_training_model.py (n_layer 2, d_model 64,
d_inner 128, dt_rank 4): a base snapshot from checkpoint.synthetic_state_dict(stress=False), 16 training and 8 validation windows of
L = 69 in parquet files, batch 4, fp32, lr 1e-3, constant schedule.  The windows' G+C content is drawn per window from U(0.15, 0.85) and
the label is "G+C fraction above the training median": a reverse-complement-invariant property, which the RC-invariant head can learn
(a strand-dependent label could not be).

  trajectory    20 step losses under optim.AdamW against the same loop under torch.optim.AdamW(foreach=False) + clip_grad_norm_ on the
                same model: max relative difference within 10 x the distance of torch's own foreach=False and foreach=True trajectories,
                floored at 1e-6 (tests/test_gpu_pretrain.py's twin comparison); output_dir loads through `predict --lora-deltas apply`
                with logits within 2 x 1e-4 x max |logit| of the trainable model's; `evaluate` returns every eval_* key
  learning      the float64 CPU restatement of the same 20 steps (tests/pool_bwd_ref.py's graph + optim_ref.adamw_step) ends below 0.8 x its
                first loss - the inputs were chosen so that the reference alone meets this with room -, and the GPU run ends below 0.9 x
  resume        to --max_steps 6, and again from checkpoint-3: adapter_model.safetensors bit-equal, log histories equal from step 4 on
  options       --train_lora 0: every saved lora_B is zero and `predict` loads it under `auto`; --bf16 true, 6 steps: finite parameters,
                the adapter loads; --lora_dropout 0.1 and --pooling max exit naming the flag
Every case prints its figures before it asserts.

Observed on an MI355X.  Step losses, float64 CPU restatement:
  0.667475 0.552543 0.863166 0.620080 0.540815 0.361620 0.428445 0.404229 0.273116 0.380798
  0.144832 0.324581 0.111299 0.275740 0.258429 0.262176 0.263644 0.276088 0.151195 0.066300      (last / first 0.099 [0.8])
the command on the GPU: the same to six digits except the last two, 0.151196 0.066301 (last / first 0.099 [0.9]; 7.4e-7 relative from
the restatement at worst); command against torch.optim.AdamW(foreach=False) 1.1e-7 relative at worst [bar 2.1e-6: torch's two forms differ
by 2.1e-7 themselves]; the loaded output against the trainable model max |d logit| 9.8e-7 [5.1e-4, max |logit| 2.56]; resume bit-equal;
--train_lora 0 losses 0.66748 -> 0.60901 and --bf16 true 0.6677 -> 0.36228 over 6 steps."""
import json
import os

import numpy as np
import pytest
import torch

import optim_ref as OR
import pool_bwd_ref as PB
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
N_TRAIN, N_VALID, L, BATCH, LR, SEED = 16, 8, 69, 4, 1e-3, 42
A, C, G, T = 3, 4, 5, 6                # CaduceusTokenizer's ids of the four bases (complement: 3 <-> 6, 4 <-> 5)


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def trunk_state():
    return synthetic_state_dict(toy_config(), seed=SEED, stress=False)


def windows():
    """-> (train ids [16, L], train labels [16], valid ids [8, L], valid labels [8]); the label is RC-invariant: G+C fraction above the
    training windows' median"""
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
    assert ytr.sum() == N_TRAIN // 2 and 0 < yva.sum() < N_VALID
    for name, x, y in (("train", tr, ytr), ("valid", va, yva)):
        pq.write_table(pa.table({"input_ids": pa.array(list(x), type=pa.list_(pa.int32())), "label": pa.array(y)}), str(tmp / f"{name}.parquet"))
    base = tmp / "base"
    save_checkpoint(str(base), toy_config(), trunk_state())
    return str(tmp / "train.parquet"), str(tmp / "valid.parquet"), str(base)


def command(tmp, out, *extra, steps=6):
    from plantcaduceus_amd import lora_predict
    train, valid, base = (str(tmp / "train.parquet"), str(tmp / "valid.parquet"), str(tmp / "base"))
    return lora_predict.main(["train", "--train_dir", train, "--valid_dir", valid, "--model_name", base, "--output_dir", str(out),
                              "--train_batch_size", str(BATCH), "--eval_batch_size", "4", "--gradient_accumulation_steps", "1",
                              "--learning_rate", str(LR), "--lr_scheduler_type", "constant", "--warmup_steps", "0", "--max_steps", str(steps),
                              "--logging_steps", "1", "--eval_steps", "3", "--save_steps", "3", "--seed", str(SEED), "--device", DEV, *extra])


def history(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return json.load(f)["log_history"]


def losses(hist):
    return np.array([e["loss"] for e in hist if "loss" in e], dtype=np.float64)


def fresh_model():
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    m = TrainableCaduceusForSequenceClassification(toy_config(), 2, "single_label_classification", device=DEV, seed=SEED)
    m.load_trunk({k: v for k, v in trunk_state().items() if k.startswith("caduceus.")})
    return m


class TorchOptimizer:
    """clip_grad_norm_ + torch.optim.AdamW behind optim.AdamW's interface, with its decay rule (tests/test_gpu_pretrain.py's twin)"""

    def __init__(self, model, foreach, lr, weight_decay, max_norm=1.0):
        from plantcaduceus_amd import optim
        named = [(k, p) for k, p in model.named_parameters() if p.requires_grad]
        self.params = [p for _, p in named]
        self.opt = OR.torch_adamw(self.params, [optim.applies_weight_decay(k, p) for k, p in named], lr, 0.9, 0.999, 1e-8, weight_decay, foreach=foreach)
        self.foreach, self.max_norm, self.grad_scale, self.norm = foreach, max_norm, 1.0, None

    def step(self, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr
        self.norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, foreach=self.foreach)
        self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad(set_to_none=False)

    def state(self):
        return {"norm": float(self.norm), "coef": float("nan"), "finite": 1, "skipped": 0}


def run_loop(which, steps=20):
    """the command's own loop (lora_predict.FinetuneTrainer) on a fresh model under the named optimizer; -> (step losses, model)"""
    from types import SimpleNamespace
    from plantcaduceus_amd import lora_predict, optim
    tr, ytr, _, _ = windows()
    model = fresh_model()
    src = lora_predict.LabelledBatches(tr, ytr, BATCH, 1, SEED)
    opt = optim.AdamW(model.named_parameters(), lr=LR, weight_decay=0.01) if which == "fused" else TorchOptimizer(model, which == "foreach", LR, 0.01)
    a = SimpleNamespace(output_dir=None, model_name=None, task_type="classification", device=DEV, learning_rate=LR, lr_scheduler_type="constant",
                        warmup_steps=0, eval_batch_size=4, eval_strategy="no", eval_steps=0, save_strategy="no", save_steps=0, logging_steps=1)
    t = lora_predict.FinetuneTrainer(model, opt, src, a, steps)
    t.run()
    return losses(t.log_history), model


def cpu_reference_trajectory(steps=20):
    """the same 20 steps in float64 on the CPU: the graph of tests/pool_bwd_ref.py, clip_grad_norm_(1.0) and AdamW (weight decay 0.01 on
    every trainable tensor, as optim.applies_weight_decay decides for factors and score) through optim_ref.adamw_step"""
    from plantcaduceus_amd import pretrain
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    cfg, sd = toy_config(), trunk_state()
    tr, ytr, _, _ = windows()
    init = TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", device="cpu", seed=SEED)
    names = [k for k, p in init.named_parameters() if p.requires_grad]
    p = [dict(init.named_parameters())[k].detach().double().clone() for k in names]
    m, v = [torch.zeros_like(t) for t in p], [torch.zeros_like(t) for t in p]
    order = pretrain.WindowOrder(N_TRAIN, BATCH, 1, SEED)
    out = []
    for step in range(steps):
        idx = order.windows(step)[0]
        lv = {k: t.clone().requires_grad_(True) for k, t in zip(names, p)}
        loss, _ = PB.model_forward(lv, sd, cfg, torch.from_numpy(tr[idx].copy()), torch.from_numpy(ytr[idx].copy()), "single_label_classification")
        loss.backward()
        OR.adamw_step(p, [lv[k].grad for k in names], m, v, [True] * len(p), LR, 0.9, 0.999, 1e-8, 0.01, step + 1, max_norm=1.0)
        out.append(loss.item())
    return np.array(out)


def test_trajectory_learning_and_the_output_loads(tmp_path):
    from plantcaduceus_amd import lora_predict
    train, valid, base = write_inputs(tmp_path)
    out = tmp_path / "run"
    command(tmp_path, out, steps=20)
    fused = losses(history(out))
    single, _ = run_loop("single")
    foreach, _ = run_loop("foreach")
    ref = cpu_reference_trajectory()
    assert len(fused) == len(single) == len(foreach) == len(ref) == 20 and np.isfinite(fused).all()
    noise = float(np.max(np.abs(single - foreach) / np.abs(single)))
    diff = float(np.max(np.abs(fused - single) / np.abs(single)))
    bar = max(10 * noise, 1e-6)
    print("command " + " ".join(f"{x:.6f}" for x in fused))
    print("torch   " + " ".join(f"{x:.6f}" for x in single))
    print("float64 " + " ".join(f"{x:.6f}" for x in ref))
    print(f"max relative difference command vs torch foreach=False {diff:.3e} [bar {bar:.3e}; torch foreach=False vs foreach=True {noise:.3e}]; "
          f"command vs float64 restatement {float(np.max(np.abs(fused - ref) / np.abs(ref))):.3e}")
    assert diff <= bar
    # learning: the reference alone meets 0.8 with room; the GPU run is held to 0.9
    print(f"last / first loss: float64 restatement {ref[-1] / ref[0]:.3f} [0.8], command {fused[-1] / fused[0]:.3f} [0.9]")
    assert ref[-1] < 0.8 * ref[0]
    assert fused[-1] < 0.9 * fused[0]
    # the output loads, and computes what the trainable model computes
    _, _, va, yva = windows()
    eng = lora_predict.load_model(str(out), "classification", None, None, DEV, "float32", "mean", "apply")
    got = lora_predict.predict_logits(eng, va, DEV, 4)
    model = fresh_model()
    model.load_adapter_weights(str(out))
    want = lora_predict.predict_logits_trainable(model, va, DEV, 4)
    top = float(np.abs(got).max())
    print(f"output loads: max |d logit| {float(np.abs(got - want).max()):.3e} [bar {2e-4 * top:.3e}, max |logit| {top:.3f}]")
    assert eng.adapter_info["merged_pairs"] == 12 and float(np.abs(got - want).max()) <= 2 * 1e-4 * top
    df = lora_predict.predict(str(out), valid, output_file=str(tmp_path / "pred.csv"), device=DEV, lora_deltas="apply")
    assert len(df) == N_VALID and os.path.exists(tmp_path / "pred.csv")
    res = lora_predict.evaluate(str(out), valid, device=DEV, batch_size=4, lora_deltas="apply")
    keys = {"eval_loss", "eval_accuracy", "eval_f1", "eval_roc_auc", "eval_average_precision", "eval_balance", "eval_runtime",
            "eval_samples_per_second", "eval_steps_per_second"}
    assert keys <= set(res) and np.isfinite(res["eval_loss"])
    # the command's own evaluations, every eval_steps = 3 steps, in the log history
    evals = [e for e in history(out) if "eval_loss" in e]
    assert [e["step"] for e in evals] == [3, 6, 9, 12, 15, 18] and all({"eval_accuracy", "eval_roc_auc"} <= set(e) for e in evals)
    # save_total_limit 5: of the checkpoints at 3, 6, .. 18 the oldest is gone
    assert sorted(d for d in os.listdir(out) if d.startswith("checkpoint-")) == sorted(f"checkpoint-{k}" for k in (6, 9, 12, 15, 18))
    for f in ("adapter_config.json", "adapter_model.safetensors", "trainer_state.json", "train_results.json"):
        assert os.path.exists(out / f), f


def test_resume_from_checkpoint_is_bit_equal(tmp_path):
    from safetensors.torch import load_file
    write_inputs(tmp_path)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    command(tmp_path, a)
    for f in ("optimizer.pt", "trainer_state.json", "adapter_model.safetensors", "adapter_config.json"):
        assert os.path.exists(a / "checkpoint-3" / f), f
    assert os.path.isdir(a / "checkpoint-6")
    command(tmp_path, b, "--resume_from_checkpoint", str(a / "checkpoint-3"))
    wa, wb = load_file(str(a / "adapter_model.safetensors")), load_file(str(b / "adapter_model.safetensors"))
    worst = max((wa[k].double() - wb[k].double()).abs().max().item() for k in wa)
    ha, hb = history(a), history(b)
    print(f"resume: max |d parameter| {worst:.3e}; losses straight {[round(x, 6) for x in losses(ha)]} resumed {[round(x, 6) for x in losses(hb)[3:]]}")
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    strip = lambda h: [{k: v for k, v in e.items() if k != "eval_runtime"} for e in h]
    at = next(i for i, e in enumerate(ha) if e["step"] == 4)
    assert [e["step"] for e in ha if "loss" in e] == [1, 2, 3, 4, 5, 6] and strip(ha[at:]) == strip(hb[at:]) and strip(hb[:at]) == strip(ha[:at])


def test_options(tmp_path):
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict
    _, valid, _ = write_inputs(tmp_path)
    # the frozen-trunk mode
    out = tmp_path / "frozen"
    command(tmp_path, out, "--train_lora", "0")
    sd = load_file(str(out / "adapter_model.safetensors"))
    assert all(not v.any() for k, v in sd.items() if ".lora_B." in k) and sum(".lora_B." in k for k in sd) == 12
    df = lora_predict.predict(str(out), valid, output_file=str(tmp_path / "frozen.csv"), device=DEV)          # lora_deltas="auto"
    assert len(df) == N_VALID and np.isfinite(df["probability_positive"].to_numpy()).all()
    h = losses(history(out))
    print(f"--train_lora 0 losses {[round(x, 5) for x in h]}")
    # the bf16 form
    out = tmp_path / "bf16"
    command(tmp_path, out, "--bf16", "true")
    sd = load_file(str(out / "adapter_model.safetensors"))
    h = losses(history(out))
    print(f"--bf16 true losses {[round(x, 5) for x in h]}")
    assert all(v.dtype == F32 and bool(torch.isfinite(v).all()) for v in sd.values()) and np.isfinite(h).all() and len(h) == 6
    assert any(v.any() for k, v in sd.items() if ".lora_B." in k)
    eng = lora_predict.load_model(str(out), "classification", None, None, DEV, "bfloat16", "mean", "apply")
    assert np.isfinite(lora_predict.predict_logits(eng, windows()[2], DEV, 4)).all()
    # refusals name the flag
    for flags, word in ((["--lora_dropout", "0.1"], "lora_dropout"), (["--pooling", "max"], "pooling")):
        with pytest.raises(SystemExit, match=word):
            command(tmp_path, tmp_path / "refused", *flags)
