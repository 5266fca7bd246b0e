"""-m gpu: `lora_predict train` with PCAD_LORA_DROPOUT=0.1 on the data recipe of tests/test_gpu_lora_train.py, restated
here: toy geometry (n_layer 2, d_model 64, d_inner 128, dt_rank 4), 16 training and 8 validation windows of L = 69, label = G+C fraction
above the training median, batch 4, fp32, lr 1e-3 constant, seed 42.

  run        6 steps: finite losses; a trajectory that differs from the run without the variable (from step 2 on: at step 1 lora_B is
             zero and the branch contributes exact zeros); adapter_config.json carries 0.1; the output loads through
             `predict --lora-deltas apply`
  resume     again from checkpoint-3: adapter_model.safetensors bit-equal - the masks are a function of (seed, step), there is no
             generator state to restore
  refusals   --train_lora 0 with the variable set exits naming both; a malformed value exits naming the variable
  world 2    tests/_lora_dropout_ddp_worker.py: one train_step at world 2 over gloo, accumulation 1, against one process with
             accumulation 2: per tensor |d flat| <= 3e-4 max |g| (§4r's bar, 2 (2 n_layer + 1) 3e-5); both draw the masks of
             micro-batches 2 n + 0 and 2 n + 1
Every case prints its figures before it asserts."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _lora_dropout_ddp_worker as W
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_lora_dropout_ddp_worker.py")
DEV = "cuda:0"
N_TRAIN, N_VALID, L, BATCH, LR, SEED = 16, 8, 69, 4, 1e-3, 42
A, C, G, T = 3, 4, 5, 6                # CaduceusTokenizer's ids of the four bases
ENV = "PCAD_LORA_DROPOUT"


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


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
    save_checkpoint(str(tmp / "base"), toy_config(), synthetic_state_dict(toy_config(), seed=SEED, stress=False))
    return str(tmp / "valid.parquet")


def command(tmp, out, *extra, steps=6):
    from plantcaduceus_amd import lora_predict
    return lora_predict.main(["train", "--train_dir", str(tmp / "train.parquet"), "--valid_dir", str(tmp / "valid.parquet"), "--model_name",
                              str(tmp / "base"), "--output_dir", str(out), "--train_batch_size", str(BATCH), "--eval_batch_size", "4",
                              "--gradient_accumulation_steps", "1", "--learning_rate", str(LR), "--lr_scheduler_type", "constant",
                              "--warmup_steps", "0", "--max_steps", str(steps), "--logging_steps", "1", "--eval_steps", "3", "--save_steps", "3",
                              "--seed", str(SEED), "--device", DEV, *extra])


def losses(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return np.array([e["loss"] for e in json.load(f)["log_history"] if "loss" in e], dtype=np.float64)


def test_run_resume_and_the_output_loads(tmp_path, monkeypatch):
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict
    valid = write_inputs(tmp_path)
    monkeypatch.delenv(ENV, raising=False)
    plain = tmp_path / "plain"
    command(tmp_path, plain)
    monkeypatch.setenv(ENV, "0.1")
    a, b = tmp_path / "dropout", tmp_path / "resumed"
    command(tmp_path, a)
    command(tmp_path, b, "--resume_from_checkpoint", str(a / "checkpoint-3"))
    monkeypatch.delenv(ENV)
    lp, la, lb = losses(plain), losses(a), losses(b)
    print("without " + " ".join(f"{x:.6f}" for x in lp))
    print("p = 0.1 " + " ".join(f"{x:.6f}" for x in la))
    print("resumed " + " ".join(f"{x:.6f}" for x in lb))
    assert len(la) == len(lp) == 6 and np.isfinite(la).all()
    assert la[0] == lp[0] and all(la[1:] != lp[1:])                               # lora_B = 0 at step 1: the branch is exact zeros
    for out, want in ((plain, 0.0), (a, 0.1), (a / "checkpoint-3", 0.1), (b, 0.1)):
        with open(out / "adapter_config.json") as f:
            assert json.load(f)["lora_dropout"] == want, out
    wa, wb = load_file(str(a / "adapter_model.safetensors")), load_file(str(b / "adapter_model.safetensors"))
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert np.array_equal(la[3:], lb[3:])
    assert any(bool(v.any()) for k, v in wa.items() if ".lora_B." in k)
    df = lora_predict.predict(str(a), valid, output_file=str(tmp_path / "pred.csv"), device=DEV, lora_deltas="apply")
    assert len(df) == N_VALID and np.isfinite(df["probability_positive"].to_numpy()).all()


def test_refusals(tmp_path, monkeypatch):
    write_inputs(tmp_path)
    monkeypatch.setenv(ENV, "0.1")
    with pytest.raises(SystemExit) as e:
        command(tmp_path, tmp_path / "refused", "--train_lora", "0")
    assert ENV in str(e.value) and "--train_lora 0" in str(e.value)
    monkeypatch.setenv(ENV, "1.0")
    with pytest.raises(SystemExit, match=ENV):
        command(tmp_path, tmp_path / "refused")
    assert not os.path.exists(tmp_path / "refused")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_world2_gloo_one_step_against_accumulation_2(tmp_path):
    import scan_ref as R
    one_dir, two_dir = tmp_path / "one", tmp_path / "two"
    os.makedirs(one_dir), os.makedirs(two_dir)
    W.main([str(one_dir), "2"])
    one = torch.load(one_dir / "r0.pt", weights_only=False)
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node=2", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER, str(two_dir), "1"]
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    ranks = [torch.load(two_dir / f"r{k}.pt", weights_only=False) for k in range(2)]
    gbar = 2 * (2 * W.toy_config().n_layer + 1) * R.BAR_SCAN[False]
    assert abs(gbar - 3e-4) < 1e-12
    assert torch.equal(ranks[0]["flat"], ranks[1]["flat"]) and ranks[0]["names"] == one["names"] and ranks[0]["offsets"] == one["offsets"]
    # the one process ran micro-batches 2 n + 0 and 2 n + 1; rank k ran 2 n + k; forward advances the counter by one
    assert one["dropout_step"] == W.STEP * 2 + 2 and [q["dropout_step"] for q in ranks] == [W.STEP * 2 + 1, W.STEP * 2 + 2]
    worst = 0.0
    for name, o, n in zip(one["names"], one["offsets"], one["sizes"]):
        ga, gb = one["flat"][o:o + n].double(), ranks[0]["flat"][o:o + n].double()
        top, d = ga.abs().max().item(), (ga - gb).abs().max().item()
        worst = max(worst, d / top)
        assert top > 0 and d <= gbar * top, (name, d, top)
    print(f"world 2 vs accumulation 2 with dropout: worst |d flat| / max |g| {worst:.2e} [bar {gbar:.1e}]; losses {ranks[0]['loss']:.7f} {one['loss']:.7f}")
    assert abs(ranks[0]["loss"] - one["loss"]) <= 4 * 2.0 ** -24 * abs(one["loss"])
