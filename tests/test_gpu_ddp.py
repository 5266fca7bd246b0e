"""-m gpu: data-parallel training under torchrun (plantcaduceus_amd/ddp.py) on §4o's toy geometry (n_layer 2, d_model 64,
d_inner 128, dt_rank 4; 8 windows of L = 69, fp32 unless said).  W ranks x A accumulation steps are one process with A W accumulation
steps; every child is `python -m torch.distributed.run` with its own timeout, a test stops at the first child that exits non-zero, and
no test starts more than 4 ranks.  With gloo all ranks share the box's one device (RCCL refuses that).

  pretrain        6 steps, --save_steps 3, batch 2: (a) plain python, accumulation 2; (b) world 2 over gloo, accumulation 1; (c) world 2
                  resumed from (a)'s checkpoint-3; (d) world 1 over RCCL, accumulation 2 (the collective and the flat path on every box).
                  model.safetensors of all four bit-equal; checkpoint-3's model.safetensors and optimizer.pt tensors of (a) and (b)
                  bit-equal; log histories (loss, learning_rate, grad_norm, skipped_steps) equal; only rank 0 wrote
  lora train      4 steps (lora_B starts at zero: enough steps for both factors to move): world 2 over gloo, batch 2, accumulation 1
                  against one process with accumulation 2: adapter_model.safetensors bit-equal, eval_* entries equal
  world 4         tests/_ddp_worker.py: one Trainer.train_step at world 4 over gloo, accumulation 1, against one process with
                  accumulation 4.  Per tensor |d flat| <= 3e-4 max |g| - tests/test_gpu_pretrain.py's accumulation bar,
                  2 (2 n_layer + 1) 3e-5: two ways of summing the same gradients; the norm within optim_ref.norm_bar (1.61e-6) of
                  the float64 norm of the rank's own reduced buffer; all four ranks' flat and checksums bit-equal to each other
  inf             the same worker, an inf written into one gradient on rank 1 only: every rank reports finite 0, skipped 1, nothing changed
  bf16            world 2 over gloo, 4 steps: finite losses, the command's own checksum comparison passes at the checkpoint and the end
                  (it raises otherwise), parameters = rounded masters
  RCCL, W > 1     the bit-equality run at world 2 and the bar run at world 4, one device per rank.  They skip when fewer devices are
                  visible, as tests/test_gpu_dist.py's do - and have NOT run until a box shows that many devices.
Observed on an MI355X: world 4 against accumulation 4, worst |d flat| / max |g| 1.45e-7 [bar 3e-4], norms 2.0e-8 and 1.8e-8 relative from
float64 [bar 1.61e-6], the two losses equal; every bit-equality holds; the file runs in 85 s, nearly all of it the children's start-up."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ddp_worker as W
import optim_ref as OR

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_ddp_worker.py")
DEV = "cuda:0"
KEYS = ("step", "loss", "learning_rate", "grad_norm", "skipped_steps")


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def torchrun(world, args, env=None, timeout=240):
    """one launch; fails the test when the child exits non-zero, so that nothing is started after it"""
    full = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""), **(env or {}))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port())] + args
    r = subprocess.run(cmd, cwd=ROOT, env=full, capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return r


def visible_gpus():
    return torch.cuda.device_count()


def pretrain_args(data, cfg, out, accumulation, *extra, steps=6, save=3):
    return ["--config_name", cfg, "--dataset_name", data, "--do_train", "--output_dir", str(out), "--per_device_train_batch_size", str(W.BATCH),
            "--gradient_accumulation_steps", str(accumulation), "--learning_rate", str(W.LR), "--lr_scheduler_type", "constant",
            "--max_steps", str(steps), "--logging_steps", "1", "--save_steps", str(save), "--seed", str(W.SEED), "--device", DEV, *extra]


def history(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return [{k: e[k] for k in KEYS} for e in json.load(f)["log_history"]]


def listing(out):
    return sorted(os.path.relpath(os.path.join(d, f), out) for d, _, fs in os.walk(out) for f in fs)


def same_tensors(a, b):
    return set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


def optimizer_tensors(path):
    sd = torch.load(path, weights_only=False)
    out = {f"{q}.{n}": t for q in ("master", "exp_avg", "exp_avg_sq") for n, t in zip(sd["names"], sd[q])}
    return out, (sd["step"], sd["skipped"])


def compare_runs(a, b, checkpoint=True):
    from safetensors.torch import load_file
    assert same_tensors(load_file(str(a / "model.safetensors")), load_file(str(b / "model.safetensors")))
    assert history(a) == history(b) and [e["step"] for e in history(a)] == [1, 2, 3, 4, 5, 6]
    if checkpoint:
        assert same_tensors(load_file(str(a / "checkpoint-3" / "model.safetensors")), load_file(str(b / "checkpoint-3" / "model.safetensors")))
        (ta, sa), (tb, sb) = optimizer_tensors(a / "checkpoint-3" / "optimizer.pt"), optimizer_tensors(b / "checkpoint-3" / "optimizer.pt")
        assert sa == sb == (3, 0) and same_tensors(ta, tb)
        with open(a / "checkpoint-3" / "trainer_state.json") as fa, open(b / "checkpoint-3" / "trainer_state.json") as fb:
            assert json.load(fa) == json.load(fb)                                # steps_per_epoch, epoch, schedule: the single process's
        assert torch.equal(torch.load(a / "checkpoint-3" / "rng_state.pt", weights_only=False)["mask_generator"],
                           torch.load(b / "checkpoint-3" / "rng_state.pt", weights_only=False)["mask_generator"])


def metrics_lines(r):
    return [ln for ln in r.stdout.splitlines() if ln.startswith("{") and "train_runtime" in ln]


@pytest.fixture(scope="module")
def single(tmp_path_factory):
    """run (a): plain python, batch 2, accumulation 2 - the run every other pretrain run here must equal"""
    from plantcaduceus_amd import pretrain
    tmp = tmp_path_factory.mktemp("ddp")
    data, cfg = W.write_inputs(tmp)
    out = tmp / "a"
    pretrain.main(pretrain_args(data, cfg, out, 2))
    return tmp, data, cfg, out


def test_pretrain_world2_gloo_equals_accumulation_2(single):
    tmp, data, cfg, a = single
    b, c = tmp / "b", tmp / "c"
    r = torchrun(2, ["-m", "plantcaduceus_amd.pretrain"] + pretrain_args(data, cfg, b, 1, "--ddp_backend", "gloo"))
    compare_runs(a, b)
    assert listing(a) == listing(b) and len(metrics_lines(r)) == 1               # only rank 0 wrote and reported
    with open(a / "train_results.json") as fa, open(b / "train_results.json") as fb:
        ra, rb = json.load(fa), json.load(fb)
    assert ra["train_loss"] == rb["train_loss"] and ra["epoch"] == rb["epoch"] == 3.0 and ra["train_samples"] == rb["train_samples"] == W.N_WIN
    # a checkpoint written by one process resumes at world 2 (accumulation halved), the backend taken from the environment this time
    r = torchrun(2, ["-m", "plantcaduceus_amd.pretrain"] + pretrain_args(data, cfg, c, 1, "--resume_from_checkpoint", str(a / "checkpoint-3")),
                 env={"PCAD_DDP_BACKEND": "gloo"})
    compare_runs(a, c, checkpoint=False)
    # ... and the other way round: the world-2 checkpoint under plain python with the accumulation doubled
    from plantcaduceus_amd import pretrain
    d = tmp / "d"
    pretrain.main(pretrain_args(data, cfg, d, 2, "--resume_from_checkpoint", str(b / "checkpoint-3")))
    compare_runs(a, d, checkpoint=False)


def test_pretrain_world1_rccl_equals_plain_python(single):
    tmp, data, cfg, a = single
    out = tmp / "nccl1"
    torchrun(1, ["-m", "plantcaduceus_amd.pretrain"] + pretrain_args(data, cfg, out, 2, "--ddp_backend", "nccl"))
    compare_runs(a, out)


def lora_args(tmp, out, accumulation):
    return ["train", "--train_dir", str(tmp / "train.parquet"), "--valid_dir", str(tmp / "valid.parquet"), "--model_name", str(tmp / "base"),
            "--output_dir", str(out), "--train_batch_size", "2", "--eval_batch_size", "4", "--gradient_accumulation_steps", str(accumulation),
            "--learning_rate", "1e-3", "--lr_scheduler_type", "constant", "--warmup_steps", "0", "--max_steps", "4", "--logging_steps", "1",
            "--eval_steps", "2", "--save_steps", "2", "--seed", "42", "--device", DEV]


def test_lora_train_world2_gloo_equals_accumulation_2(tmp_path):
    from safetensors.torch import load_file
    import test_gpu_lora_train as LT
    from plantcaduceus_amd import lora_predict
    LT.write_inputs(tmp_path)
    a, b = tmp_path / "one", tmp_path / "two"
    lora_predict.main(lora_args(tmp_path, a, 2))
    torchrun(2, ["-m", "plantcaduceus_amd.lora_predict"] + lora_args(tmp_path, b, 1), env={"PCAD_DDP_BACKEND": "gloo"})
    wa, wb = load_file(str(a / "adapter_model.safetensors")), load_file(str(b / "adapter_model.safetensors"))
    assert same_tensors(wa, wb)
    assert any("lora_B" in k and bool(v.any()) for k, v in wa.items())           # the factors moved
    with open(a / "trainer_state.json") as fa, open(b / "trainer_state.json") as fb:
        ha, hb = json.load(fa)["log_history"], json.load(fb)["log_history"]
    strip = lambda h: [{k: v for k, v in e.items() if k != "eval_runtime"} for e in h]
    assert strip(ha) == strip(hb) and sum("eval_loss" in e for e in ha) == 2
    assert listing(a) == listing(b)


def run_worker(world, out, accumulation, *extra, backend="gloo"):
    os.makedirs(out, exist_ok=True)
    args = [WORKER, str(out), str(accumulation), "--backend", backend, *extra]
    if world == 0:                                                               # one process, no group: in this one
        W.main(args[1:])
        return [torch.load(os.path.join(out, "r0.pt"), weights_only=False)]
    torchrun(world, args)
    return [torch.load(os.path.join(out, f"r{k}.pt"), weights_only=False) for k in range(world)]


def check_world4_against_accumulation_4(ranks, one):
    import scan_ref as R
    gbar = 2 * (2 * W.toy_config().n_layer + 1) * R.BAR_SCAN[False]
    assert abs(gbar - 3e-4) < 1e-12
    first = ranks[0]
    assert [r["rank"] for r in ranks] == [0, 1, 2, 3] and all(r["world"] == 4 and r["scale"] == 0.25 == one["scale"] for r in ranks)
    for r in ranks[1:]:
        assert torch.equal(r["flat"], first["flat"]) and r["checksum"] == first["checksum"] and r["state"] == first["state"]
    assert first["offsets"] == one["offsets"] and first["names"] == one["names"]
    worst = 0.0
    for name, o, n in zip(first["names"], first["offsets"], first["sizes"]):
        ga, gb = one["flat"][o:o + n].double(), first["flat"][o:o + n].double()
        top = ga.abs().max().item()
        d = (ga - gb).abs().max().item()
        worst = max(worst, d / top)
        assert top > 0 and d <= gbar * top, (name, d, top)
    for r in (first, one):
        norm64 = float((r["flat"].double() * r["scale"]).pow(2).sum().sqrt())
        rel = abs(r["state"]["norm"] - norm64) / norm64
        print(f"world {r['world']}: norm {r['state']['norm']:.7f} float64 {norm64:.7f} relative {rel:.2e} [bar {OR.norm_bar(r['chunks']):.2e}]; loss {r['loss']:.6f}")
        assert rel <= OR.norm_bar(r["chunks"]) == OR.norm_bar(300) and r["state"]["finite"] == 1 and r["changed"]
    print(f"world 4 vs accumulation 4: worst |d flat| / max |g| over the tensors {worst:.2e} [bar {gbar:.1e}]")
    # the four micro-batch losses are the same fp32 values in both runs (the same kernels on the same windows and masks); only the order
    # of their sum differs: 3 additions of positive terms on either side, each within 2^-24 relative of the running sum
    assert abs(first["loss"] - one["loss"]) <= 6 * 2.0 ** -24 * abs(one["loss"])


def test_world4_gloo_one_step_against_accumulation_4(tmp_path):
    one = run_worker(0, tmp_path / "one", 4)[0]
    ranks = run_worker(4, tmp_path / "four", 1)
    check_world4_against_accumulation_4(ranks, one)


def test_one_ranks_inf_skips_the_step_on_every_rank(tmp_path):
    ranks = run_worker(4, tmp_path / "inf", 1, "--inf_rank", "1")
    for r in ranks:
        assert r["state"]["finite"] == 0 and r["state"]["skipped"] == 1 and not r["changed"], r["rank"]
    assert len({r["checksum"] for r in ranks}) == 1


def test_bf16_world2_gloo(tmp_path):
    from safetensors.torch import load_file
    data, cfg = W.write_inputs(tmp_path)
    out = tmp_path / "bf16"
    torchrun(2, ["-m", "plantcaduceus_amd.pretrain"] + pretrain_args(data, cfg, out, 1, "--ddp_backend", "gloo", "--dtype", "bfloat16", steps=4, save=4))
    sd = load_file(str(out / "checkpoint-4" / "model.safetensors"))
    opt = torch.load(str(out / "checkpoint-4" / "optimizer.pt"), weights_only=False)
    with open(out / "trainer_state.json") as f:
        hist = json.load(f)["log_history"]
    print(f"bf16 world 2 losses {[round(e['loss'], 5) for e in hist]}")
    assert opt["step"] == 4 and opt["skipped"] == 0 and len(hist) == 4 and all(np.isfinite(e["loss"]) for e in hist)
    for name, master in zip(opt["names"], opt["master"]):
        assert sd[name].dtype == torch.bfloat16 and master.dtype == torch.float32 and torch.equal(sd[name], master.to(torch.bfloat16)), name


# N > 1 over RCCL, one device per rank: collected and skipped on a one-GPU box, so these have NOT run until a box shows N devices.
def test_pretrain_world2_rccl_equals_accumulation_2(single):
    if visible_gpus() < 2:
        pytest.skip(f"needs 2 GPUs, {visible_gpus()} visible")
    tmp, data, cfg, a = single
    out = tmp / "nccl2"
    torchrun(2, ["-m", "plantcaduceus_amd.pretrain"] + pretrain_args(data, cfg, out, 1, "--ddp_backend", "nccl"))
    compare_runs(a, out)


def test_world4_rccl_one_step_against_accumulation_4(tmp_path):
    if visible_gpus() < 4:
        pytest.skip(f"needs 4 GPUs, {visible_gpus()} visible")
    one = run_worker(0, tmp_path / "one", 4)[0]
    ranks = run_worker(4, tmp_path / "four", 1, backend="nccl")
    check_world4_against_accumulation_4(ranks, one)
