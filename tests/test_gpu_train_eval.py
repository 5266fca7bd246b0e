"""-m gpu: evaluation inside the pretraining loop and validation sharded over the ranks, on §4o's toy geometry (n_layer 2,
d_model 64, d_inner 128, dt_rank 4; the 8 training windows of tests/test_gpu_pretrain.py, L = 69, batch 4, fp32 unless said) with a
validation table of 7 OTHER windows and --per_device_eval_batch_size 2: a short last loss batch and, at world 2, an uneven last shard
(4 batches: rank 0 takes rows 0 - 3, rank 1 rows 4 - 6).

  run 1         --eval_strategy steps --eval_steps 2 --save_steps 2 --max_steps 6: evaluation entries at 2, 4, 6 with every key; each
                eval_loss == (as floats) pretrain.evaluate_model on a fresh TrainableCaduceusForMaskedLM.from_pretrained(checkpoint-<step>)
                - in fp32 the checkpoint holds the live weights and the kernels are reproducible; eval_loss_token_mean within the
                project's forward bar 2 x 1e-4 x max |logit| of mlm_eval.evaluate_split on the inference class with the same seed
  no evaluation the same command with --eval_strategy no: model.safetensors bit-equal, the training entries equal
  resume        run 1 again from checkpoint-4, in run 1's output_dir (a copy of the finished run 1 is kept to compare with):
                model.safetensors bit-equal, the log history from step 5 on equal less the timing keys, the best_* fields equal
  best          --save_total_limit 2 --load_best_model_at_end: best_metric is the minimum logged eval_loss, output_dir's model is that
                checkpoint's, at most two checkpoints remain (three if the best is neither of the two newest)
  world 2       accumulation 2 in one process against torchrun world 2 over gloo (both ranks on cuda:0), accumulation 1, both evaluating:
                evaluation entries equal less the timing keys, model.safetensors bit-equal, only rank 0 wrote
  world 1 RCCL  run 1 under torchrun with one rank over RCCL (the gather on a device tensor): evaluation entries and weights as run 1's
  lora train    tests/test_gpu_lora_train.py's inputs, validation cut to 5 windows, --eval_batch_size 2: the same pair of runs; eval_*
                entries equal less eval_runtime, adapter_model.safetensors bit-equal
  bf16          --dtype bfloat16, 4 steps, evaluation every 2: finite eval_loss entries
Every child is `python -m torch.distributed.run` under tests/test_gpu_ddp.py's helper: its own time limit, and the test stops at the
first child that exits non-zero.  Every case prints its figures before it asserts."""
import json
import math
import os
import shutil

import numpy as np
import pytest
import torch

import test_gpu_ddp as D
import test_gpu_pretrain as P

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
F32 = torch.float32
N_VALID, EVAL_BATCH, SEED = 7, 2, P.SEED
TIMING = ("eval_runtime", "eval_samples_per_second", "eval_steps_per_second")
EVAL_KEYS = ("eval_loss", "perplexity", "eval_token_accuracy", "eval_loss_token_mean", "eval_samples", "eval_labelled_tokens") + TIMING + ("step", "epoch")
EVAL = ("--eval_strategy", "steps", "--eval_steps", "2")


def valid_sequences():
    g = np.random.default_rng(10)                                       # not the training windows' stream (9)
    return ["".join(g.choice(list("ACGTacgt"), size=P.L)) for _ in range(N_VALID)]


def write_inputs(tmp):
    from plantcaduceus_amd.checkpoint import save_checkpoint, synthetic_state_dict
    data = tmp / "data"
    data.mkdir()
    for split, seqs in (("train", P.sequences()), ("validation", valid_sequences())):
        with open(data / f"{split}.tsv", "w") as f:
            f.write("seq\n" + "\n".join(seqs) + "\n")
    save_checkpoint(str(tmp / "cfg"), P.toy_config(), synthetic_state_dict(P.toy_config(), seed=SEED, stress=False), with_tokenizer=False)
    return str(data), str(tmp / "cfg" / "config.json")


def argv(data, cfg, out, *extra, batch=P.BATCH, accumulation=1):
    return ["--config_name", cfg, "--dataset_name", data, "--do_train", "--output_dir", str(out), "--per_device_train_batch_size", str(batch),
            "--gradient_accumulation_steps", str(accumulation), "--per_device_eval_batch_size", str(EVAL_BATCH), "--learning_rate", str(P.LR),
            "--lr_scheduler_type", "constant", "--max_steps", "6", "--logging_steps", "1", "--save_steps", "2", "--seed", str(SEED),
            "--device", DEV, *extra]


def state(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return json.load(f)


def evaluations(hist, timing=True):
    return [{k: v for k, v in e.items() if timing or k not in TIMING} for e in hist if "eval_loss" in e]


def trainings(hist):
    return [e for e in hist if "loss" in e]


def best_of(ts):
    return {k: ts[k] for k in ("best_metric", "best_global_step", "best_model_checkpoint")}


def weights(path):
    from safetensors.torch import load_file
    return load_file(str(path))


@pytest.fixture(scope="module")
def run1(tmp_path_factory):
    """-> (data, cfg, kept, out): run 1 in `out`, and `kept`, a copy of the finished run that no later test writes to"""
    from plantcaduceus_amd import pretrain
    tmp = tmp_path_factory.mktemp("train_eval")
    data, cfg = write_inputs(tmp)
    out, kept = tmp / "run1", tmp / "run1_kept"
    pretrain.main(argv(data, cfg, out, *EVAL))
    shutil.copytree(out, kept)
    return data, cfg, kept, out


def test_evaluations_in_the_loop_equal_the_checkpoints_own(run1):
    from plantcaduceus_amd import mlm_eval, pretrain
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    data, cfg, kept, out = run1
    ts = state(kept)
    evs = evaluations(ts["log_history"])
    assert [e["step"] for e in evs] == [2, 4, 6] and [e["step"] for e in trainings(ts["log_history"])] == [1, 2, 3, 4, 5, 6]
    for e in evs:
        assert set(e) == set(EVAL_KEYS), sorted(set(e) ^ set(EVAL_KEYS))
        assert e["eval_samples"] == N_VALID and e["eval_labelled_tokens"] > 0 and e["epoch"] == e["step"] / 2
        assert e["perplexity"] == math.exp(e["eval_loss"]) and e["eval_runtime"] > 0 and e["eval_samples_per_second"] > 0
    # log, evaluate, save: checkpoint-<step>'s own trainer_state.json ends with that step's evaluation
    for e in evs:
        assert state(kept / f"checkpoint-{e['step']}")["log_history"][-1] == e
    tok, seqs = CaduceusTokenizer(), valid_sequences()
    rng = torch.get_rng_state()
    valid = pretrain.ValidationSet.build(tok, seqs, 1.0, 0.15, EVAL_BATCH, SEED)
    assert torch.equal(torch.get_rng_state(), rng) and valid.n == N_VALID
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    for e in evs:
        ckpt = str(kept / f"checkpoint-{e['step']}")
        model = TrainableCaduceusForMaskedLM.from_pretrained(ckpt, dtype=F32, device=DEV)
        sums = pretrain.evaluate_model(model, valid, DEV)
        mine = mlm_eval.metrics_from_sums(sums, EVAL_BATCH, "eval")
        eng = CaduceusForMaskedLM.from_pretrained(ckpt).to(F32).to(DEV).eval()
        ref = mlm_eval.evaluate_split(eng, tok, seqs, "eval", 1.0, 0.15, EVAL_BATCH, SEED, None, DEV)
        with torch.no_grad():
            top = eng(input_ids=up(valid.ids), labels=up(valid.labels), loss_weights=up(valid.weights)).logits.abs().max().item()
        bar = 2 * 1e-4 * top
        print(f"step {e['step']}: eval_loss logged {e['eval_loss']!r} checkpoint's {mine['eval_loss']!r}; eval_loss_token_mean {e['eval_loss_token_mean']:.7f} "
              f"evaluate_split {ref['eval_loss_token_mean']:.7f} [bar {bar:.3e}, max |logit| {top:.3f}]; labelled {e['eval_labelled_tokens']} / {ref['eval_labelled_tokens']}")
        assert sums.shape == (N_VALID, 4) and sums.dtype == np.float32
        assert e["eval_loss"] == mine["eval_loss"] and np.isfinite(e["eval_loss"])
        assert all(e[k] == mine[k] for k in mine)
        assert e["eval_labelled_tokens"] == ref["eval_labelled_tokens"] and e["eval_samples"] == ref["eval_samples"]      # the same masks
        assert abs(e["eval_loss_token_mean"] - ref["eval_loss_token_mean"]) <= bar
    # the best is the lowest eval_loss, every evaluated step being a saved one here
    low = min(evs, key=lambda e: e["eval_loss"])
    assert best_of(ts) == {"best_metric": low["eval_loss"], "best_global_step": low["step"],
                           "best_model_checkpoint": os.path.join(str(out), f"checkpoint-{low['step']}")}


def test_an_evaluation_changes_nothing_it_does_not_own(run1, tmp_path):
    from plantcaduceus_amd import pretrain
    data, cfg, kept, _ = run1
    out = tmp_path / "no_eval"
    pretrain.main(argv(data, cfg, out, "--eval_strategy", "no"))
    ha, hb = state(kept)["log_history"], state(out)["log_history"]
    print(f"losses with evaluation {[round(e['loss'], 6) for e in trainings(ha)]} without {[round(e['loss'], 6) for e in hb]}")
    assert D.same_tensors(weights(kept / "model.safetensors"), weights(out / "model.safetensors"))
    assert evaluations(hb) == [] and trainings(ha) == hb and len(hb) == 6
    assert all(k in e for e in hb for k in ("loss", "grad_norm", "learning_rate"))
    assert best_of(state(out)) == {"best_metric": None, "best_global_step": 0, "best_model_checkpoint": None}
    for step in (2, 4, 6):
        assert D.same_tensors(weights(kept / f"checkpoint-{step}" / "model.safetensors"), weights(out / f"checkpoint-{step}" / "model.safetensors"))


def test_resume_restores_the_evaluations_and_the_best(run1):
    from plantcaduceus_amd import pretrain
    data, cfg, kept, out = run1
    pretrain.main(argv(data, cfg, out, *EVAL, "--resume_from_checkpoint", str(out / "checkpoint-4")))
    ta, tb = state(kept), state(out)
    strip = lambda h: [{k: v for k, v in e.items() if k not in TIMING} for e in h]
    later = lambda h: [e for e in strip(h) if e["step"] >= 5]
    print(f"resumed: best {best_of(tb)}; straight: best {best_of(ta)}; entries from step 5 on: {len(later(tb['log_history']))}")
    assert D.same_tensors(weights(kept / "model.safetensors"), weights(out / "model.safetensors"))
    assert later(ta["log_history"]) == later(tb["log_history"]) and len(later(tb["log_history"])) == 3       # losses 5, 6 and the evaluation at 6
    assert ta["log_history"][:6] == tb["log_history"][:6]                   # up to step 4: the checkpoint's own history, timing included
    assert best_of(ta) == best_of(tb) and tb["best_metric"] is not None
    assert D.same_tensors(weights(kept / "checkpoint-6" / "model.safetensors"), weights(out / "checkpoint-6" / "model.safetensors"))


def test_save_total_limit_and_load_best_model_at_end(run1, tmp_path):
    from plantcaduceus_amd import pretrain
    data, cfg, kept, _ = run1
    out = tmp_path / "best"
    pretrain.main(argv(data, cfg, out, *EVAL, "--save_total_limit", "2", "--load_best_model_at_end"))
    ts = state(out)
    evs = evaluations(ts["log_history"])
    left = sorted(int(os.path.basename(d).split("-")[1]) for d in pretrain.checkpoint_dirs(str(out)))
    print(f"eval_loss {[e['eval_loss'] for e in evs]}; best {best_of(ts)}; checkpoints left {left}")
    assert [e["step"] for e in evs] == [2, 4, 6]
    assert ts["best_metric"] == min(e["eval_loss"] for e in evs) and os.path.isdir(ts["best_model_checkpoint"])
    assert ts["best_model_checkpoint"] == os.path.join(str(out), f"checkpoint-{ts['best_global_step']}")
    assert D.same_tensors(weights(out / "model.safetensors"), weights(os.path.join(ts["best_model_checkpoint"], "model.safetensors")))
    assert 6 in left and ts["best_global_step"] in left
    assert len(left) <= (3 if ts["best_global_step"] not in (4, 6) else 2)
    assert evaluations(state(kept)["log_history"], timing=False) == evaluations(ts["log_history"], timing=False)      # the flags change no number


def test_world2_gloo_shards_the_validation_and_equals_one_process(run1, tmp_path):
    from plantcaduceus_amd import pretrain
    data, cfg, _, _ = run1
    a, b = tmp_path / "one", tmp_path / "two"
    pretrain.main(argv(data, cfg, a, *EVAL, accumulation=2))
    r = D.torchrun(2, ["-m", "plantcaduceus_amd.pretrain"] + argv(data, cfg, b, *EVAL, "--ddp_backend", "gloo", accumulation=1))
    ea, eb = evaluations(state(a)["log_history"], timing=False), evaluations(state(b)["log_history"], timing=False)
    print(f"eval_loss one process {[e['eval_loss'] for e in ea]} world 2 {[e['eval_loss'] for e in eb]}")
    assert [e["step"] for e in ea] == [2, 4, 6] and ea == eb
    assert D.same_tensors(weights(a / "model.safetensors"), weights(b / "model.safetensors"))
    assert D.listing(a) == D.listing(b) and len(D.metrics_lines(r)) == 1           # only rank 0 wrote and reported
    strip = lambda ts: dict(ts, log_history=[{k: v for k, v in e.items() if k not in TIMING} for e in ts["log_history"]],
                            best_model_checkpoint=os.path.basename(ts["best_model_checkpoint"]))
    assert strip(state(a)) == strip(state(b))


def test_world1_rccl_gathers_on_the_device_and_equals_plain_python(run1, tmp_path):
    """the gather's RCCL form (a device tensor, no host staging) on every box: a one-rank group runs the same collective as N ranks"""
    data, cfg, kept, _ = run1
    out = tmp_path / "nccl1"
    D.torchrun(1, ["-m", "plantcaduceus_amd.pretrain"] + argv(data, cfg, out, *EVAL, "--ddp_backend", "nccl"))
    ea, eb = evaluations(state(kept)["log_history"], timing=False), evaluations(state(out)["log_history"], timing=False)
    print(f"eval_loss plain python {[e['eval_loss'] for e in ea]} world 1 over RCCL {[e['eval_loss'] for e in eb]}")
    assert [e["step"] for e in eb] == [2, 4, 6] and ea == eb
    assert D.same_tensors(weights(kept / "model.safetensors"), weights(out / "model.safetensors"))
    assert state(kept)["best_metric"] == state(out)["best_metric"] and state(out)["best_global_step"] == state(kept)["best_global_step"]


def test_lora_train_world2_gloo_shards_the_validation(tmp_path):
    import pyarrow as pa
    import pyarrow.parquet as pq
    import test_gpu_lora_train as LT
    from plantcaduceus_amd import lora_predict
    LT.write_inputs(tmp_path)
    _, _, va, yva = LT.windows()
    pq.write_table(pa.table({"input_ids": pa.array(list(va[:5]), type=pa.list_(pa.int32())), "label": pa.array(yva[:5])}), str(tmp_path / "valid.parquet"))
    args = lambda out, accumulation: ["train", "--train_dir", str(tmp_path / "train.parquet"), "--valid_dir", str(tmp_path / "valid.parquet"),
                                      "--model_name", str(tmp_path / "base"), "--output_dir", str(out), "--train_batch_size", "2",
                                      "--eval_batch_size", "2", "--gradient_accumulation_steps", str(accumulation), "--learning_rate", "1e-3",
                                      "--lr_scheduler_type", "constant", "--warmup_steps", "0", "--max_steps", "4", "--logging_steps", "1",
                                      "--eval_steps", "2", "--save_steps", "2", "--seed", "42", "--device", DEV]
    a, b = tmp_path / "one", tmp_path / "two"
    lora_predict.main(args(a, 2))
    D.torchrun(2, ["-m", "plantcaduceus_amd.lora_predict"] + args(b, 1), env={"PCAD_DDP_BACKEND": "gloo"})
    strip = lambda h: [{k: v for k, v in e.items() if k != "eval_runtime"} for e in h if "eval_loss" in e]
    ea, eb = strip(state(a)["log_history"]), strip(state(b)["log_history"])
    print(f"lora eval_loss one process {[e['eval_loss'] for e in ea]} world 2 {[e['eval_loss'] for e in eb]}")
    assert [e["step"] for e in ea] == [2, 4] and ea == eb and all(np.isfinite(e["eval_loss"]) for e in ea)
    assert D.same_tensors(weights(a / "adapter_model.safetensors"), weights(b / "adapter_model.safetensors"))
    assert D.listing(a) == D.listing(b)


def test_bf16_evaluations_are_finite(run1, tmp_path):
    from plantcaduceus_amd import pretrain
    data, cfg, _, _ = run1
    out = tmp_path / "bf16"
    pretrain.main(argv(data, cfg, out, *EVAL, "--dtype", "bfloat16", "--max_steps", "4"))
    evs = evaluations(state(out)["log_history"])
    print(f"bf16 eval_loss {[e['eval_loss'] for e in evs]}")
    assert [e["step"] for e in evs] == [2, 4] and all(np.isfinite(e["eval_loss"]) and np.isfinite(e["eval_loss_token_mean"]) for e in evs)
    assert all(e["eval_samples"] == N_VALID for e in evs)
