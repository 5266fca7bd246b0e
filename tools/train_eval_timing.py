"""Time one evaluation inside the pretraining loop against `mlm_eval` through the inference engine, on the same windows and the same
device (recorded, nothing asserted):

    (a)  pretrain.Trainer.evaluate: the training model under torch.no_grad(), one forward per loss batch, masks drawn before the run -
         its own `eval_samples_per_second`
    (b)  mlm_eval.evaluate_split on CaduceusForMaskedLM (the engine's fused loss head): tokenization, the mask draw and the forward,
         as the `mlm_eval` command and `pretrain --do_eval` run it
    (b') mlm_eval.window_sums alone: (b) without tokenization and mask draw

at the PlantCaduceus_l20 geometry, bf16, 512 validation windows of 512 bp, synthetic weights (timing only).  Wall clock with a device
synchronisation on either side; the figure of a series is the median over --repeats calls after --warmup.

    python tools/train_eval_timing.py [--out profiles/train_eval_timing.txt] [--windows 512] [--length 512] [--eval_batch 32]
"""
import argparse
import os
import statistics
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from plantcaduceus_amd import mlm_eval, pretrain  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict  # noqa: E402
from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM  # noqa: E402


def wall(fn, dev):
    torch.cuda.synchronize(dev)
    t0 = time.time()
    out = fn()
    torch.cuda.synchronize(dev)
    return time.time() - t0, out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default="l20")
    ap.add_argument("--windows", type=int, default=512)
    ap.add_argument("--length", type=int, default=512)
    ap.add_argument("--eval_batch", type=int, default=32)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    w = ap.parse_args()
    dev = "cuda:0"
    cfg = make_config(w.size)
    sd = synthetic_state_dict(cfg, seed=w.seed, stress=False)
    g = np.random.default_rng(w.seed)
    seqs = ["".join(g.choice(list("ACGTacgt"), size=w.length)) for _ in range(w.windows)]
    lines = [f"device {torch.cuda.get_device_name(0)}; {w.size} geometry (n_layer {cfg.n_layer}, d_model {cfg.d_model}), bfloat16, synthetic weights; "
             f"{w.windows} windows of {w.length} bp, loss batches of {w.eval_batch}; median of {w.repeats} calls after {w.warmup}"]
    with tempfile.TemporaryDirectory() as tmp:
        save_checkpoint(tmp, cfg, sd)
        # (a) the evaluation of the training loop, on the training model
        model = TrainableCaduceusForMaskedLM(cfg, dtype=torch.bfloat16, device=dev)
        model.load_state_dict(sd)
        eng, tok = mlm_eval.load_model_and_tokenizer(tmp, None, dev, "bfloat16")
        valid = pretrain.ValidationSet.build(tok, seqs, 1.0, 0.15, w.eval_batch, w.seed)
        a = pretrain.build_parser().parse_args(["--dataset_name", "-", "--output_dir", tmp, "--device", dev])
        source = type("Source", (), {"steps_per_epoch": 1})()
        tr = pretrain.Trainer(model, None, source, tok, a, 1, 0, valid=valid)
        series = {
            "a  pretrain.Trainer.evaluate (training model, no_grad)": lambda: tr.evaluate(),
            "b  mlm_eval.evaluate_split (engine; tokenize + masks + forward)":
                lambda: mlm_eval.evaluate_split(eng, tok, seqs, "eval", 1.0, 0.15, w.eval_batch, w.seed, None, dev),
            "b' mlm_eval.window_sums (engine; forward only)":
                lambda: mlm_eval.metrics_from_sums(mlm_eval.window_sums(eng, valid.ids, valid.labels, valid.weights, dev)[0], w.eval_batch, "eval"),
        }
        for name, fn in series.items():
            for _ in range(w.warmup):
                fn()
            runs = [wall(fn, dev) for _ in range(w.repeats)]
            sec = statistics.median(t for t, _ in runs)
            res = runs[-1][1]
            extra = f"; its own eval_samples_per_second {res['eval_samples_per_second']}" if "eval_samples_per_second" in res else ""
            lines.append(f"{name}: {sec * 1e3:.1f} ms, {w.windows / sec:.0f} samples/s; eval_loss {res['eval_loss']:.6f} "
                         f"eval_loss_token_mean {res['eval_loss_token_mean']:.6f}{extra}")
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if w.out:
        with open(w.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
