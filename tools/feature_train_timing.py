"""Time the frozen-trunk fine-tuning mode on cached features against the plain `--train_lora 0` path (recorded, nothing
asserted), at the PlantCAD2 Small geometry with synthetic weights, L = 8 192, 64 training windows, batch 4, for a bf16 model and for an
fp32 model whose feature engine runs with "f32_gemm_split" 1 (what `lora_predict train` sets):

    plain    one micro-step of the parent's path: model(input_ids, labels) + loss.backward() on the trainable model (the trunk is frozen,
             so autograd reaches `score` alone, but every window goes through the operator composition)
    pass     the feature pass: model.pooled_features over the 64 windows in fixed blocks of 2^18 // L = 32, in windows/s
    cached   one micro-step on cached features: index_select of 4 rows + model(pooled=..., labels=...) + loss.backward()
    eval     one evaluation on cached features: logits of the 64 rows in batches of --eval_batch

HIP events on the current stream, one process; the legs are interleaved (plain, pass, cached, eval, plain, ...) and the figure of a leg
is the median over --repeats rounds after --warmup.

    python tools/feature_train_timing.py [--out profiles/feature_train_timing.txt] [--size pc2-small] [--length 8192] [--windows 64]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import torch  # noqa: E402

from plantcaduceus_amd import lora_predict  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402
from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification  # noqa: E402


def timed(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    out = fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b), out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--size", default="pc2-small")
    ap.add_argument("--length", type=int, default=8192)
    ap.add_argument("--windows", type=int, default=64)
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--eval_batch", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=1)
    ap.add_argument("--seed", type=int, default=42)
    w = ap.parse_args()
    dev = "cuda:0"
    cfg = make_config(w.size)
    sd = {k: v for k, v in synthetic_state_dict(cfg, seed=w.seed, stress=False).items() if k.startswith("caduceus.")}
    g = np.random.default_rng(w.seed)
    ids = g.integers(3, 7, size=(w.windows, w.length)).astype(np.int32)
    labels = torch.from_numpy(g.integers(0, 2, size=w.windows).astype(np.int64))
    fb = lora_predict.feature_block_windows(w.length, {})
    lines = [f"device {torch.cuda.get_device_name(0)}; {w.size} geometry (n_layer {cfg.n_layer}, d_model {cfg.d_model}), synthetic weights; "
             f"{w.windows} windows of {w.length} bp, micro-batch {w.batch}, feature blocks of {fb}, evaluation batches of {w.eval_batch}; HIP events, "
             f"legs interleaved, median of {w.repeats} rounds after {w.warmup}"]
    for name, dtype, options in (("bf16", torch.bfloat16, {}), ("fp32 + f32_gemm_split", torch.float32, {"f32_gemm_split": 1})):
        model = TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", dtype=dtype, device=dev, seed=w.seed, train_lora=False)
        model.load_trunk(sd)
        model.feature_engine(options)
        t = torch.from_numpy(ids)
        idx = torch.arange(w.batch, device=dev)
        state = {}

        def plain():
            out = model(t[:w.batch].to(dev), labels[:w.batch].to(dev))
            out.loss.backward()
            return out.loss.detach()

        def feature_pass():
            state["cache"] = lora_predict.cache_features(model, ids, dev, fb)
            return state["cache"]

        def cached():
            out = model(pooled=state["cache"].index_select(0, idx), labels=labels[:w.batch].to(dev))
            out.loss.backward()
            return out.loss.detach()

        def evaluation():
            with torch.no_grad():
                return torch.cat([model.logits_from_features(state["cache"][b0:b0 + w.eval_batch]) for b0 in range(0, w.windows, w.eval_batch)])

        legs = {"plain": plain, "pass": feature_pass, "cached": cached, "eval": evaluation}
        ms = {k: [] for k in legs}
        for r in range(w.warmup + w.repeats):
            for k, fn in legs.items():
                dt, _ = timed(fn)
                model.zero_grad(set_to_none=True)
                if r >= w.warmup:
                    ms[k].append(dt)
        med = {k: statistics.median(v) for k, v in ms.items()}
        with torch.no_grad():
            d = (model(pooled=state["cache"][:w.batch]).logits - model(t[:w.batch].to(dev)).logits).abs().max().item()
        lines.append(f"{name}: plain micro-step {med['plain']:.1f} ms ({w.batch * 1e3 / med['plain']:.1f} windows/s); feature pass {med['pass']:.1f} ms "
                     f"({w.windows * 1e3 / med['pass']:.1f} windows/s); cached micro-step {med['cached']:.3f} ms; cached evaluation of {w.windows} rows "
                     f"{med['eval']:.3f} ms")
        lines.append(f"{name}: trunk forward per window, plain / engine {med['plain'] / w.batch / (med['pass'] / w.windows):.2f}x; micro-step plain / cached "
                     f"{med['plain'] / med['cached']:.0f}x; the pass costs {med['pass'] / med['plain']:.1f} plain micro-steps; cache "
                     f"{state['cache'].numel() * 4} bytes; max |d logit| cached vs plain on the first micro-batch {d:.3e}")
        del model, state
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text, end="", flush=True)
    if w.out:
        with open(w.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
