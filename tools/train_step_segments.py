"""Time one training step (forward + backward) of both trainable models with the scan unsegmented (scan_bwd_segments = scan_fwd_segments
= 1: the default path, bit for bit), with its backward on "auto" (DESIGN.md §4v), and with its backward and its forward on "auto" (§4w), in
one process on one device: tools/train_memory.py's configuration - synthetic weights at PlantCAD2 Small's geometry, L = 8 192, fp32 and
bf16, recompute off - at one and four windows.  HIP events around forward + backward, one untimed step first, median over --reps steps;
the legs of a (model, dtype, batch) run in the order off, backward auto, both auto.

    python tools/train_step_segments.py [--out profiles/train_step_segments.txt (the default)] [--reps 3] [--batches 1,4] [--L 8192]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine, ops  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402
from tools.train_memory import DEV, build, inputs, step, timed  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_step_segments.txt"))
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--batches", default="1,4")
    ap.add_argument("--size", default="pc2-small")
    ap.add_argument("--L", type=int, default=8192)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_step_segments needs a ROCm device: a time taken anywhere else says nothing")
    cfg = make_config(a.size)
    sd = synthetic_state_dict(cfg, stress=False)
    L = a.L
    lines = [f"# one training step (forward + backward), scan unsegmented, backward on auto, backward and forward on auto, {torch.cuda.get_device_name(0)}, "
             f"build {engine.load_library().pcad_build_hash().decode()}",
             f"# {a.size}: D={cfg.d_model} E={cfg.d_inner} R={cfg.dt_rank} n_layer={cfg.n_layer}, L={L}; synthetic weights; recompute off; "
             f"HIP events, median of {a.reps} steps after one untimed step; SCAN_BWD_SEG_MIN_STEPS = {ops.SCAN_BWD_SEG_MIN_STEPS}",
             "model      dtype     windows  segments(auto)  off_ms    auto_ms   auto/off  both_ms  both/off  both/auto"]
    for kind in ("masked LM", "LoRA"):
        for dt in (torch.float32, torch.bfloat16):
            model = build(kind, cfg, sd, dt)
            step(model, inputs(kind, 1, 64))                             # first use: handles and workspaces are created once
            for nb in (int(v) for v in a.batches.split(",")):
                batch = inputs(kind, nb, L)
                with torch.cuda.device(DEV):
                    G = ops.scan_bwd_auto_segments(2 * nb, L, cfg.d_inner)
                ms = {}
                for setting, (bwd, fwd) in ((1, (1, 1)), ("auto", ("auto", 1)), ("both", ("auto", "auto"))):
                    model.scan_bwd_segments, model.scan_fwd_segments = bwd, fwd
                    step(model, batch)
                    ms[setting] = timed(model, batch, a.reps)
                model.scan_bwd_segments = model.scan_fwd_segments = 1
                model.zero_grad(set_to_none=True)
                lines.append(f"{kind:9s}  {str(dt).split('.')[-1]:8s}  {nb:7d}  {G:14d}  {ms[1]:8.1f}  {ms['auto']:8.1f}  {ms['auto'] / ms[1]:9.3f}"
                             f"  {ms['both']:7.1f}  {ms['both'] / ms[1]:8.3f}  {ms['both'] / ms['auto']:9.3f}")
                print(lines[-1], flush=True)
                del batch
            del model
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
