"""Measure what DESIGN.md §4n / §4p compute from a formula: the peak bytes and the time of one training step (forward + backward) of both
trainable models, with every block's activations kept by autograd (the default) and with gradient checkpointing (each
block keeps its inputs and runs again inside the backward), next to training.stored_bytes_per_strand_position's prediction.

Synthetic weights at PlantCAD2 Small's geometry (D = 768, E = 1 536, R = 48, 24 layers), one window of L = 8 192; the masked LM with about
15 % of the positions labelled, the LoRA model as a two-class classifier with lora_B = 0.05 N(0, 1); fp32 and bf16 (fp32 residual stream).
  peak      torch.cuda.max_memory_allocated() of one forward + backward above the bytes allocated before it (model, inputs and the
            libraries' workspaces exist: one small step has run; gradients are released between the legs), recompute off, then on
  step      HIP events around forward + backward, median over the repeats: ten where they fit the leg's share of --budget seconds, fewer
            otherwise (the number used is printed)
  batch     the largest batch that ran with recompute on, doubling from 2 to 64: the search stops at the first failed allocation, or
            where the next step would pass the time budget (said so); nothing is tried twice, and any other error ends the run
One process; meant to run under `timeout -k 10 600`.  --legs off measures the default path alone and needs nothing of §4q, so the same
file times the parent commit's tree for the record.

    python tools/train_memory.py [--out profiles/train_memory.txt (the default)] [--budget 540] [--legs both|off] [--max_batch 64]
"""
import argparse
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine, training  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402

DEV = "cuda:0"


def formula(cfg, dtype, lora, recompute, L):
    """bytes per window by the formula, or None on a tree without it"""
    f = getattr(training, "stored_bytes_per_strand_position", None)
    return 2 * L * f(cfg, dtype, lora=lora, gradient_checkpointing=recompute) if f else None


def build(kind, cfg, sd, dtype):
    if kind == "masked LM":
        m = training.TrainableCaduceusForMaskedLM(cfg, dtype=dtype, device=DEV)
        m.load_state_dict(sd)
        return m
    m = training.TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", dtype=dtype, device=DEV)
    m.load_trunk({k: v for k, v in sd.items() if k.startswith("caduceus.")})
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".lora_B." in k:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))
    return m


def inputs(kind, batch, L):
    g = torch.Generator().manual_seed(17)
    ids = torch.randint(3, 7, (batch, L), generator=g)
    if kind == "masked LM":
        labels = torch.where(torch.rand(batch, L, generator=g) < 0.15, ids, torch.full_like(ids, -100)).to(torch.int32)
        return ids.to(DEV), labels.to(DEV)
    return ids.to(DEV), (torch.arange(batch) % 2).to(DEV)


def step(model, batch):
    model(*batch).loss.backward()


def set_recompute(model, on):
    if on:
        model.gradient_checkpointing_enable()
    elif hasattr(model, "gradient_checkpointing_disable"):
        model.gradient_checkpointing_disable()


def peak_of(model, batch):
    """(peak above the baseline, wall seconds) of one forward + backward"""
    model.zero_grad(set_to_none=True)
    torch.cuda.synchronize()
    torch.cuda.reset_peak_memory_stats()
    base = torch.cuda.memory_allocated()
    t0 = time.time()
    step(model, batch)
    torch.cuda.synchronize()
    return torch.cuda.max_memory_allocated() - base, time.time() - t0


def timed(model, batch, repeats):
    ms = []
    for _ in range(repeats):
        model.zero_grad(set_to_none=True)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        step(model, batch)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms)


def gib(n):
    return "      -" if n is None else f"{n / 2 ** 30:7.2f}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "train_memory.txt"))
    ap.add_argument("--budget", type=float, default=540.0, help="seconds the whole run may take; repeats and the batch search are cut to fit")
    ap.add_argument("--legs", default="both", choices=("both", "off"))
    ap.add_argument("--size", default="pc2-small")
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--max_batch", type=int, default=64)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("train_memory needs a ROCm device: a peak read anywhere else says nothing")
    start = time.time()
    left = lambda: a.budget - (time.time() - start)
    cfg = make_config(a.size)
    sd = synthetic_state_dict(cfg, stress=False)
    L = a.L
    free, total = torch.cuda.mem_get_info(DEV)
    cases = [(kind, dt) for kind in ("masked LM", "LoRA") for dt in (torch.float32, torch.bfloat16)]
    modes = (False, True) if a.legs == "both" else (False,)
    lines = [f"# one training step (forward + backward), {torch.cuda.get_device_name(0)}, {free / 1e9:.1f} of {total / 1e9:.1f} GB free at the start, "
             f"build {engine.load_library().pcad_build_hash().decode()}",
             f"# {a.size}: D={cfg.d_model} E={cfg.d_inner} R={cfg.dt_rank} n_layer={cfg.n_layer}, L={L}, one window (2 strands); synthetic weights; legs: {a.legs}",
             "# formula = 2 L x training.stored_bytes_per_strand_position (DESIGN.md §4n, §4p, §4q); peak = max_memory_allocated of the step above the "
             "bytes allocated before it; ms = HIP events, median of `reps` steps; GiB = 2^30 bytes",
             "model      dtype     recompute  formula_GiB  peak_GiB  peak/formula  step_ms  reps"]
    summary, search, ended = [], [], False
    share = a.budget * 0.45 / (len(cases) * len(modes))                  # seconds a (case, mode) leg may spend on its timed repeats
    for kind, dt in cases:
        name = str(dt).split(".")[-1]
        model = build(kind, cfg, sd, dt)
        step(model, inputs(kind, 1, 64))                                 # first use: handles and workspaces are created once
        batch = inputs(kind, 1, L)
        got = {}
        for on in modes:
            set_recompute(model, on)
            peak, wall = peak_of(model, batch)
            reps = int(max(1, min(10, share // max(wall, 1e-3))))
            ms = timed(model, batch, reps)
            f = formula(cfg, dt, kind == "LoRA", on, L)
            got[on] = (peak, ms, f)
            lines.append(f"{kind:9s}  {name:8s}  {'on ' if on else 'off'}        {gib(f)}      {gib(peak)}  {(f'{peak / f:12.2f}' if f else '           -')}  "
                         f"{ms:7.1f}  {reps:4d}")
            print(lines[-1], flush=True)
        if True in got:
            (p0, m0, f0), (p1, m1, f1) = got[False], got[True]
            summary.append(f"{kind:9s}  {name:8s}  peak on / off {p1 / p0:5.3f} (formula {f1 / f0:5.3f})   step on / off {m1 / m0:5.3f}")
            # the largest batch under recompute, by doubling; a step is expected to take at most 2.5 x the step at half its batch
            best, why, nb, last = (1, got[True][0]), f"reached --max_batch {a.max_batch}", 2, m1 * 1e-3
            per_case = left() / (len(cases) - cases.index((kind, dt))) - 5.0
            t_case = time.time()
            while nb <= a.max_batch:
                if 2.5 * last > per_case - (time.time() - t_case):
                    why = f"stopped for time before batch {nb} (not a failure: batch {nb} was not tried)"
                    break
                try:
                    wide = inputs(kind, nb, L)
                    peak, last = peak_of(model, wide)
                except torch.OutOfMemoryError as e:                      # a failed allocation: the host refused, the device is as it was
                    why = f"batch {nb} failed to allocate: {str(e).splitlines()[0][:160]}"
                    break
                except RuntimeError as e:                                # anything else ends the run: nothing more is started on the device
                    why = f"batch {nb} failed, run ended: {str(e).splitlines()[0][:200]}"
                    ended = True
                    break
                best = (nb, peak)
                nb *= 2
            if not ended:
                model.zero_grad(set_to_none=True)
            f = formula(cfg, dt, kind == "LoRA", True, L)
            search.append(f"{kind:9s}  {name:8s}  largest batch run with recompute on: {best[0]:2d} (peak {gib(best[1]).strip()} GiB, formula "
                          f"{gib(best[0] * f).strip()} GiB); {why}")
            print(search[-1], flush=True)
        if ended:
            break
        del model, batch
        torch.cuda.empty_cache()
    text = "\n".join(lines + (["#"] + ["# " + s for s in summary] + ["#"] + ["# " + s for s in search] if summary else [])
                     + [f"# run time {time.time() - start:.0f} s of a budget of {a.budget:.0f} s"]) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)
    if ended:
        raise SystemExit(1)


if __name__ == "__main__":
    main()
