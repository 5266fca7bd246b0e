"""Time the fused optimizer step (include/pcad_bwd.h pcad_adamw_step through plantcaduceus_amd.optim.AdamW) on the l32 parameter set
with random gradients, next to the torch step it replaces:
    torch.nn.utils.clip_grad_norm_(params, 1.0) -> torch.optim.AdamW(fused=True).step()       (foreach=True where fused is unavailable)
in fp32 (the parameter is its own master) and in bf16 with fp32 master weights (torch: fp32 parameters only - it has no master-weight
form, so the bf16 row is set beside torch's fp32 row).  Also the one-launch zero_grad against torch's zero_grad(set_to_none=False).
Tensors generated on the device; HIP events around each call on the current stream, warm-up rounds first, the figure of a series is
the median over the rounds.  Bytes are those the formula needs per element: the gradient read once for the norm, then gradient, master,
exp_avg and exp_avg_sq read and the last three written (fp32: 4 + 28 B; bf16 + master: 2 + 26 + 2 B for the rounded parameter); the rate
is given as a fraction of the 8 TB/s HBM peak DESIGN.md §8 quotes.  The working set (several GB) is far beyond the 256 MiB of last-level cache.

    python tools/adamw_timing.py [--out profiles/adamw_timing.txt] [--steps 20] [--warmup 3] [--size l32]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine, ops, optim  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config  # noqa: E402
from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s: the spec figure DESIGN.md §8 measures kernels against


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(fn, warmup, steps):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    t = [event_ms(fn) for _ in range(steps)]
    return statistics.median(t), min(t), max(t)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="l32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("adamw_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = "cuda:0"
    lib = engine.load_library()
    cfg = make_config(a.size)
    lines = []
    torch_ms = {}
    for dt in (torch.float32, torch.bfloat16):
        model = TrainableCaduceusForMaskedLM(cfg, dtype=dt, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        params = [p for _, p in model.named_parameters()]
        with torch.no_grad():
            for p in params:
                p.copy_(torch.randn(p.shape, device=dev, generator=g) * 0.05)
                p.grad = (torch.randn(p.shape, device=dev, generator=g) * 0.01).to(dt)
        n = sum(p.numel() for p in params)
        opt = optim.AdamW(model.named_parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
        tab = opt.table()
        if not lines:
            lines += [f"# fused AdamW step (clip + update, 3 launches) vs clip_grad_norm_ + torch.optim.AdamW, {torch.cuda.get_device_name(0)}, "
                      f"build {lib.pcad_build_hash().decode()}",
                      f"# {a.size}: {len(params)} tensors, {n} elements, smallest {min(p.numel() for p in params)}, largest {max(p.numel() for p in params)}; "
                      f"chunk {ops.OPTIM_CHUNK}: {tab.chunks} chunks; HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds",
                      f"# bytes by the formula per element: fp32 4 (norm) + 28 (update); bf16 + fp32 master 2 + 28; of_peak = of {HBM_PEAK / 1e12:.0f} TB/s",
                      "form             step_ms  min_ms   max_ms   GB      TB/s   of_peak  zero_ms  torch_step_ms  torch_form     torch/fused  torch_zero_ms"]
        ms, lo, hi = series(opt.step, a.warmup, a.steps)
        st = opt.state()
        assert st["finite"] == 1 and st["skipped"] == 0 and all(bool(torch.isfinite(p).all()) for p in params[:8]), st
        for p in params:                                   # zero_grad is timed on non-zero gradients (the values do not matter to a store)
            p.grad.normal_(generator=g)
        zms, _, _ = series(opt.zero_grad, a.warmup, a.steps)
        assert all(not bool(p.grad.any()) for p in params[:8])
        per = 32 if dt == torch.float32 else 30
        nbytes = per * n
        rate = nbytes / (ms * 1e-3)
        del opt, tab
        if dt == torch.float32:                            # the torch step on the same tensors: fp32 parameters, fp32 gradients
            with torch.no_grad():
                for p in params:
                    p.grad = torch.randn(p.shape, device=dev, generator=g) * 0.01
            form = "fused=True"
            try:
                topt = torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01, fused=True)
            except Exception:
                form, topt = "foreach=True", torch.optim.AdamW(params, lr=1e-4, weight_decay=0.01, foreach=True)

            def tstep():
                torch.nn.utils.clip_grad_norm_(params, 1.0)
                topt.step()
            torch_ms["step"], _, _ = series(tstep, a.warmup, a.steps)
            torch_ms["zero"], _, _ = series(lambda: topt.zero_grad(set_to_none=False), a.warmup, a.steps)
            torch_ms["form"] = form
            del topt
        name = "fp32" if dt == torch.float32 else "bf16+fp32 master"
        lines.append(f"{name:16s} {ms:7.3f}  {lo:7.3f}  {hi:7.3f}  {nbytes / 1e9:6.3f}  {rate / 1e12:5.2f}  {rate / HBM_PEAK:7.2f}  {zms:7.3f}  "
                     f"{torch_ms['step']:13.3f}  {torch_ms['form'] + (' (fp32)' if dt != torch.float32 else ''):13s}  {torch_ms['step'] / ms:11.2f}  "
                     f"{torch_ms['zero']:13.3f}")
        print(lines[-1], flush=True)
        del model, params
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
