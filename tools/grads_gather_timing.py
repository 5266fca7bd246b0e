"""Time the gathering of every gradient into one fp32 buffer (include/pcad_bwd.h pcad_grads_gather through plantcaduceus_amd.ops.grads_gather;
DESIGN.md §4r) on the l32 parameter set with random gradients, fp32 and bf16, next to the optimizer step that follows it on the buffer
(optim.AdamW(reducer=GradReducer(None, ...)).step(): gather + the three launches of pcad_adamw_step with fp32 gradients; no collective
at a world of one) and to the plain step of tools/adamw_timing.py on the same tensors.
Tensors generated on the device; HIP events around each call on the current stream, warm-up rounds first, the figure of a series is the
median over the rounds.  Bytes of the gather are those the copy needs per element: the gradient read once, its fp32 image written once
(fp32: 4 + 4 B; bf16: 2 + 4 B); the rate is given as a fraction of the 8 TB/s HBM peak DESIGN.md §8 quotes.  The working set (1.8 / 1.35 GB)
is far beyond the 256 MiB of last-level cache.

    python tools/grads_gather_timing.py [--out profiles/grads_gather_timing.txt] [--steps 20] [--warmup 3] [--size l32]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from adamw_timing import HBM_PEAK, series  # noqa: E402
from plantcaduceus_amd import ddp, engine, ops, optim  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config  # noqa: E402
from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="l32")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("grads_gather_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = "cuda:0"
    lib = engine.load_library()
    cfg = make_config(a.size)
    lines = []
    for dt in (torch.float32, torch.bfloat16):
        model = TrainableCaduceusForMaskedLM(cfg, dtype=dt, device=dev)
        g = torch.Generator(device=dev).manual_seed(1)
        params = [p for _, p in model.named_parameters()]
        with torch.no_grad():
            for p in params:
                p.copy_(torch.randn(p.shape, device=dev, generator=g) * 0.05)
                p.grad = (torch.randn(p.shape, device=dev, generator=g) * 0.01).to(dt)
        n = sum(p.numel() for p in params)
        plain = optim.AdamW(model.named_parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0)
        plain_ms, _, _ = series(plain.step, a.warmup, a.steps)
        del plain
        opt = optim.AdamW(model.named_parameters(), lr=1e-4, weight_decay=0.01, max_grad_norm=1.0, reducer=ddp.GradReducer(None, dev))
        tab, flat = opt.table(), opt.reducer.grads
        offsets, total = tab.flat_plan()
        if not lines:
            lines += [f"# every gradient into one fp32 buffer (pcad_grads_gather, 1 launch) and the step on it, {torch.cuda.get_device_name(0)}, "
                      f"build {lib.pcad_build_hash().decode()}",
                      f"# {a.size}: {len(params)} tensors, {n} elements, buffer {total} + {ddp.TAIL} fp32 elements ({total - n} of padding); "
                      f"chunk {ops.OPTIM_CHUNK}: {tab.chunks} chunks; HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds",
                      f"# bytes of the gather by the formula per element: fp32 4 + 4; bf16 2 + 4; of_peak = of {HBM_PEAK / 1e12:.0f} TB/s; "
                      "flat_step = gather + adamw_step on the buffer (world 1: no collective); plain_step = adamw_step on the gradients",
                      "gradients  gather_ms  min_ms   max_ms   GB      TB/s   of_peak  flat_step_ms  plain_step_ms  flat - plain_ms"]
        dev_off = tab.flat_offsets()
        ms, lo, hi = series(lambda: ops.grads_gather(tab, flat, dev_off), a.warmup, a.steps)
        at = offsets[len(offsets) // 2]
        assert torch.equal(flat[at:at + 64], params[len(offsets) // 2].grad.reshape(-1)[:64].float())
        step_ms, _, _ = series(opt.step, a.warmup, a.steps)
        st = opt.state()
        assert st["finite"] == 1 and st["skipped"] == 0, st
        nbytes = (8 if dt == torch.float32 else 6) * n
        rate = nbytes / (ms * 1e-3)
        lines.append(f"{'fp32' if dt == torch.float32 else 'bf16':9s}  {ms:9.3f}  {lo:7.3f}  {hi:7.3f}  {nbytes / 1e9:6.3f}  {rate / 1e12:5.2f}  {rate / HBM_PEAK:7.2f}  "
                     f"{step_ms:12.3f}  {plain_ms:13.3f}  {step_ms - plain_ms:15.3f}")
        print(lines[-1], flush=True)
        del opt, tab, flat, model, params
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
