"""Time the weight-gradient kernel of the fp32 main gradients (include/pcad_bwd.h pcad_linear_wgrad through plantcaduceus_amd.ops.linear_wgrad
with accumulate=True) on the eight projection shapes of l32 and PlantCAD2 Small at M = 8 192 and M = 65 536 rows, next to
what the stock path needs for the same effect: `dy.t() @ x` in bf16 (hipBLASLt) plus the add of its bf16 result into the fp32 buffer.
Then one `pretrain` optimizer step in bf16 (forward, backward, fused AdamW, zero_grad on random windows) with and without
fp32_grad_accumulation.

Operands generated on the device; HIP events around each call on the current stream, warm-up rounds first, the figure of a series is the
median over the rounds, one process.  A fat shape (in_proj, out_proj) is reported in TFLOP/s = 2 M N K / time as a fraction of the 2.5 PFLOP/s
bf16 peak DESIGN.md §8 quotes; a skinny one (x_proj, dt_proj) in TB/s over the bytes the product needs once - dy and x read, dw read and
written - as a fraction of 8 TB/s.  Nothing here is a gate: the feature's claim is precision, and a kernel slower than hipBLASLt is recorded.

    python tools/linear_wgrad_timing.py [--out profiles/linear_wgrad_timing.txt] [--steps 20] [--warmup 3] [--size l32 --batch 8 --seq_len 512]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402

from adamw_timing import HBM_PEAK, series  # noqa: E402
from plantcaduceus_amd import engine, ops, optim  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402
from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM  # noqa: E402

MFMA_PEAK = 2.5e15      # bf16 flop / s: the figure DESIGN.md §8 measures the GEMMs against
SHAPES = [("in_proj l32", 4096, 1024, True), ("out_proj l32", 1024, 2048, True), ("x_proj l32", 96, 2048, False), ("dt_proj l32", 2048, 64, False),
          ("in_proj Small", 3072, 768, True), ("out_proj Small", 768, 1536, True), ("x_proj Small", 80, 1536, False), ("dt_proj Small", 1536, 48, False)]


def operator_lines(a, dev):
    lines = ["projection      N     K     M       slabs  kernel_ms  min_ms   max_ms   rate          of_peak  stock_ms  stock / kernel"]
    g = torch.Generator(device=dev).manual_seed(1)
    for name, N, K, fat in SHAPES:
        for M in (8192, 65536):
            dy = (torch.randn((M, N), device=dev, generator=g) / M ** 0.5).to(torch.bfloat16)
            x = torch.randn((M, K), device=dev, generator=g).to(torch.bfloat16)
            main = torch.zeros((N, K), device=dev)
            ms, lo, hi = series(lambda: ops.linear_wgrad(dy, x, out=main, accumulate=True), a.warmup, a.steps)
            stock_ms, _, _ = series(lambda: main.add_(dy.t() @ x), a.warmup, a.steps)
            if fat:
                rate = 2.0 * M * N * K / (ms * 1e-3)
                shown, frac = f"{rate / 1e12:7.1f} TFLOP/s", rate / MFMA_PEAK
            else:
                rate = (2.0 * M * (N + K) + 8.0 * N * K) / (ms * 1e-3)
                shown, frac = f"{rate / 1e12:7.2f} TB/s   ", rate / HBM_PEAK
            lines.append(f"{name:14s}  {N:4d}  {K:4d}  {M:6d}  {ops.linear_wgrad_slabs(M, N, K)[0]:5d}  {ms:9.3f}  {lo:7.3f}  {hi:7.3f}  {shown}  {frac:7.3f}  "
                         f"{stock_ms:8.3f}  {stock_ms / ms:14.2f}")
            print(lines[-1], flush=True)
            del dy, x, main
    return lines


def step_lines(a, dev):
    """one optimizer step of the pretrain loop at accumulation 1: forward + backward + AdamW.step + zero_grad, on random windows"""
    cfg = make_config(a.size)
    g = torch.Generator().manual_seed(2)
    ids = torch.randint(3, 7, (a.batch, a.seq_len), generator=g)
    labels = torch.where(torch.rand(ids.shape, generator=g) < 0.15, ids, torch.full_like(ids, -100)).to(torch.int32).to(dev)
    ids = ids.to(torch.int32).to(dev)
    sd = synthetic_state_dict(cfg, seed=3, stress=False)
    lines = [f"# one pretrain step, {a.size}, bf16, batch {a.batch} x {a.seq_len} (M = {2 * a.batch * a.seq_len} rows), accumulation 1; "
             f"1 warm-up step, median of {a.step_rounds}",
             "fp32_grad_accumulation  step_ms   min_ms    max_ms"]
    for flag in (False, True):
        model = TrainableCaduceusForMaskedLM(cfg, dtype=torch.bfloat16, device=dev)
        model.load_state_dict(sd)
        opt = optim.AdamW(model.named_parameters(), lr=1e-5, weight_decay=0.01, max_grad_norm=1.0, fp32_grad_accumulation=flag)

        def step():
            model(ids, labels).loss.backward()
            opt.step()
            opt.zero_grad()
        ms, lo, hi = series(step, 1, a.step_rounds)
        st = opt.state()
        assert st["finite"] == 1 and st["skipped"] == 0, st
        lines.append(f"{str(flag):22s}  {ms:8.2f}  {lo:8.2f}  {hi:8.2f}")
        print(lines[-1], flush=True)
        del opt, model
        torch.cuda.empty_cache()
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="l32")
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--seq_len", type=int, default=512, help="window length (l32's windows are 512 bp: batch 8 is M = 8 192 rows)")
    ap.add_argument("--step_rounds", type=int, default=5, help="timed pretrain steps per setting, after one warm-up step")
    ap.add_argument("--no_step", action="store_true", help="operators only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("linear_wgrad_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = "cuda:0"
    lib = engine.load_library()
    lines = [f"# pcad_linear_wgrad (accumulate into fp32) against dy.t() @ x in bf16 + the fp32 add, {torch.cuda.get_device_name(0)}, build "
             f"{lib.pcad_build_hash().decode()}",
             f"# HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds; fat shapes: 2 M N K flop of {MFMA_PEAK / 1e15:.1f} PFLOP/s; skinny: "
             f"2 M (N + K) + 8 N K bytes of {HBM_PEAK / 1e12:.0f} TB/s"]
    lines += operator_lines(a, dev)
    if not a.no_step:
        try:
            lines += step_lines(a, dev)
        except torch.OutOfMemoryError as e:
            lines.append(f"# one pretrain step at {a.size}, batch {a.batch} x {a.seq_len}: not measured (out of memory: {str(e)[:80]})")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
