"""Time the LoRA dropout kernels (include/pcad_bwd.h pcad_lora_down / pcad_lora_down_bwd) on the six adapted input widths of
PlantCAD2 Small and l32 at M = 8 192 and M = 65 536 rows, bf16, r = 8, p = 0.1, next to the stock sequence for the same effect on the
same device: `F.dropout(x, p) @ A^T` in bf16 and its autograd backward (dx and dA from u).  Then one fine-tuning step (forward +
backward of TrainableCaduceusForSequenceClassification, the model `lora_predict train` runs) at Small, one window of L = 8 192, bf16,
with lora_dropout 0 - the calls the parent commit makes - and 0.1, with its peak memory by tools/train_memory.py's method.

The C entries are called directly on preallocated buffers, so that the events bracket the kernels and not the wrappers' allocations.
Rates are over the bytes each call needs once - forward: x read; backward: x read, dx read and written - against the 8 TB/s DESIGN.md §8
quotes.  HIP events, warm-up rounds first, median of the rounds, one process.  Nothing here is a gate.

    python tools/lora_dropout_timing.py [--out profiles/lora_dropout_timing.txt] [--steps 20] [--warmup 3] [--no_step]
"""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from adamw_timing import HBM_PEAK, series  # noqa: E402
from plantcaduceus_amd import engine, ops  # noqa: E402
from plantcaduceus_amd.engine import _stream_ptr  # noqa: E402

WIDTHS = [("in_proj Small", 768), ("x_proj Small", 1536), ("out_proj Small", 1536), ("in_proj l32", 1024), ("x_proj l32", 2048), ("out_proj l32", 2048)]
R, P, SEED = 8, 0.1, 42
BF = torch.bfloat16


def operator_lines(a, dev):
    lib = engine.load_bwd_library()
    lines = ["projection       K     M      slabs  fwd_ms   TB/s  of_8  stock_fwd_ms  bwd_ms   TB/s  of_8  stock_bwd_ms  stock/kernel fwd  bwd"]
    g = torch.Generator(device=dev).manual_seed(1)
    for name, K in WIDTHS:
        for M in (8192, 65536):
            x = torch.randn((M, K), device=dev, generator=g).to(BF)
            A = (torch.rand((R, K), device=dev, generator=g) * 2 - 1) / K ** 0.5
            u = torch.randn((M, R), device=dev, generator=g)
            dx = torch.randn((M, K), device=dev, generator=g).to(BF)
            t = torch.empty((M, R), device=dev)
            dA = torch.empty((R, K), device=dev)
            nb = lib.pcad_lora_down_bwd_scratch_bytes(M, K, R)
            scratch, sp = ops._scratch(nb, dev)
            args = (float(P), SEED, 7, 1)

            def fwd():
                ops._check(lib.pcad_lora_down(x.data_ptr(), K, A.data_ptr(), t.data_ptr(), M, K, R, *args, _stream_ptr()), "pcad_lora_down")

            def bwd():
                ops._check(lib.pcad_lora_down_bwd(x.data_ptr(), K, A.data_ptr(), u.data_ptr(), dx.data_ptr(), K, dA.data_ptr(), sp, nb, M, K, R,
                                                  *args, _stream_ptr()), "pcad_lora_down_bwd")
            f_ms, _, _ = series(fwd, a.warmup, a.steps)
            b_ms, _, _ = series(bwd, a.warmup, a.steps)
            # the stock sequence: a dropped copy of x, the rank-r product, and autograd's backward through both
            xs, As, ub = x.clone().requires_grad_(True), A.to(BF).requires_grad_(True), u.to(BF)
            sf_ms, _, _ = series(lambda: F.linear(F.dropout(xs, P), As), a.warmup, a.steps)
            ts = F.linear(F.dropout(xs, P), As)
            sb_ms, _, _ = series(lambda: torch.autograd.grad(ts, (xs, As), ub, retain_graph=True), a.warmup, a.steps)
            f_rate, b_rate = 2.0 * M * K / (f_ms * 1e-3), 6.0 * M * K / (b_ms * 1e-3)
            lines.append(f"{name:14s}  {K:4d}  {M:6d}  {ops.lora_down_bwd_slabs(M, K, R)[0]:5d}  {f_ms:6.3f}  {f_rate / 1e12:5.2f}  {f_rate / HBM_PEAK:4.2f}  "
                         f"{sf_ms:12.3f}  {b_ms:6.3f}  {b_rate / 1e12:5.2f}  {b_rate / HBM_PEAK:4.2f}  {sb_ms:12.3f}  {sf_ms / f_ms:16.2f}  {sb_ms / b_ms:4.2f}")
            print(lines[-1], flush=True)
            del x, A, u, dx, t, dA, scratch, xs, As, ub, ts
            torch.cuda.empty_cache()
    return lines


def step_lines(a, dev):
    """forward + backward of the fine-tuning model at Small, one window of L, bf16, lora_B = 0.05 N(0, 1): time and peak memory"""
    import train_memory as TM
    from plantcaduceus_amd import training
    from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
    cfg = make_config(a.size)
    sd = synthetic_state_dict(cfg, stress=False)
    M, n_proj = 2 * a.L, cfg.n_layer * 2 * 3
    lines = [f"# one fine-tuning step (forward + backward), {a.size}, bf16, one window of L = {a.L} (M = {M} rows per projection, {n_proj} adapted "
             f"projections), recompute off; 1 warm-up step, median of {a.step_rounds}; peak = max_memory_allocated of the step above the bytes before it",
             "lora_dropout  step_ms  peak_GiB"]
    peaks = {}
    for p in (0.0, P):
        m = training.TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", dtype=BF, device=dev, lora_dropout=p)
        m.load_trunk({k: v for k, v in sd.items() if k.startswith("caduceus.")})
        gen = torch.Generator().manual_seed(31)
        with torch.no_grad():
            for k, q in m.named_parameters():
                if ".lora_B." in k:
                    q.copy_((torch.randn(q.shape, generator=gen) * 0.05).to(dev))
        m.train()
        TM.step(m, TM.inputs("LoRA", 1, 64))
        batch = TM.inputs("LoRA", 1, a.L)
        peak, _ = TM.peak_of(m, batch)
        ms = TM.timed(m, batch, a.step_rounds)
        peaks[p] = peak
        lines.append(f"{p:12.1f}  {ms:7.1f}  {peak / 2 ** 30:8.3f}")
        print(lines[-1], flush=True)
        del m, batch
        torch.cuda.empty_cache()
    extra, t_bytes, x_bytes = peaks[P] - peaks[0.0], n_proj * M * R * 4, M * cfg.d_inner * 2
    lines.append(f"# peak with dropout - without: {extra / 2 ** 20:.1f} MiB; the saved t tensors, {n_proj} x M r 4 bytes: {t_bytes / 2 ** 20:.1f} MiB; one "
                 f"[M, E] bf16 tensor: {x_bytes / 2 ** 20:.1f} MiB, a dropped copy of every LoRA input per layer: {cfg.n_layer * 2 * (cfg.d_model + 2 * cfg.d_inner) * M * 2 / 2 ** 20:.1f} MiB")
    return lines


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--size", default="pc2-small")
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--step_rounds", type=int, default=3)
    ap.add_argument("--no_step", action="store_true", help="operators only")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("lora_dropout_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = "cuda:0"
    lines = [f"# pcad_lora_down / pcad_lora_down_bwd (bf16, r = {R}, p = {P}) against F.dropout + the rank-r matmuls in bf16, "
             f"{torch.cuda.get_device_name(0)}, build {engine.load_library().pcad_build_hash().decode()}",
             f"# HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds; forward bytes 2 M K, backward bytes 6 M K, of {HBM_PEAK / 1e12:.0f} TB/s"]
    lines += operator_lines(a, dev)
    if not a.no_step:
        try:
            lines += step_lines(a, dev)
        except torch.OutOfMemoryError as e:
            lines.append(f"# the fine-tuning step at {a.size}, L = {a.L}: not measured (out of memory: {str(e)[:80]})")
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
