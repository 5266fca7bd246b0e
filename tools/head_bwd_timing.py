"""Time the loss head's backward (include/pcad_bwd.h pcad_loss_head_bwd) next to its forward (pcad_loss_head) on the same tensors, and
next to the backward of the torch composition it replaces:
    ops.rms_norm_fn (norm_f, differentiable) -> F.linear x 2 with the flips -> F.cross_entropy
B = 256 windows x L = 512 x D = 1024, bf16 with an fp32 residual stream and fp32 / fp32, 15 % and 100 % of the positions labelled.
Tensors generated on the device; HIP events around each call on the current stream, warm-up rounds first, one round = forward then
backward, the figure of a series is the median over the rounds.  Bytes are those the formula needs: the labelled rows of h and res
read, every row of dh and dres written, the parameter partials written and read once; the rate is given as a fraction of the 8 TB/s HBM
peak DESIGN.md §8 quotes.

    python tools/head_bwd_timing.py [--out profiles/head_bwd_timing.txt] [--steps 20] [--warmup 3]
"""
import argparse
import math
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

from plantcaduceus_amd import engine, ops  # noqa: E402

HBM_PEAK = 8.0e12      # bytes / s: the spec figure DESIGN.md §8 measures kernels against
COMP = [0, 1, 2, 6, 5, 4, 3, 7]


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def series(fwd, bwd, warmup, steps):
    for _ in range(warmup):
        fwd()
        bwd()
    torch.cuda.synchronize()
    tf, tb = [], []
    for _ in range(steps):
        tf.append(event_ms(fwd))
        tb.append(event_ms(bwd))
    return statistics.median(tf), statistics.median(tb), min(tb), max(tb)


def aligned(t):
    return (t.data_ptr() + 255) // 256 * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=256)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--D", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("head_bwd_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, blib = engine.load_library(), engine.load_bwd_library()
    B, L, D = a.B, a.L, a.D
    rows = 2 * B * L
    st = torch.cuda.current_stream().cuda_stream
    nb = blib.pcad_loss_head_bwd_scratch_bytes(B, L, D)
    nseg = (L + ops.LOSS_SEG - 1) // ops.LOSS_SEG
    lines = [f"# loss head backward vs forward vs the torch composition's backward, {torch.cuda.get_device_name(0)}, build {lib.pcad_build_hash().decode()}",
             f"# B={B} L={L} D={D} (segment {ops.LOSS_SEG}); HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds (forward, backward alternating)",
             f"# bytes by the formula: labelled rows of h and res read, all rows of dh and dres written, B ceil(L / {ops.LOSS_SEG}) rows of 9 D partials written "
             f"and read; of_peak = of {HBM_PEAK / 1e12:.0f} TB/s;  scratch {nb / 2 ** 20:.0f} MiB",
             "# composed = ops.rms_norm_fn -> F.linear x 2 with flips -> F.cross_entropy, differentiated by torch (its forward builds the graph)",
             "dtypes     labelled  fwd_ms   bwd_ms   bwd_GB   bwd_TB/s  of_peak  bwd_min_ms  bwd_max_ms  composed_fwd_ms  composed_bwd_ms  composed/fused"]
    comp = torch.tensor(COMP, dtype=torch.int32, device=dev)
    for dt in (torch.bfloat16, torch.float32):
        es, code = torch.empty((), dtype=dt).element_size(), engine._DT[dt]
        g = torch.Generator(device=dev).manual_seed(1)
        h = torch.randn(rows, D, device=dev, generator=g).to(dt)
        res = torch.randn(rows, D, device=dev, generator=g) * 0.5 + 0.25
        wn = torch.rand(D, device=dev, generator=g) + 0.5
        emb = (torch.randn(8, D, device=dev, generator=g) * (3.0 / math.sqrt(D))).to(dt)
        e32 = emb.float().contiguous()
        wt = torch.rand(B, L, device=dev, generator=g) + 0.5
        dsum = torch.rand(B, device=dev, generator=g) + 0.5
        sums = torch.empty(B, 4, device=dev)
        dh, dres = torch.empty_like(h), torch.empty_like(res)
        dwn, demb = torch.empty(D, device=dev), torch.empty(8, D, device=dev)
        fscratch = torch.empty(lib.pcad_loss_head_scratch_bytes(B, L) + 256, dtype=torch.uint8, device=dev)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        fsp, sp = aligned(fscratch), aligned(scratch)
        for frac in (0.15, 1.0):
            lab = torch.randint(0, 8, (B, L), device=dev, generator=g)
            if frac < 1.0:
                lab = torch.where(torch.rand(B, L, device=dev, generator=g) < frac, lab, torch.full_like(lab, -100))
            lab32 = lab.to(torch.int32).contiguous()
            nlab = int((lab >= 0).sum().item())

            def fwd():
                engine._check(lib.pcad_loss_head(h.data_ptr(), res.data_ptr(), wn.data_ptr(), e32.data_ptr(), comp.data_ptr(), lab32.data_ptr(),
                                                 wt.data_ptr(), -100, sums.data_ptr(), None, None, B, L, D, 1e-5, None, None, code, 0, 0, fsp,
                                                 fscratch.numel() - 256, st), "pcad_loss_head")

            def bwd():
                engine._check(blib.pcad_loss_head_bwd(h.data_ptr(), res.data_ptr(), wn.data_ptr(), e32.data_ptr(), comp.data_ptr(), lab32.data_ptr(),
                                                      wt.data_ptr(), -100, dsum.data_ptr(), None, dh.data_ptr(), dres.data_ptr(), dwn.data_ptr(),
                                                      demb.data_ptr(), sp, nb, B, L, D, 1e-5, code, 0, st), "pcad_loss_head_bwd")
            mf, mb, lo, hi = series(fwd, bwd, a.warmup, a.steps)
            assert bool(torch.isfinite(dwn).all()) and bool(torch.isfinite(demb).all()) and bool(torch.isfinite(dh.float()).all())
            # the composition: leaves h, res, norm weight, embedding
            lv = [h.view(2 * B, L, D).clone().requires_grad_(True), res.view(2 * B, L, D).clone().requires_grad_(True), wn.clone().requires_grad_(True),
                  emb.clone().requires_grad_(True)]
            box = {}

            def cfwd():
                for t in lv:
                    t.grad = None
                H = ops.rms_norm_fn(lv[0], lv[2], None, lv[1], 1e-5, prenorm=False, residual_in_fp32=True)
                lg = (F.linear(H[:B], lv[3]) + F.linear(H[B:].flip(1), lv[3][comp.long()])).float()
                nll = F.cross_entropy(lg.view(-1, 8), lab.view(-1), reduction="none", ignore_index=-100).view(B, L)
                box["loss"] = ((nll * wt).sum(1) * dsum).sum()

            def cbwd():
                box.pop("loss").backward()
            cf, cb, _, _ = series(cfwd, cbwd, a.warmup, a.steps)
            del lv, box
            torch.cuda.empty_cache()
            nbytes = 2 * nlab * D * (es + 4) + rows * D * (es + 4) + 2 * B * nseg * 9 * D * 4
            rate = nbytes / (mb * 1e-3)
            lines.append(f"{str(dt).split('.')[-1][:8]:8s}/f32 {100 * nlab / (B * L):7.1f}%  {mf:7.3f}  {mb:7.3f}  {nbytes / 1e9:7.3f}  {rate / 1e12:8.2f}  "
                         f"{rate / HBM_PEAK:7.2f}  {lo:10.3f}  {hi:10.3f}  {cf:15.3f}  {cb:15.3f}  {cb / mb:14.2f}")
            print(lines[-1], flush=True)
        del h, res, dh, dres, scratch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
