"""Time the pooled classification head's backward (include/pcad_bwd.h pcad_pooled_head_bwd) next to its forward (pcad_pooled_head) on the
same tensors, and next to torch autograd through a torch restatement of the same head on the same device:
    v = h + res -> RMSNorm in fp32, rounded to the model dtype -> mean over each strand's rows -> F.linear(score) per strand -> average
PlantCAD2 Small width (D = 768), B = 4 windows x L = 8 192, num_labels 2, mean pooling, fp32 / fp32 and bf16 with an fp32 residual stream.
Tensors generated on the device; HIP events around each call on the current stream, warm-up rounds first, one round = forward then
backward, the figure of a series is the median over the rounds.  Bytes are those the formula needs: every row of h and res read, every
row of dh and dres written, the dnorm_weight partials written and read once; the rate is given as a fraction of the 8 TB/s HBM peak
DESIGN.md §8 quotes.

    python tools/pooled_head_bwd_timing.py [--out profiles/pooled_head_bwd_timing.txt (the default)] [--steps 20] [--warmup 3]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "pooled_head_bwd_timing.txt"))
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--B", type=int, default=4)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--D", type=int, default=768)
    ap.add_argument("--NL", type=int, default=2)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("pooled_head_bwd_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, blib = engine.load_library(), engine.load_bwd_library()
    B, L, D, NL = a.B, a.L, a.D, a.NL
    rows = 2 * B * L
    st = torch.cuda.current_stream().cuda_stream
    nb = blib.pcad_pooled_head_bwd_scratch_bytes(B, L, D, 0)
    nf = lib.pcad_pooled_head_scratch_bytes(B, L, D, 0)
    nseg = (L + ops.POOL_BWD_SEG - 1) // ops.POOL_BWD_SEG
    lines = [f"# pooled head backward vs forward vs torch autograd through a torch restatement, {torch.cuda.get_device_name(0)}, build {lib.pcad_build_hash().decode()}",
             f"# B={B} L={L} D={D} NL={NL} mean pooling (segment {ops.POOL_BWD_SEG}); HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds "
             "(forward, backward alternating)",
             f"# bytes by the formula: all rows of h and res read, all rows of dh and dres written, 2 B ceil(L / {ops.POOL_BWD_SEG}) rows of D partials written and "
             f"read; of_peak = of {HBM_PEAK / 1e12:.0f} TB/s;  scratch {nb} bytes",
             "# torch = v = h + res, RMSNorm in fp32 rounded to the model dtype, mean per strand, F.linear per strand, average; differentiated by torch",
             "dtypes        fwd_ms   bwd_ms   bwd_GB   bwd_TB/s  of_peak  bwd_min_ms  bwd_max_ms  torch_fwd_ms  torch_bwd_ms  torch/fused"]
    for dt in (torch.float32, torch.bfloat16):
        es, code = torch.empty((), dtype=dt).element_size(), engine._DT[dt]
        g = torch.Generator(device=dev).manual_seed(1)
        h = torch.randn(rows, D, device=dev, generator=g).to(dt)
        res = torch.randn(rows, D, device=dev, generator=g) * 0.5 + 0.25
        wn = torch.rand(D, device=dev, generator=g) + 0.5
        W = (torch.randn(NL, D, device=dev, generator=g) * (3.0 / math.sqrt(D))).to(dt)
        W32 = W.float().contiguous()
        dl = torch.randn(B, NL, device=dev, generator=g)
        lg, pooled = torch.empty(B, NL, device=dev), torch.empty(B, 2, D, device=dev)
        dh, dres = torch.empty_like(h), torch.empty_like(res)
        dwn, dW = torch.empty(D, device=dev), torch.empty(NL, D, device=dev)
        fscratch = torch.empty(nf + 256, dtype=torch.uint8, device=dev)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        fsp, sp = aligned(fscratch), aligned(scratch)

        def fwd():
            engine._check(lib.pcad_pooled_head(h.data_ptr(), res.data_ptr(), wn.data_ptr(), W32.data_ptr(), NL, pooled.data_ptr(), lg.data_ptr(), B, L, D,
                                               1e-5, 0, None, None, code, 0, 0, fsp, nf, st), "pcad_pooled_head")

        def bwd():
            engine._check(blib.pcad_pooled_head_bwd(h.data_ptr(), res.data_ptr(), wn.data_ptr(), W32.data_ptr(), pooled.data_ptr(), dl.data_ptr(),
                                                    dh.data_ptr(), dres.data_ptr(), dwn.data_ptr(), dW.data_ptr(), sp, nb, B, L, D, NL, 1e-5, 0, code, 0,
                                                    st), "pcad_pooled_head_bwd")
        mf, mb, lo, hi = series(fwd, bwd, a.warmup, a.steps)
        assert bool(torch.isfinite(dwn).all()) and bool(torch.isfinite(dW).all()) and bool(torch.isfinite(dh.float()).all())
        # the torch restatement: leaves h, res, norm weight, score weight
        lv = [h.view(2 * B, L, D).clone().requires_grad_(True), res.view(2 * B, L, D).clone().requires_grad_(True), wn.clone().requires_grad_(True),
              W.clone().requires_grad_(True)]
        box = {}

        def tfwd():
            for t in lv:
                t.grad = None
            v = lv[0].float() + lv[1]
            o = (v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + 1e-5) * lv[2]).to(dt)
            p = o.float().mean(1).to(dt)                                    # [2B, D]
            s = F.linear(p, lv[3])                                           # [2B, NL]
            box["loss"] = (((s[:B] + s[B:]) / 2).float() * dl).sum()

        def tbwd():
            box.pop("loss").backward()
        cf, cb, _, _ = series(tfwd, tbwd, a.warmup, a.steps)
        del lv, box
        torch.cuda.empty_cache()
        nbytes = 2 * rows * D * (es + 4) + 2 * 2 * B * nseg * D * 4
        rate = nbytes / (mb * 1e-3)
        lines.append(f"{str(dt).split('.')[-1][:8]:8s}/f32  {mf:7.3f}  {mb:7.3f}  {nbytes / 1e9:7.3f}  {rate / 1e12:8.2f}  {rate / HBM_PEAK:7.2f}  "
                     f"{lo:10.3f}  {hi:10.3f}  {cf:12.3f}  {cb:12.3f}  {cb / mb:11.2f}")
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
