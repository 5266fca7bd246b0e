"""Time the conv and the add + RMSNorm backward operators (include/pcad_bwd.h) next to their forwards on the same tensors:
  conv   pcad_causal_conv1d_silu_bwd next to pcad_causal_conv1d_silu_dir, S = 256 strands x L = 512 x E = 2048 channels (l32's d_inner), both
         directions;
  norm   pcad_add_rmsnorm_bwd next to pcad_add_rmsnorm, rows = 131072 x D = 1024, with a residual (fp32 stream) and the prenorm gradient;
both dtypes.  Tensors generated on the device; HIP events around each call on the current stream, warm-up rounds first, one round =
forward then backward, the figure of a series is the median over the rounds.  Bytes are those the formulas need (every operand read
once, every output written once; the partial sums in the scratch are not counted), the rate is given as a fraction of the 8 TB/s HBM
peak DESIGN.md §8 quotes.

    python tools/block_bwd_timing.py [--out profiles/block_bwd_timing.txt] [--steps 20] [--warmup 3]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

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


def row(tag, dt, rows, mf, mb, lo, hi, fbytes, bbytes):
    rate = lambda nbytes, ms: nbytes / (ms * 1e-3)
    return (f"{tag:14s} {str(dt).split('.')[-1]:9s} {mf:7.3f}  {mf * 1e6 / rows:10.2f}  {rate(fbytes, mf) / 1e12:8.2f}  {rate(fbytes, mf) / HBM_PEAK:8.2f}  "
            f"{mb:7.3f}  {mb * 1e6 / rows:10.2f}  {rate(bbytes, mb) / 1e12:8.2f}  {rate(bbytes, mb) / HBM_PEAK:8.2f}  {mb / mf:7.2f}  {lo:10.3f}  {hi:10.3f}")


def aligned(t):
    return (t.data_ptr() + 255) // 256 * 256


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--E", type=int, default=2048)
    ap.add_argument("--rows", type=int, default=131072)
    ap.add_argument("--D", type=int, default=1024)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("block_bwd_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, blib = engine.load_library(), engine.load_bwd_library()
    S, L, E, rows, D = a.S, a.L, a.E, a.rows, a.D
    st = torch.cuda.current_stream().cuda_stream
    lines = [f"# conv and add + RMSNorm backward vs forward, {torch.cuda.get_device_name(0)}, build {lib.pcad_build_hash().decode()}",
             f"# conv S={S} L={L} E={E} (segment {ops.CONV_BWD_SEG}); norm rows={rows} D={D}, fp32 residual stream, prenorm gradient given (slab "
             f"{ops.NORM_BWD_ROWS}); HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds (forward, backward alternating)",
             f"# bytes by the formulas: conv fwd 2, bwd 3 tensors of S L E; norm fwd 2 + 2, bwd 3 + 3 tensors of rows D (model + residual dtype); "
             f"of_peak = of {HBM_PEAK / 1e12:.0f} TB/s",
             f"# scratch: conv {blib.pcad_causal_conv1d_silu_bwd_scratch_bytes(S, L, E) / 2 ** 20:.0f} MiB, "
             f"norm {blib.pcad_add_rmsnorm_bwd_scratch_bytes(rows, D) / 2 ** 20:.0f} MiB",
             "operator       dtype     fwd_ms   fwd_ns/row  fwd_TB/s   of_peak  bwd_ms   bwd_ns/row  bwd_TB/s   of_peak  bwd/fwd  bwd_min_ms  bwd_max_ms"]
    for dt in (torch.bfloat16, torch.float32):
        es, code = torch.empty((), dtype=dt).element_size(), engine._DT[dt]
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)
        # ---- conv ----
        x, dout = rnd(S, L, E).to(dt), rnd(S, L, E).to(dt)
        w, b = ((torch.rand(E, 4, device=dev, generator=g) * 2 - 1) * 0.5).contiguous(), (torch.rand(E, device=dev, generator=g) * 2 - 1) * 0.5
        y, dx = torch.empty_like(x), torch.empty_like(x)
        dw, db = torch.empty(E, 4, device=dev), torch.empty(E, device=dev)
        nb = blib.pcad_causal_conv1d_silu_bwd_scratch_bytes(S, L, E)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        sp = aligned(scratch)
        for rev in (0, 1):
            def fwd():
                engine._check(lib.pcad_causal_conv1d_silu_dir(x.data_ptr(), E, w.data_ptr(), b.data_ptr(), y.data_ptr(), E, S, L, E, rev, 0, 0, code, st),
                              "pcad_causal_conv1d_silu_dir")

            def bwd():
                engine._check(blib.pcad_causal_conv1d_silu_bwd(x.data_ptr(), E, w.data_ptr(), b.data_ptr(), dout.data_ptr(), dx.data_ptr(), dw.data_ptr(),
                                                               db.data_ptr(), sp, nb, S, L, E, rev, code, st), "pcad_causal_conv1d_silu_bwd")
            mf, mb, lo, hi = series(fwd, bwd, a.warmup, a.steps)
            assert bool(torch.isfinite(dw).all()) and bool(torch.isfinite(dx.float()).all())
            lines.append(row("conv reverse" if rev else "conv forward", dt, S * L, mf, mb, lo, hi, 2 * S * L * E * es, 3 * S * L * E * es))
            print(lines[-1], flush=True)
        del x, dout, y, dx, scratch
        torch.cuda.empty_cache()
        # ---- add + RMSNorm ----
        x, dy = rnd(rows, D).to(dt), rnd(rows, D).to(dt)
        res, dres_out = rnd(rows, D) * 2.0, rnd(rows, D)
        wn = torch.rand(D, device=dev, generator=g) + 0.5
        y, dx = torch.empty_like(x), torch.empty_like(x)
        res_out, dres_in = torch.empty_like(res), torch.empty_like(res)
        dwn = torch.empty(D, device=dev)
        nb = blib.pcad_add_rmsnorm_bwd_scratch_bytes(rows, D)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        sp = aligned(scratch)

        def nfwd():
            engine._check(lib.pcad_add_rmsnorm(x.data_ptr(), res.data_ptr(), wn.data_ptr(), y.data_ptr(), res_out.data_ptr(), rows, D, 1e-5, code, 0, st),
                          "pcad_add_rmsnorm")

        def nbwd():
            engine._check(blib.pcad_add_rmsnorm_bwd(x.data_ptr(), res.data_ptr(), wn.data_ptr(), dy.data_ptr(), dres_out.data_ptr(), dx.data_ptr(),
                                                    dres_in.data_ptr(), dwn.data_ptr(), sp, nb, rows, D, 1e-5, code, 0, st), "pcad_add_rmsnorm_bwd")
        mf, mb, lo, hi = series(nfwd, nbwd, a.warmup, a.steps)
        assert bool(torch.isfinite(dwn).all()) and bool(torch.isfinite(dx.float()).all())
        lines.append(row("add + rmsnorm", dt, rows, mf, mb, lo, hi, rows * D * (2 * es + 2 * 4), rows * D * (3 * es + 3 * 4)))
        print(lines[-1], flush=True)
        del x, dy, res, dres_out, y, dx, res_out, dres_in, scratch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
