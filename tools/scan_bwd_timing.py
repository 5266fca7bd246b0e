"""Time the selective scan's backward (pcad_selective_scan_bwd) next to its forward (pcad_selective_scan) on the same tensors:
S = 256 strands x L = 512 x E = 2048 channels (l32's d_inner: a training batch of 128 windows, both strands), both dtypes, both directions,
gated.  Token-major tensors generated on the device, no transposes in the timed calls; HIP events around each call on the current
stream, warm-up launches first, one round = forward then backward, the figure of a series is the median over the rounds.

    python tools/scan_bwd_timing.py [--out profiles/scan_bwd_timing.txt] [--steps 20] [--warmup 3] [--S 256] [--L 512] [--E 2048]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine, ops  # noqa: E402


def event_ms(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--S", type=int, default=256)
    ap.add_argument("--L", type=int, default=512)
    ap.add_argument("--E", type=int, default=2048)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_bwd_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, tlib = engine.load_library(), engine.load_train_library()
    S, L, E = a.S, a.L, a.E
    rows = S * L
    lines = [f"# selective scan backward vs forward, {torch.cuda.get_device_name(0)}, build {lib.pcad_build_hash().decode()}",
             f"# S={S} L={L} E={E} gated; HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds (forward, backward alternating); "
             f"chunk T={ops.SCAN_BWD_CHUNK}",
             f"# scratch {tlib.pcad_selective_scan_bwd_scratch_bytes(S, L, E) / 2 ** 20:.0f} MiB",
             "dtype     direction  fwd_ms   fwd_ns/row  bwd_ms   bwd_ns/row  bwd/fwd  bwd_min_ms  bwd_max_ms"]
    for dt in (torch.bfloat16, torch.float32):
        g = torch.Generator(device=dev).manual_seed(1)
        rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)
        u, z, dout = (rnd(S, L, E).to(dt) for _ in range(3))
        delta = (rnd(S, L, E) * 0.5 - 3.0).to(dt)
        bc = rnd(rows, 32)
        A = -torch.exp(torch.log(torch.arange(1, 17, device=dev).float())[None, :] + 0.3 * rnd(E, 16)).contiguous()
        D, db = torch.rand(E, device=dev, generator=g) + 0.5, rnd(E)
        y, du, dd, dz = (torch.empty_like(u) for _ in range(4))
        dbc = torch.empty(rows, 32, device=dev)
        dA, dD, dbias = torch.empty(E, 16, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev)
        nb = tlib.pcad_selective_scan_bwd_scratch_bytes(S, L, E)
        scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
        sp = (scratch.data_ptr() + 255) // 256 * 256
        code, st = engine._DT[dt], torch.cuda.current_stream().cuda_stream
        for rev in (0, 1):
            def fwd():
                engine._check(lib.pcad_selective_scan(u.data_ptr(), delta.data_ptr(), z.data_ptr(), E, bc.data_ptr(), A.data_ptr(), D.data_ptr(),
                                                      db.data_ptr(), y.data_ptr(), S, L, E, rev, 0, code, st), "pcad_selective_scan")

            def bwd():
                engine._check(tlib.pcad_selective_scan_bwd(u.data_ptr(), delta.data_ptr(), z.data_ptr(), E, bc.data_ptr(), A.data_ptr(),
                                                          D.data_ptr(), db.data_ptr(), dout.data_ptr(), du.data_ptr(), dd.data_ptr(),
                                                          dz.data_ptr(), dbc.data_ptr(), dA.data_ptr(), dD.data_ptr(), dbias.data_ptr(), sp, nb,
                                                          S, L, E, rev, code, st), "pcad_selective_scan_bwd")
            for _ in range(a.warmup):
                fwd()
                bwd()
            torch.cuda.synchronize()
            tf, tb = [], []
            for _ in range(a.steps):
                tf.append(event_ms(fwd))
                tb.append(event_ms(bwd))
            mf, mb = statistics.median(tf), statistics.median(tb)
            assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(du.float()).all())
            lines.append(f"{str(dt).split('.')[-1]:9s} {'reverse' if rev else 'forward':9s}  {mf:7.3f}  {mf * 1e6 / rows:10.1f}  {mb:7.3f}  "
                         f"{mb * 1e6 / rows:10.1f}  {mb / mf:7.2f}  {min(tb):10.3f}  {max(tb):10.3f}")
            print(lines[-1], flush=True)
        del u, z, dout, delta, y, du, dd, dz, scratch
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
