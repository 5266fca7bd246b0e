"""Time the segmented backward of the selective scan (pcad_selective_scan_bwd_seg) next to the unsegmented entry
(pcad_selective_scan_bwd) on the same tensors: long windows at a small batch - E = 1536 (PlantCAD2 Small's d_inner), L = 8192,
S = 2, 8 and 86 strands (1, 4 and 43 windows) -, both dtypes, both directions, gated, segments = 2 .. 64.  The method is
tools/scan_bwd_timing.py's: token-major tensors generated on the device, no transposes in the timed calls, HIP events around each call
on the current stream, warm-up rounds first, one round = every series once, the figure of a series is the median over the rounds.
The last column is what ops.scan_bwd_auto_segments picks for the shape on this device.

    python tools/scan_bwd_seg_timing.py [--out profiles/scan_bwd_seg_timing.txt] [--steps 20] [--warmup 3] [--S 2,8,86] [--L 8192] [--E 1536]
"""
import argparse
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine, ops  # noqa: E402
from tools.scan_bwd_timing import event_ms  # noqa: E402

SEGMENTS = (2, 4, 8, 16, 32, 64)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--S", default="2,8,86")
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--E", type=int, default=1536)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_bwd_seg_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, tlib, blib = engine.load_library(), engine.load_train_library(), engine.load_bwd_library()
    L, E = a.L, a.E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"# selective scan backward, unsegmented (G = 1: pcad_selective_scan_bwd) and in G segments (pcad_selective_scan_bwd_seg), "
             f"{torch.cuda.get_device_name(0)} ({cus} CUs), build {lib.pcad_build_hash().decode()}",
             f"# L={L} E={E} gated; HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds (every series once per round); "
             f"chunk T={ops.SCAN_BWD_CHUNK}; steps per segment: " + " ".join(f"G={G}:{ops.scan_bwd_seg_steps(L, G)}" for G in SEGMENTS),
             f"# ms per call; auto = ops.scan_bwd_auto_segments(S, L, E) with SCAN_BWD_SEG_MIN_STEPS = {ops.SCAN_BWD_SEG_MIN_STEPS}",
             "S    dtype     direction  " + "  ".join(f"{'G=' + str(G):>8s}" for G in (1,) + SEGMENTS) + "  auto  best"]
    for S in (int(v) for v in a.S.split(",")):
        rows = S * L
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=dev).manual_seed(1)
            rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)
            u, z, dout = (rnd(S, L, E).to(dt) for _ in range(3))
            delta = (rnd(S, L, E) * 0.5 - 3.0).to(dt)
            bc = rnd(rows, 32)
            A = -torch.exp(torch.log(torch.arange(1, 17, device=dev).float())[None, :] + 0.3 * rnd(E, 16)).contiguous()
            D, db = torch.rand(E, device=dev, generator=g) + 0.5, rnd(E)
            du, dd, dz = (torch.empty_like(u) for _ in range(3))
            dbc = torch.empty(rows, 32, device=dev)
            dA, dD, dbias = torch.empty(E, 16, device=dev), torch.empty(E, device=dev), torch.empty(E, device=dev)
            nb = max([tlib.pcad_selective_scan_bwd_scratch_bytes(S, L, E)] + [blib.pcad_selective_scan_bwd_seg_scratch_bytes(S, L, E, G) for G in SEGMENTS])
            scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
            sp = (scratch.data_ptr() + 255) // 256 * 256
            code, st = engine._DT[dt], torch.cuda.current_stream().cuda_stream
            for rev in (0, 1):
                head = (u.data_ptr(), delta.data_ptr(), z.data_ptr(), E, bc.data_ptr(), A.data_ptr(), D.data_ptr(), db.data_ptr(), dout.data_ptr(),
                        du.data_ptr(), dd.data_ptr(), dz.data_ptr(), dbc.data_ptr(), dA.data_ptr(), dD.data_ptr(), dbias.data_ptr(), sp, nb, S, L, E,
                        rev, code)

                def call(G):
                    if G == 1:
                        engine._check(tlib.pcad_selective_scan_bwd(*head, st), "pcad_selective_scan_bwd")
                    else:
                        engine._check(blib.pcad_selective_scan_bwd_seg(*head, G, st), "pcad_selective_scan_bwd_seg")
                series = (1,) + SEGMENTS
                for _ in range(a.warmup):
                    for G in series:
                        call(G)
                torch.cuda.synchronize()
                t = {G: [] for G in series}
                for _ in range(a.steps):
                    for G in series:
                        t[G].append(event_ms(lambda: call(G)))
                assert bool(torch.isfinite(dA).all()) and bool(torch.isfinite(du.float()).all())
                med = {G: statistics.median(t[G]) for G in series}
                auto = ops.scan_bwd_auto_segments(S, L, E)
                lines.append(f"{S:<4d} {str(dt).split('.')[-1]:9s} {'reverse' if rev else 'forward':9s}  " +
                             "  ".join(f"{med[G]:8.3f}" for G in series) + f"  {auto:4d}  {min(series, key=med.get):4d}")
                print(lines[-1], flush=True)
            del u, z, dout, delta, du, dd, dz, scratch, bc, dbc
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
