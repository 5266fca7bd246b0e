"""Time the segmented training forward of the selective scan (pcad_selective_scan_fwd_seg) next to today's call
(pcad_selective_scan on plain rows with an explicit delta: the call ops.selective_scan_fn makes) on the same tensors: long windows at a
small batch - E = 1536 (PlantCAD2 Small's d_inner), L = 8192, S = 2, 8, 16, 32 and 86 strands (1, 4, 8, 16 and 43 windows) -, both dtypes, gated,
segments = 2 .. 64.  The method is tools/scan_bwd_seg_timing.py's: token-major tensors generated on the device, no transposes in the
timed calls, HIP events around each call on the current stream, warm-up rounds first, one round = every series once, the figure of a
series is the median over the rounds.  `auto` is what the forward's policy (ops.scan_fwd_auto_segments) picks for the
shape on this device, and auto_ms that series' figure (G = 1: the unsegmented call).

    python tools/scan_fwd_seg_timing.py [--out profiles/scan_fwd_seg_timing.txt] [--steps 20] [--warmup 3] [--S 2,8,16,32,86] [--L 8192] [--E 1536]
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
    ap.add_argument("--S", default="2,8,16,32,86")
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--E", type=int, default=1536)
    ap.add_argument("--directions", default="0", help="0, 1 or 0,1 (reverse)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("scan_fwd_seg_timing needs a ROCm device: a time taken anywhere else says nothing")
    dev = torch.device("cuda:0")
    lib, blib = engine.load_library(), engine.load_bwd_library()
    L, E = a.L, a.E
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    lines = [f"# selective scan training forward, unsegmented (G = 1: pcad_selective_scan, plain rows, explicit delta) and in G segments "
             f"(pcad_selective_scan_fwd_seg), {torch.cuda.get_device_name(0)} ({cus} CUs), build {lib.pcad_build_hash().decode()}",
             f"# L={L} E={E} gated; HIP events, {a.warmup} warm-up rounds, median of {a.steps} rounds (every series once per round); "
             f"steps per segment: " + " ".join(f"G={G}:{ops.scan_bwd_seg_steps(L, G)}" for G in SEGMENTS),
             f"# ms per call; auto = ops.scan_fwd_auto_segments(S, L, E) with SCAN_BWD_SEG_MIN_STEPS = {ops.SCAN_BWD_SEG_MIN_STEPS}, "
             f"SCAN_FWD_SEG_MIN_FILL = {ops.SCAN_FWD_SEG_MIN_FILL}",
             "S    dtype     direction  " + "  ".join(f"{'G=' + str(G):>8s}" for G in (1,) + SEGMENTS) + "  auto   auto_ms  best"]
    for S in (int(v) for v in a.S.split(",")):
        rows = S * L
        for dt in (torch.bfloat16, torch.float32):
            g = torch.Generator(device=dev).manual_seed(1)
            rnd = lambda *sh: torch.randn(*sh, device=dev, generator=g)
            u, z = (rnd(S, L, E).to(dt) for _ in range(2))
            delta = (rnd(S, L, E) * 0.5 - 3.0).to(dt)
            bc = rnd(rows, 32)
            A = -torch.exp(torch.log(torch.arange(1, 17, device=dev).float())[None, :] + 0.3 * rnd(E, 16)).contiguous()
            D, db = torch.rand(E, device=dev, generator=g) + 0.5, rnd(E)
            y = torch.empty_like(u)
            nb = max(blib.pcad_selective_scan_fwd_seg_scratch_bytes(S, L, E, G) for G in SEGMENTS)
            scratch = torch.empty(nb + 256, dtype=torch.uint8, device=dev)
            sp = (scratch.data_ptr() + 255) // 256 * 256
            code, st = engine._DT[dt], torch.cuda.current_stream().cuda_stream
            for rev in (int(v) for v in a.directions.split(",")):
                head = (u.data_ptr(), delta.data_ptr(), z.data_ptr(), E, bc.data_ptr(), A.data_ptr(), D.data_ptr(), db.data_ptr(), y.data_ptr())

                def call(G):
                    if G == 1:
                        engine._check(lib.pcad_selective_scan(*head, S, L, E, rev, 0, code, st), "pcad_selective_scan")
                    else:
                        engine._check(blib.pcad_selective_scan_fwd_seg(*head, sp, nb, S, L, E, rev, code, G, st), "pcad_selective_scan_fwd_seg")
                series = (1,) + SEGMENTS
                for _ in range(a.warmup):
                    for G in series:
                        call(G)
                torch.cuda.synchronize()
                t = {G: [] for G in series}
                for _ in range(a.steps):
                    for G in series:
                        t[G].append(event_ms(lambda: call(G)))
                assert bool(torch.isfinite(y.float()).all())
                med = {G: statistics.median(t[G]) for G in series}
                auto = ops.scan_fwd_auto_segments(S, L, E)
                lines.append(f"{S:<4d} {str(dt).split('.')[-1]:9s} {'reverse' if rev else 'forward':9s}  " +
                             "  ".join(f"{med[G]:8.3f}" for G in series) + f"  {auto:4d}  {med[auto]:8.3f}  {min(series, key=med.get):4d}")
                print(lines[-1], flush=True)
            del u, z, delta, y, scratch, bc
            torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)


if __name__ == "__main__":
    main()
