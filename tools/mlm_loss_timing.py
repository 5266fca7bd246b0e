"""Time the masked-LM loss forward (pcad_forward_loss) against the plain full-window forward that writes every position's logits
(pcad_forward, positions == NULL), same process, interleaved, HIP events:

    (a)  pcad_forward, logits_out [B, L, 8]            - of --baseline-lib (a libpcad.so built from the parent commit) when given,
                                                         else of this build
    (a') the same call again (a second series of the same thing: the A/A spread the acceptance bound is compared with)
    (b)  pcad_forward_loss, sums_out only, 15 % of the positions labelled
    (c)  pcad_forward_loss, sums_out + nll_out + logits_out, every position labelled

at l32 bf16 512 x 512 bp and PlantCAD2 Medium bf16 32 x 8 192 bp.  One round = (a), (b), (c), (a') once each in that order; the
figure of a series is the median over the rounds.  Synthetic weights generated on the device (timing only).

    python tools/mlm_loss_timing.py [--out profiles/mlm_loss_timing.json] [--steps 20] [--warmup 3] [--baseline-lib PATH]
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config  # noqa: E402
from seqcls_timing import device_weights  # noqa: E402


def baseline_engine(path, cfg, sd, dtype, dev):
    """An Engine on another libpcad.so (the parent commit's build, which lacks the loss symbols): the same binding code."""
    lib = C.CDLL(path)
    for name, (res, args) in engine.SIGNATURES.items():
        if hasattr(lib, name):
            fn = getattr(lib, name)
            fn.restype, fn.argtypes = res, args
    mine, engine._lib = engine._lib, lib
    try:
        return engine.Engine(cfg, sd, dtype, dev), lib.pcad_build_hash().decode()
    finally:
        engine._lib = mine


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
    ap.add_argument("--baseline-lib", default=None)
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    for size, B, L in (("l32", 512, 512), ("pc2-medium", 32, 8192)):
        cfg = make_config(size)
        sd = device_weights(cfg, dev)
        eng = engine.Engine(cfg, sd, torch.bfloat16, dev)
        base, base_hash = (baseline_engine(a.baseline_lib, cfg, sd, torch.bfloat16, dev) if a.baseline_lib
                           else (eng, eng.lib.pcad_build_hash().decode()))
        g = torch.Generator(device=dev).manual_seed(1)
        ids = torch.randint(3, 7, (B, L), device=dev, generator=g)
        full = torch.randint(3, 7, (B, L), device=dev, generator=g).to(torch.int32)
        sparse = torch.where(torch.rand(B, L, device=dev, generator=g) < 0.15, full, torch.full_like(full, -100))
        w = torch.rand(B, L, device=dev, generator=g)
        series = {
            "a_forward_logits": lambda: base.forward(ids),
            "b_loss_sums_15pct": lambda: eng.forward_loss(ids, sparse, w),
            "c_loss_all_outputs_100pct": lambda: eng.forward_loss(ids, full, w, want_nll=True, want_logits=True),
            "a2_forward_logits_again": lambda: base.forward(ids),
        }
        for _ in range(a.warmup):
            for fn in series.values():
                fn()
        torch.cuda.synchronize()
        ms = {k: [] for k in series}
        for _ in range(a.steps):
            for k, fn in series.items():
                ms[k].append(event_ms(fn))
        med = {k: statistics.median(v) for k, v in ms.items()}
        eng.profile(1)
        series["b_loss_sums_15pct"]()
        hb = eng.profile_read()["final_head"][1]
        series["c_loss_all_outputs_100pct"]()
        hc = eng.profile_read()["final_head"][1]
        eng.profile(False)
        base.profile(1)
        series["a_forward_logits"]()
        ha = base.profile_read()["final_head"][1]
        base.profile(False)
        aa = abs(med["a2_forward_logits_again"] / med["a_forward_logits"] - 1)
        r = dict(model=size, dtype="bfloat16", B=B, L=L, steps=a.steps, warmup=a.warmup, build_hash=eng.lib.pcad_build_hash().decode(),
                 baseline_build_hash=base_hash, median_ms={k: round(v, 3) for k, v in med.items()},
                 min_ms={k: round(min(v), 3) for k, v in ms.items()},
                 b_over_a=round(med["b_loss_sums_15pct"] / med["a_forward_logits"], 5),
                 c_over_a=round(med["c_loss_all_outputs_100pct"] / med["a_forward_logits"], 5),
                 a_over_a_spread=round(aa, 5), head_ms=dict(a=round(ha, 4), b=round(hb, 4), c=round(hc, 4)))
        print(json.dumps(r), flush=True)
        rows.append(r)
        for e in {id(eng): eng, id(base): base}.values():
            e.close()
        del eng, base, sd
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
