"""Time the nucleotide-probability forward (pcad_forward_probs) against the plain full-window forward that writes every position's
logits (pcad_forward, positions == NULL), same process, interleaved, HIP events:

    (a)  pcad_forward, logits_out [B, L, 8]            - of --baseline-lib (a libpcad.so built from the parent commit) when given,
                                                         else of this build
    (a') the same call again (a second series of the same thing: the A/A spread the acceptance bound is compared with)
    (b)  pcad_forward_probs, all positions, probs_out [B, L, 4] only
    (c)  pcad_forward_probs, ten positions per window (device list), probs_out [B, 10, 4] only

at l32 bf16 512 x 512 bp and PlantCAD2 Medium bf16 32 x 8 192 bp.  One round = (a), (b), (c), (a') once each in that order; the
figure of a series is the median over the rounds.  Synthetic weights generated on the device (timing only).

    python tools/probs_head_timing.py [--out profiles/probs_head_timing.json] [--steps 20] [--warmup 3] [--baseline-lib PATH]
"""
import argparse
import json
import os
import statistics
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config  # noqa: E402
from mlm_loss_timing import baseline_engine, event_ms  # noqa: E402
from seqcls_timing import device_weights  # noqa: E402

COLS = (3, 4, 5, 6)


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
        own = torch.randint(0, L, (B, 10), device=dev, generator=g)
        series = {
            "a_forward_logits": lambda: base.forward(ids),
            "b_probs_all_positions": lambda: eng.forward_probs(ids, COLS),
            "c_probs_10_per_window": lambda: eng.forward_probs(ids, COLS, positions_per_window=own),
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
        head = {}
        for key, e, k in (("a", base, "a_forward_logits"), ("b", eng, "b_probs_all_positions"), ("c", eng, "c_probs_10_per_window")):
            e.profile(1)
            series[k]()
            head[key] = round(e.profile_read()["final_head"][1], 4)
            e.profile(False)
        aa = abs(med["a2_forward_logits_again"] / med["a_forward_logits"] - 1)
        r = dict(model=size, dtype="bfloat16", B=B, L=L, steps=a.steps, warmup=a.warmup, build_hash=eng.lib.pcad_build_hash().decode(),
                 baseline_build_hash=base_hash, median_ms={k: round(v, 3) for k, v in med.items()},
                 min_ms={k: round(min(v), 3) for k, v in ms.items()},
                 b_over_a=round(med["b_probs_all_positions"] / med["a_forward_logits"], 5),
                 c_over_a=round(med["c_probs_10_per_window"] / med["a_forward_logits"], 5),
                 a_over_a_spread=round(aa, 5), head_ms=head,
                 b_within_spread=bool(med["b_probs_all_positions"] <= med["a_forward_logits"] * (1 + aa)),
                 c_within_spread=bool(med["c_probs_10_per_window"] <= med["a_forward_logits"] * (1 + aa)))
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
