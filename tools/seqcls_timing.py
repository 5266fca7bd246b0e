"""Time the sequence-classification forward (pcad_forward_pooled) against the plain full-window forward (pcad_forward, every
position's LM logits) on the PlantCAD2 Small / Medium / Large geometries at L = 600 and 8 192, and report the pooled head's
share (kernel class PCAD_K_HEAD, HIP events).  Synthetic weights generated on the device (timing only; values are irrelevant
beyond being finite).

    python tools/seqcls_timing.py [--out profiles/seqcls_timing.json] [--steps 3]
"""
import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd.checkpoint import expected_keys, make_config  # noqa: E402
from plantcaduceus_amd.engine import Engine  # noqa: E402


def device_weights(cfg, dev, seed=0):
    g = torch.Generator(device=dev).manual_seed(seed)
    sd = {}
    for k, shape in expected_keys(cfg).items():
        if k.endswith("A_log"):
            sd[k] = torch.log(torch.arange(1, shape[1] + 1, device=dev, dtype=torch.float32)).expand(shape).contiguous()
        elif k.endswith(".D") or "norm" in k:
            sd[k] = torch.ones(shape, device=dev)
        elif k.endswith("dt_proj.bias"):
            dt = torch.exp(torch.rand(shape, device=dev, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3))
            sd[k] = dt + torch.log(-torch.expm1(-dt))
        else:
            fan_in = shape[-1] if len(shape) > 1 else shape[0]
            sd[k] = (torch.rand(shape, device=dev, generator=g) * 2 - 1) * fan_in ** -0.5
    return sd


def timed(fn, steps):
    fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(steps):
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        t.append(time.perf_counter() - t0)
    return min(t), sorted(t)[len(t) // 2]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--sizes", default="pc2-small,pc2-medium,pc2-large")
    a = ap.parse_args()
    dev = torch.device("cuda:0")
    rows = []
    runs = [(s, torch.bfloat16, {}) for s in a.sizes.split(",")] + [("pc2-small", torch.float32, {"f32_gemm_split": 1})]
    for size, dtype, opts in runs:
        cfg = make_config(size)
        cfg.engine_options = opts
        eng = Engine(cfg, device_weights(cfg, dev), dtype, dev)
        W = torch.randn(2, cfg.d_model, device=dev) * 0.05
        for L, B in ((600, 128), (8192, 16)):
            ids = torch.randint(3, 7, (B, L), device=dev)
            pooled = lambda: eng.forward_pooled(ids, "mean", W)      # noqa: E731
            plain = lambda: eng.forward(ids)                        # noqa: E731
            tp, tpm = timed(pooled, a.steps)
            tf, tfm = timed(plain, a.steps)
            eng.profile(1)
            pooled()
            st = eng.profile_read()
            eng.profile(False)
            total = sum(ms for _, ms in st.values())
            head = st["final_head"][1]
            r = dict(model=size, dtype=str(dtype).replace("torch.", ""), options=opts, L=L, B=B,
                     pooled_s=round(tp, 5), pooled_median_s=round(tpm, 5), plain_forward_s=round(tf, 5),
                     plain_median_s=round(tfm, 5), pooled_over_plain=round(tp / tf, 4),
                     head_ms=round(head, 4), head_launches=st["final_head"][0], head_share=round(head / total, 5),
                     windows_per_s=round(B / tp, 2))
            print(json.dumps(r), flush=True)
            rows.append(r)
        eng.close()
        del eng
        torch.cuda.empty_cache()
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": torch.cuda.get_device_name(0), "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
