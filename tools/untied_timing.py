"""Cost of the untied-directions form: forward_pooled on PlantCAD2 Small, L = 8192, B = 4, fp32 + f32_gemm_split - the
untied form, reference_order 2 and the default tied form in one process, interleaved, medians.
    python tools/untied_timing.py [out.json]      (default: profiles/untied_forward_timing.json)"""
import json, os, statistics, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT); sys.path.insert(0, os.path.join(ROOT, "tests"))
import torch
from plantcaduceus_amd.checkpoint import make_config
from plantcaduceus_amd.engine import Engine
from untied_ref import untied_state_dict

DEV = torch.device("cuda:0")
sd = untied_state_dict(make_config("pc2-small"), seed=1)
sd = {k: v for k, v in sd.items() if k.startswith("caduceus.")}
def eng(**o):
    cfg = make_config("pc2-small"); cfg.engine_options = dict(f32_gemm_split=1, **o)
    return Engine(cfg, sd, torch.float32, DEV)
engines = {"untied_directions": eng(untied_directions=1), "reference_order_2": eng(reference_order=2), "tied_default": eng()}
ids = torch.randint(3, 7, (4, 8192), generator=torch.Generator().manual_seed(0)).to(DEV)
W = (torch.randn(2, 768, generator=torch.Generator().manual_seed(1)) * 0.05).to(DEV)
times = {k: [] for k in engines}
for it in range(3 + 9):
    for k, e in engines.items():
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record(); e.forward_pooled(ids, "mean", W); b.record(); b.synchronize()
        if it >= 3:
            times[k].append(a.elapsed_time(b))
med = {k: statistics.median(v) for k, v in times.items()}
out = {"workload": "forward_pooled, PlantCAD2 Small (d_model 768, 24 layers), B = 4, L = 8192, fp32 + f32_gemm_split, synthetic weights",
       "method": "one process, the three engines interleaved per iteration, 3 warm-up + 9 timed iterations, HIP events, medians",
       "median_ms": med, "min_ms": {k: min(v) for k, v in times.items()}, "max_ms": {k: max(v) for k, v in times.items()},
       "ratio_untied_over_reference_order_2": med["untied_directions"] / med["reference_order_2"],
       "ratio_untied_over_tied_default": med["untied_directions"] / med["tied_default"],
       "device": torch.cuda.get_device_name(0)}
dst = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "profiles", "untied_forward_timing.json")
with open(dst, "w") as f:
    json.dump(out, f, indent=1)
print(json.dumps(out))
