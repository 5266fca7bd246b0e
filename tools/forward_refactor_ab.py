"""A/B of two builds of libpcad.so on the same inputs, in one process: this build against --baseline-lib (a libpcad.so built from
the parent commit, bound a second time through ctypes).  Written for the change that split the layer walk into a request, a plan
and named phases (csrc/forward.hip), which must not change one launch or one output bit.

  0. Sizes.  pcad_workspace_bytes / pcad_weight_arena_bytes of both builds over the geometries of tests/test_gpu_geometries.py, both
     dtypes and every combination of untied_directions, f32_gemm_split, norm_fold, reference_order and scan_segments (--sizes-only: no GPU).
  1. Bit-for-bit.  Toy models (d_model 128 / 256 / 384, 2-3 layers, L <= 256, B <= 9), each chosen to take one branch of the walk,
     crossed with the entry points.  For every call: every output buffer compared as raw bytes, and pcad_profile_read's launches per
     kernel class compared.  Verdict per call: differing bytes, differing classes.
  2. Speed.  l32 width, B = 1, L = 512, bf16: (i) the host-side duration of one pcad_forward call (until it returns, no
     synchronisation) and (ii) its HIP-event duration, as medians.  One round = parent, this build, parent again (the A/A pair) and
     this build again, once each; the starting series rotates from round to round, so that every series runs equally often after
     each other one.  Two things besides the code differ between two engines, and the design takes both out of the A/B figure:
       - each engine has its own weight arena and workspace.  The A/A partner is therefore a SECOND engine of the parent's library
         (one engine timed twice agrees with itself to 0.003 % of the HIP-event time, which says nothing about two engines);
       - the order of creation: on one MI355X the engine created first ran this call 0.45 % slower in HIP-event time whichever
         library it came from (this build first: +0.44 % against the parent; the parent first: -0.46 %).  So the rounds are run
         twice, with fresh engines, this build created first and the parent created first, and a figure's A/B difference and its
         A/A spread are the means of the two orders' ratios.  Each order's own medians and ratios are written out beside them.

    python tools/forward_refactor_ab.py --baseline-lib PATH [--out profiles/forward_refactor_ab.json] [--steps 300] [--warmup 20]
                                        [--skip-bits] [--skip-speed] [--sizes-only]

Exit status 1 when any call differs in a byte or in a launch count, or when this build is slower than the parent by more than the
parent-against-itself (A/A) spread of the same rounds, in the host enqueue time or in the HIP-event time, or when a size query
differs; the JSON is written first.
"""
import argparse
import ctypes as C
import itertools
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import torch  # noqa: E402

from plantcaduceus_amd import engine  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402
from mlm_loss_timing import baseline_engine  # noqa: E402
from seqcls_timing import device_weights  # noqa: E402

DEV = torch.device("cuda:0")
COLS = [3, 4, 5, 6]

# name: (dtype, d_model, n_layer, B, L, engine options, config overrides) - the branch of the walk the case is there for
CASES = {
    "fold":               ("bf16", 256, 3, 2, 128, {}, {}),                              # fold engaged: whole 256-row tiles
    "fold-padded-width":  ("bf16", 384, 2, 2, 128, {}, {}),                              # D 384 -> 512 columns, rows % 256 == 0
    "fold-refused":       ("bf16", 256, 3, 3, 45, {}, {}),                               # ragged rows: every chunk unfolded
    "fp32":               ("fp32", 128, 2, 3, 64, {}, {}),
    "fp32-split":         ("fp32", 128, 3, 2, 128, {"f32_gemm_split": 1}, {}),           # scan-written out_proj operand
    "fp32-split-ragged":  ("fp32", 128, 2, 3, 45, {"f32_gemm_split": 1}, {}),            # L % 8 != 0: the conversion pass
    "reforder1":          ("bf16", 256, 3, 2, 128, {"reference_order": 1}, {}),
    "reforder2":          ("bf16", 256, 3, 2, 128, {"reference_order": 2}, {}),          # strict-order out_proj
    "untied":             ("bf16", 128, 3, 3, 64, {}, {"bidirectional_weight_tie": False}),
    "untied-split":       ("fp32", 128, 2, 2, 128, {"f32_gemm_split": 1}, {"bidirectional_weight_tie": False}),
    "segmented-scan":     ("bf16", 128, 3, 1, 256, {}, {}),
    "segmented-split":    ("fp32", 128, 2, 1, 256, {"f32_gemm_split": 1}, {}),
    "pair-walk":          ("bf16", 128, 3, 3, 128, {}, {}),
    "convx-ksplit":       ("bf16", 128, 2, 3, 77, {}, {"dt_rank": 80}),                  # Rp 96, K-split 2
    "noseg":              ("bf16", 128, 3, 1, 256, {"scan_segments": 0}, {}),
    "dt-rank-128":        ("bf16", 128, 2, 3, 45, {}, {"dt_rank": 128}),                 # unfused conv, x_proj as a GEMM
    "no-shortcut":        ("bf16", 256, 3, 2, 128, {"last_layer_shortcut": 0}, {}),
    "no-shortcut-strict": ("fp32", 128, 2, 3, 64, {"last_layer_shortcut": 0, "reference_order": 2}, {}),
    "strict-split":       ("fp32", 128, 2, 2, 64, {"reference_order": 2, "f32_gemm_split": 1}, {}),
    "chunk-uneven":       ("bf16", 128, 2, 5, 64, {"chunk_seqs": 2}, {}),                # chunks of 2, 2, 1
    "chunk-uneven-fold":  ("bf16", 256, 2, 5, 128, {"chunk_seqs": 2}, {}),
    "nine-windows":       ("bf16", 128, 2, 9, 96, {"chunk_seqs": 4}, {}),
    "poison":             ("bf16", 256, 3, 2, 128, {"poison_workspace": 1}, {}),
    "poison-fp32":        ("fp32", 128, 2, 3, 45, {"poison_workspace": 1}, {}),
    "debug-repeat":       ("bf16", 128, 2, 2, 64, {"debug_repeat_class": 1, "debug_repeat": 3}, {}),
    "debug-repeat-scan":  ("bf16", 128, 3, 3, 128, {"debug_repeat_class": 4, "debug_repeat": 3}, {}),   # pair-walk's shape: repeats refuse the pair walk
}
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}


# the geometries of tests/test_gpu_geometries.py (CASES and D2048): (d_model, expand, dt_rank or None: "auto", residual_in_fp32, B, L)
GEOMETRIES = [(128, 2, 100, 1, 3, 45), (256, 2, 128, 1, 2, 128), (128, 2, 129, 1, 2, 64), (64, 2, 256, 1, 2, 40), (128, 2, 100, 1, 2, 300),
              (64, 2, 100, 1, 1, 2080), (128, 2, 80, 1, 3, 77), (64, 1, None, 1, 3, 64), (256, 1, None, 1, 2, 128), (128, 3, None, 1, 2, 96),
              (256, 3, None, 1, 2, 128), (64, 4, None, 1, 3, 128), (128, 2, None, 0, 3, 45), (256, 2, None, 0, 2, 128), (2048, 2, None, 1, 2, 64)]
SIZE_OPTIONS = {"untied_directions": (0, 1), "f32_gemm_split": (0, 1), "norm_fold": (None, 0, 1), "reference_order": (0, 1, 2), "scan_segments": (1, 0)}


def sizes(path):
    """pcad_workspace_bytes and pcad_weight_arena_bytes of both builds over GEOMETRIES x both dtypes x every combination of
    SIZE_OPTIONS (None: the option left at its default).  Needs no GPU.  -> (handles compared, the rows that differ)"""
    libs = engine.load_library(), C.CDLL(path)
    for name in ("pcad_create", "pcad_set_option", "pcad_workspace_bytes", "pcad_weight_arena_bytes", "pcad_destroy"):
        getattr(libs[1], name).restype, getattr(libs[1], name).argtypes = engine.SIGNATURES[name]
    n, bad = 0, []
    for (D, expand, R, res32, B, L), dtype in itertools.product(GEOMETRIES, (0, 1)):
        for values in itertools.product(*SIZE_OPTIONS.values()):
            opts = {k: v for k, v in zip(SIZE_OPTIONS, values) if v is not None}
            got = []
            for lib in libs:
                c = engine.PcadConfig(d_model=D, n_layer=2, d_state=16, d_conv=4, expand=expand, dt_rank=R or (D + 15) // 16, vocab=8, eps=1e-5,
                                      dtype=dtype, residual_in_fp32=res32, complement=(C.c_int32 * 8)(0, 1, 2, 6, 5, 4, 3, 7))
                h = C.c_void_p()
                rc = [lib.pcad_create(C.byref(c), C.byref(h))]
                if rc[0] == 0:
                    rc += [lib.pcad_set_option(h, k.encode(), v) for k, v in opts.items()]
                    rc += [lib.pcad_workspace_bytes(h, B, L), lib.pcad_weight_arena_bytes(h)]
                    lib.pcad_destroy(h)
                got.append(rc)
            n += 1
            if got[0] != got[1]:
                bad.append(dict(geometry=[D, expand, R, res32, B, L], dtype=dtype, options=opts, this_build=got[0], parent=got[1]))
    return n, bad


def build_pair(path, dtype, D, NL, opts, over):
    over = dict(over)
    ssm = dict(d_state=16, d_conv=4, expand=2, dt_rank=over.pop("dt_rank", "auto"), bias=False, conv_bias=True)
    cfg = make_config("x", d_model=D, n_layer=NL, ssm_cfg=ssm, **over)
    cfg.engine_options = dict(opts)
    sd = {k: v for k, v in synthetic_state_dict(cfg, seed=D + NL).items() if k.startswith("caduceus.")}
    if not cfg.bidirectional_weight_tie:        # mamba_rev's own projections differ from mamba_fwd's
        for k in sd:
            if ".mamba_rev." in k and (k.endswith("in_proj.weight") or k.endswith("out_proj.weight")):
                sd[k] = sd[k].flip(0).contiguous()
    new = engine.Engine(cfg, sd, DTYPES[dtype], DEV)
    old, old_hash = baseline_engine(path, cfg, sd, DTYPES[dtype], DEV)
    return cfg, new, old, old_hash


def calls(cfg, B, L):
    """name -> fn(engine) -> tuple of output tensors: the entry points, in every position form."""
    g = torch.Generator().manual_seed(B * 1000 + L)
    ids = torch.randint(3, 7, (B, L), generator=g).to(DEV)
    shared = [L // 2, 1, L - 2]
    own1 = torch.randint(0, L, (B,), generator=g).to(DEV)
    own3 = torch.randint(0, L, (B, 3), generator=g).to(DEV)
    labels = torch.where(torch.rand(B, L, generator=g) < 0.3, torch.randint(3, 7, (B, L), generator=g), torch.tensor(-100)).to(DEV)
    lw = torch.rand(B, L, generator=g).to(DEV)
    score = torch.randn(3, cfg.d_model, generator=g) * 0.1
    nl = cfg.n_layer
    return {
        "forward": lambda e: e.forward(ids, want_hidden=True),
        "forward_positions": lambda e: e.forward(ids, positions=shared, want_hidden=True),
        "forward_one_position": lambda e: e.forward(ids, positions=[L // 2]),
        "forward_at": lambda e: e.forward(ids, positions=own1, want_hidden=True),
        "forward_all_hidden": lambda e: e.forward(ids, want_hidden=True, all_hidden=True),
        "forward_pooled_mean": lambda e: e.forward_pooled(ids, "mean", score, want_pooled=True),
        "forward_pooled_max": lambda e: e.forward_pooled(ids, "max", score, want_pooled=True),
        "forward_loss": lambda e: e.forward_loss(ids, labels, lw, want_nll=True, want_logits=True),
        "forward_probs_all": lambda e: e.forward_probs(ids, COLS, want_logits=True),
        "forward_probs_shared": lambda e: e.forward_probs(ids, COLS, positions=shared, want_logits=True),
        "forward_probs_per_window": lambda e: e.forward_probs(ids, COLS, positions_per_window=own3, want_logits=True),
        "forward_layers_last_shared": lambda e: (e.forward_layers(ids, layers=[nl], positions=shared),),
        "forward_layers_last_per_window": lambda e: (e.forward_layers(ids, layers=[nl], positions_per_window=own3),),
        "forward_layers_last_one_per_window": lambda e: (e.forward_layers(ids, layers=[nl], positions_per_window=own3[:, :1].contiguous()),),
        "forward_layers_lower": lambda e: (e.forward_layers(ids, layers=[0, 1, nl], positions=shared, average=True),),
        "forward_layers_all_per_window": lambda e: (e.forward_layers(ids, positions_per_window=own3),),
    }


def differing_bytes(a, b):
    n = 0
    for x, y in zip(a, b):
        if x is None and y is None:
            continue
        assert x.shape == y.shape and x.dtype == y.dtype
        n += int((x.contiguous().view(torch.uint8) != y.contiguous().view(torch.uint8)).sum())
    return n


def differs(c):
    return bool(c["differing_bytes"] or c["differing_launch_classes"])


def bit_for_bit(path):
    rows = []
    for name, (dtype, D, NL, B, L, opts, over) in CASES.items():
        cfg, new, old, old_hash = build_pair(path, dtype, D, NL, opts, over)
        new.profile(1)
        old.profile(1)
        row = dict(case=name, dtype=dtype, d_model=D, n_layer=NL, B=B, L=L, options=opts, config=over, calls=[])
        for call, fn in calls(cfg, B, L).items():
            out_new, out_old = fn(new), fn(old)
            torch.cuda.synchronize()
            new.check_status()
            old.check_status()
            ln = {k: v[0] for k, v in new.profile_read().items()}
            lo = {k: v[0] for k, v in old.profile_read().items()}
            row["calls"].append(dict(call=call, output_bytes=sum(t.numel() * t.element_size() for t in out_new if t is not None),
                                     differing_bytes=differing_bytes(out_new, out_old), launches=" ".join(f"{k}:{v}" for k, v in ln.items() if v),
                                     differing_launch_classes=sorted(k for k in set(ln) | set(lo) if ln.get(k) != lo.get(k))))
        new.close()
        old.close()
        rows.append(row)
        print(f"{name}: {len(row['calls'])} calls, {sum(differs(c) for c in row['calls'])} differ", flush=True)
    return rows, old_hash


def speed_order(path, cfg, sd, steps, warmup, baseline_first):
    """One creation order of the engines: the medians and minima of the four series, and the two ratios per figure."""
    if baseline_first:
        old, _ = baseline_engine(path, cfg, sd, torch.bfloat16, DEV)
    new = engine.Engine(cfg, sd, torch.bfloat16, DEV)
    if not baseline_first:
        old, _ = baseline_engine(path, cfg, sd, torch.bfloat16, DEV)
    old2, _ = baseline_engine(path, cfg, sd, torch.bfloat16, DEV)      # the A/A partner: its own arena and workspace, as the A/B pair has
    B, L = 1, 512
    ids = torch.randint(3, 7, (B, L), device=DEV, dtype=torch.int32)
    logits = torch.empty((B, L, 8), dtype=torch.float32, device=DEV)
    stream = torch.cuda.current_stream().cuda_stream

    def one(e):
        ws, ws_bytes = e._workspace(B, L)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        t0 = time.perf_counter_ns()
        rc = e.lib.pcad_forward(e._h, ids.data_ptr(), B, L, None, 0, None, logits.data_ptr(), ws, ws_bytes, stream)
        t1 = time.perf_counter_ns()
        b.record()
        b.synchronize()
        assert rc == 0
        return (t1 - t0) / 1e3, a.elapsed_time(b) * 1e3

    series = {"parent": old, "this_build": new, "parent_again": old2, "this_build_again": new}
    names = list(series)
    for _ in range(warmup):
        for e in series.values():
            one(e)
    host, dev = {k: [] for k in series}, {k: [] for k in series}
    for i in range(steps):
        for k in names[i % 4:] + names[:i % 4]:
            h, d = one(series[k])
            host[k].append(h)
            dev[k].append(d)
    out = dict(baseline_engine_created_first=baseline_first)
    for what, t in (("host_enqueue_us", host), ("hip_event_us", dev)):
        med = {k: statistics.median(v) for k, v in t.items()}
        out[what] = dict(median={k: round(v, 2) for k, v in med.items()}, min={k: round(min(v), 2) for k, v in t.items()},
                         parent_again_over_parent_minus_1=med["parent_again"] / med["parent"] - 1,
                         this_build_again_over_this_build_minus_1=med["this_build_again"] / med["this_build"] - 1,
                         this_build_over_parent_minus_1=med["this_build"] / med["parent"] - 1)
    for e in (new, old, old2):
        e.close()
    return out


def speed(path, steps, warmup):
    """Host enqueue time and HIP-event time of pcad_forward at l32 width, B = 1, L = 512: both creation orders, each with its own
    engines; a figure's A/B difference and A/A spread are the means of the two orders' ratios."""
    cfg = make_config("l32")
    sd = device_weights(cfg, DEV)
    orders = [speed_order(path, cfg, sd, steps, warmup, first) for first in (False, True)]
    out = {}
    for what in ("host_enqueue_us", "hip_event_us"):
        mean = lambda key: sum(o[what][key] for o in orders) / len(orders)
        delta, spread = mean("this_build_over_parent_minus_1"), abs(mean("parent_again_over_parent_minus_1"))
        out[what] = dict(this_build_over_parent_minus_1=round(delta, 5), a_over_a_spread=round(spread, 5), not_slower_beyond_spread=bool(delta <= spread))
    for o in orders:
        for what in ("host_enqueue_us", "hip_event_us"):
            o[what] = {k: round(v, 5) if isinstance(v, float) else v for k, v in o[what].items()}
    return dict(model="l32", dtype="bfloat16", B=1, L=512, steps=steps, warmup=warmup, orders=orders,
                a_over_a="parent_again is a second engine of the parent's library; this_build_again is the same engine as this_build", **out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--baseline-lib", required=True)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "forward_refactor_ab.json"))
    ap.add_argument("--steps", type=int, default=300)
    ap.add_argument("--warmup", type=int, default=20)
    ap.add_argument("--skip-speed", action="store_true")
    ap.add_argument("--skip-bits", action="store_true")
    ap.add_argument("--sizes-only", action="store_true", help="only the size queries (no GPU needed)")
    a = ap.parse_args()
    n_sizes, bad_sizes = sizes(a.baseline_lib)
    print(f"sizes: {n_sizes} handles (geometry x dtype x options), {len(bad_sizes)} with a differing return code, workspace or arena size", flush=True)
    for r in bad_sizes:
        print("SIZE DIFFERS", json.dumps(r), flush=True)
    if a.sizes_only:
        return 1 if bad_sizes else 0
    rows, old_hash = ([], None) if a.skip_bits else bit_for_bit(a.baseline_lib)
    flat = [dict(c, case=r["case"]) for r in rows for c in r["calls"]]
    bad = [c for c in flat if differs(c)]
    res = dict(device=torch.cuda.get_device_name(0), build_hash=engine.load_library().pcad_build_hash().decode(), baseline_build_hash=old_hash,
               size_queries=n_sizes, size_queries_that_differ=len(bad_sizes), cases=len(rows), calls=len(flat), calls_with_differing_bytes=sum(bool(c["differing_bytes"]) for c in flat),
               calls_with_differing_launch_counts=sum(bool(c["differing_launch_classes"]) for c in flat),
               speed=None if a.skip_speed else speed(a.baseline_lib, a.steps, a.warmup), rows=rows)
    print(json.dumps({k: v for k, v in res.items() if k != "rows"}), flush=True)
    for r in bad:
        print("DIFFERS", json.dumps(r), flush=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
    slower = [k for k in ("host_enqueue_us", "hip_event_us") if res["speed"] and not res["speed"][k]["not_slower_beyond_spread"]]
    for k in slower:
        print("SLOWER", k, json.dumps(res["speed"][k]), flush=True)
    return 1 if bad or bad_sizes or slower else 0


if __name__ == "__main__":
    sys.exit(main())
