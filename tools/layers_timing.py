"""Time the per-layer hidden-state forward (pcad_forward_layers) against the calls it restates, at the l32 geometry,
64 x 512 bp, bf16, position 255, same process, interleaved, HIP events:

  pair "all_levels"   (a)  pcad_forward_all_hidden, all_hidden [32, B, L, 2D] + hidden_out [B, L, 2D]
                      (b)  pcad_forward_layers, all 33 levels at position 255, out [33, B, 1, 2D]       - the same layer walk
  pair "last_level"   (a)  pcad_forward(positions=[255]), hidden_out [B, 1, 2D]
                      (b)  pcad_forward_layers(layers=[n_layer], positions=[255]), out [1, B, 1, 2D]    - the same walk + one small launch
  pairs "level_1", "level_mid", "level_below_top", "levels_4_mid": layers = [1], [n_layer / 2], [n_layer - 1], [4, n_layer / 2]
                      (a)  pcad_forward_layers(layers, positions=[255]) on the baseline library: all n_layer blocks
                      (b)  the same call on this build: K blocks for the highest level K, block K - 1 shortened to walk_len steps.
                           Recorded beside the ratio: what construction predicts, (K - 1 + walk_len / L) / n_layer of the parent's
                           block time (embedding, row gathers and the head / id check are outside that figure)

(a) runs on --baseline-lib (a libpcad.so built from the parent commit) when given, else on this build.  One round = (a), (b), (a')
once each in that order, (a') being the same call as (a) again: the A/A spread the result is read against; the figure of a series
is the median over the rounds.  Synthetic weights generated on the device (timing only).

Every pair runs in a child process of its own under its own time limit, one after the other; a pair that fails or runs out of time
ends the run (nothing further is started on the device).

    python tools/layers_timing.py [--out profiles/layers_timing.json] [--steps 20] [--warmup 3] [--baseline-lib PATH]
"""
import argparse
import json
import os
import statistics
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

PAIRS = ("all_levels", "last_level", "level_1", "level_mid", "level_below_top", "levels_4_mid")
PAIR_LIMIT_S = 240            # per pair: engine build + (warmup + steps) x 3 forwards of ~0.1 s
B, L, POS = 64, 512, 255


def run_pair(a):
    import torch
    from plantcaduceus_amd import engine
    from plantcaduceus_amd.checkpoint import make_config
    from mlm_loss_timing import baseline_engine, event_ms
    from seqcls_timing import device_weights
    dev = torch.device("cuda:0")
    cfg = make_config("l32")
    sd = device_weights(cfg, dev)
    eng = engine.Engine(cfg, sd, torch.bfloat16, dev)
    base, base_hash = (baseline_engine(a.baseline_lib, cfg, sd, torch.bfloat16, dev) if a.baseline_lib
                       else (eng, eng.lib.pcad_build_hash().decode()))
    ids = torch.randint(3, 7, (B, L), device=dev, generator=torch.Generator(device=dev).manual_seed(1))
    if a.pair == "all_levels":
        fa = lambda: base.forward(ids, want_hidden=True, want_logits=False, all_hidden=True)          # noqa: E731
        fb = lambda: eng.forward_layers(ids, None, positions=[POS])                                   # noqa: E731
    elif a.pair == "last_level":
        fa = lambda: base.forward(ids, positions=[POS], want_hidden=True, want_logits=False)          # noqa: E731
        fb = lambda: eng.forward_layers(ids, [cfg.n_layer], positions=[POS])                          # noqa: E731
    else:
        nl = cfg.n_layer
        layers = {"level_1": [1], "level_mid": [nl // 2], "level_below_top": [nl - 1], "levels_4_mid": [4, nl // 2]}[a.pair]
        fa = lambda: base.forward_layers(ids, layers, positions=[POS])                                # noqa: E731
        fb = lambda: eng.forward_layers(ids, layers, positions=[POS])                                 # noqa: E731
        walk_len = min(L, (max(POS + 1, L - POS) + 7) // 8 * 8)           # csrc/forward.hip plan_forward
        predicted = (layers[-1] - 1 + walk_len / L) / nl
    series = {"a_parent_call": fa, "b_forward_layers": fb, "a2_parent_call_again": fa}
    for _ in range(a.warmup):
        for fn in series.values():
            fn()
    torch.cuda.synchronize()
    ms = {k: [] for k in series}
    for _ in range(a.steps):
        for k, fn in series.items():
            ms[k].append(event_ms(fn))
    eng.check_status()
    med = {k: statistics.median(v) for k, v in ms.items()}
    aa = abs(med["a2_parent_call_again"] / med["a_parent_call"] - 1)
    ratio = med["b_forward_layers"] / med["a_parent_call"]
    r = dict(pair=a.pair, model="l32", dtype="bfloat16", B=B, L=L, position=POS, steps=a.steps, warmup=a.warmup,
             build_hash=eng.lib.pcad_build_hash().decode(), baseline_build_hash=base_hash,
             median_ms={k: round(v, 3) for k, v in med.items()}, min_ms={k: round(min(v), 3) for k, v in ms.items()},
             b_over_a=round(ratio, 5), a_over_a_spread=round(aa, 5), b_not_slower_beyond_3pct=bool(ratio <= 1.03))
    if a.pair not in ("all_levels", "last_level"):
        r.update(layers=layers, walk_len=walk_len, predicted_b_over_a=round(predicted, 5), b_below_a_beyond_spread=bool(ratio < 1 - aa))
    print(json.dumps(r), flush=True)
    with open(a.part, "w") as f:
        json.dump(dict(device=torch.cuda.get_device_name(0), row=r), f)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--baseline-lib", default=None)
    ap.add_argument("--pair", choices=PAIRS, default=None, help="(internal) run one pair in this process")
    ap.add_argument("--part", default=None, help="(internal) where the pair's row is written")
    a = ap.parse_args()
    if a.pair:
        return run_pair(a)
    rows, device = [], None
    with tempfile.TemporaryDirectory() as tmp:
        for pair in PAIRS:
            part = os.path.join(tmp, pair + ".json")
            cmd = ["timeout", "-k", "10", str(PAIR_LIMIT_S), sys.executable, os.path.abspath(__file__), "--pair", pair, "--part", part,
                   "--steps", str(a.steps), "--warmup", str(a.warmup)] + (["--baseline-lib", a.baseline_lib] if a.baseline_lib else [])
            rc = subprocess.run(cmd).returncode
            if rc != 0:
                sys.exit(f"pair {pair} ended with status {rc}: nothing further is started")
            with open(part) as f:
                got = json.load(f)
            device = got["device"]
            rows.append(got["row"])
    if a.out:
        with open(a.out, "w") as f:
            json.dump({"device": device, "rows": rows}, f, indent=1)


if __name__ == "__main__":
    main()
