"""Wall time of plantcad2_eval.sv_effect on synthetic structural variants (default 64 SVs x 8 192-bp windows, PlantCAD2 Small bf16,
synthetic weights): one warm-up call, then the median of --steps timed calls.  With --dense the dense path is forced (the [n, L, 4]
probabilities are kept: what `--save_ref_logits` runs).  Run from a checkout of another commit to time that commit's sv_effect.

    python tools/sv_effect_wall.py [--n 64] [--L 8192] [--steps 3] [--batch-size 32] [--dense]
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

import numpy as np  # noqa: E402
import pandas as pd  # noqa: E402
import torch  # noqa: E402

from plantcaduceus_amd import plantcad2_eval as pe  # noqa: E402
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict  # noqa: E402
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM  # noqa: E402
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--n", type=int, default=64)
    ap.add_argument("--L", type=int, default=8192)
    ap.add_argument("--steps", type=int, default=3)
    ap.add_argument("--batch-size", type=int, default=32)
    ap.add_argument("--size", default="pc2-small")
    ap.add_argument("--dense", action="store_true")
    a = ap.parse_args()
    cfg = make_config(a.size)
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(synthetic_state_dict(cfg, seed=1, stress=False), strict=False)
    m.tie_weights()
    m = m.to(torch.bfloat16).to("cuda:0").eval()
    rng = np.random.default_rng(0)
    F = 5
    mk = lambda: "".join(rng.choice(list("ACGT"), size=a.L))
    df = pd.DataFrame({"RefSeq": [mk() for _ in range(a.n)], "MutSeq": [mk() for _ in range(a.n)],
                       "left": rng.integers(F + 1, a.L // 2, size=a.n), "right": rng.integers(a.L // 2, a.L - F, size=a.n),
                       "label": rng.integers(0, 2, size=a.n)})
    tok = CaduceusTokenizer()
    sparse = bool(getattr(m, "supports_nucleotide_probs", False)) and not a.dense

    def run():
        if a.dense:
            ref = pe.unmasked_probs(df["RefSeq"], tok, m, "cuda:0", a.batch_size)
            mut = pe.unmasked_probs(df["MutSeq"], tok, m, "cuda:0", a.batch_size)
            return pe.average_precision(df["label"], pe.sv_llr_boundary(df["left"], df["right"], df["MutSeq"], ref, mut, F))
        return pe.sv_effect(df, m, tok, "cuda:0", batch_size=a.batch_size, flanking=F)["AUPRC"]

    auprc = run()
    t = []
    for _ in range(a.steps):
        t0 = time.perf_counter()
        run()
        t.append(time.perf_counter() - t0)
    print(json.dumps(dict(tool="sv_effect_wall", root=ROOT, size=a.size, n=a.n, L=a.L, batch_size=a.batch_size, path="sparse" if sparse else "dense",
                          wall_s_median=round(statistics.median(t), 4), wall_s=[round(x, 4) for x in t], auprc=auprc,
                          bytes_per_sequence_gathered=(2 * F if sparse else a.L) * 16)), flush=True)


if __name__ == "__main__":
    main()
