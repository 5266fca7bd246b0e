"""Inputs shared by tests/test_untied.py and tests/test_gpu_untied.py (test helper): synthetic checkpoints whose mamba_rev has its
own in_proj / out_proj, and the oracle runs on them, computed once per process."""
import math

import numpy as np
import torch

from oracle import caduceus_oracle as O
from plantcaduceus_amd.checkpoint import layer_keys, make_config, synthetic_state_dict

TOY = dict(d_model=128, n_layer=2)      # a toy geometry of tests/test_gpu_model.py (E = 256, dt_rank 8)
B, L = 3, 70                            # L = 70: no multiple of 8 (row blocks) or 64 (conv segments, tiles)


def untied_state_dict(cfg, seed, tie=False, stress=True):
    """checkpoint.synthetic_state_dict (stress: its perturbed variant, the suite's default) with mamba_rev.in_proj / out_proj replaced by independent draws of the same scale
    (tie=True: by clones of mamba_fwd's - distinct tensors, tied values)."""
    sd = dict(synthetic_state_dict(cfg, seed=seed, stress=stress))
    rng = np.random.default_rng(seed + 1000)
    D, E = cfg.d_model, cfg.d_inner
    for i in range(cfg.n_layer):
        f, r = layer_keys(i, "fwd"), layer_keys(i, "rev")
        if tie:
            sd[r["in_proj"]], sd[r["out_proj"]] = sd[f["in_proj"]].clone(), sd[f["out_proj"]].clone()
        else:
            sd[r["in_proj"]] = torch.from_numpy(rng.uniform(-D ** -0.5, D ** -0.5, (2 * E, D)).astype(np.float32))
            sd[r["out_proj"]] = torch.from_numpy(rng.uniform(-E ** -0.5, E ** -0.5, (D, E)).astype(np.float32)) / math.sqrt(cfg.n_layer)
    return sd


def retied(sd, cfg):
    """sd with mamba_rev := mamba_fwd for in_proj / out_proj: what an engine that reads 'the first of each pair' computes."""
    out = dict(sd)
    for i in range(cfg.n_layer):
        f, r = layer_keys(i, "fwd"), layer_keys(i, "rev")
        out[r["in_proj"]], out[r["out_proj"]] = sd[f["in_proj"]], sd[f["out_proj"]]
    return out


def rand_ids(nb, length, seed, mask=None):
    ids = torch.randint(3, 7, (nb, length), generator=torch.Generator().manual_seed(seed))
    ids[0, 0] = 2
    if mask is not None:
        ids[:, mask] = 1
    return ids


_CACHE = {}


def toy_case(stress=True):
    """-> dict(cfg, sd, ids, ref (fp32 forward_strands tie_fold=False), lit (forward_literal), ref_bf16, tied / tied_bf16 (mamba_rev :=
    mamba_fwd)).  stress=False: the checkpoint's plain variant (small embedding, unit norm weights): there the mixers, not the
    embedding, make the residual stream, so untying moves the logits by half their range - enough to tell the forms apart at the
    bf16 bar too (on the stress variant the logits move by 2 % of their range: 100x the fp32 bar, but below the bf16 one)."""
    key = ("toy", stress)
    if key not in _CACHE:
        cfg = make_config("x", **TOY)
        sd = untied_state_dict(cfg, seed=31, stress=stress)
        ids = rand_ids(B, L, 5, mask=L // 2 - 1)
        P = O.params_from_state_dict(sd, cfg)
        bf = lambda s: O.forward_strands(ids, O.params_from_state_dict(s, cfg, dtype=torch.bfloat16), rnd=O.round_bf16, tie_fold=False)
        _CACHE[key] = dict(
            cfg=cfg, sd=sd, ids=ids, ref=O.forward_strands(ids, P, tie_fold=False), lit=O.forward_literal(ids, P),
            ref_bf16=bf(sd), tied_bf16=bf(retied(sd, cfg)),
            tied=O.forward_strands(ids, O.params_from_state_dict(retied(sd, cfg), cfg), tie_fold=False))
    return _CACHE[key]


def rel(a, b):
    """max |a - b| of the range of b."""
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()
