"""Child of tests/test_gpu_dev_variants.py: one forward of a two-layer synthetic model with ONE PCAD_DEV=1 developer switch set.

The switches (plantcaduceus_amd/csrc: dev_env) are read once per process, so every case needs a process of its own: this one sets
the switch before the library is loaded, runs the model with the kernel-class profile on and saves logits, the last hidden state and
the per-class launch counts for the parent, which holds the oracle.  `setup` is shared with the parent so that both build the same
weights and ids.
Not collected by pytest (leading underscore)."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def setup(D, dt_rank, B, L):
    """-> (config, state dict, ids [B, L] with [MASK] at the centre); dt_rank None: "auto" = ceil(D / 16)"""
    import torch
    from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
    kw = {} if dt_rank is None else dict(ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=dt_rank, bias=False, conv_bias=True))
    cfg = make_config("x", d_model=D, n_layer=2, **kw)
    sd = synthetic_state_dict(cfg, seed=D + L + B, stress=True)
    ids = torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(L + B))
    ids[:, L // 2] = 1
    return cfg, sd, ids


def run(cfg, sd, ids, dtype, opts=None):
    """-> dict(logits, hidden, stats): one profiled forward on cuda:0; opts: engine options (pcad_set_option)"""
    import torch
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    cfg.engine_options = dict(opts or {})
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    m = m.to(dtype).to("cuda:0").eval()
    eng = m._engine()
    eng.profile(1)
    out = m(input_ids=ids.to("cuda:0"), output_hidden_states=True)
    torch.cuda.synchronize()
    stats = eng.profile_read()
    eng.profile(False)
    return dict(logits=out.logits.float().cpu(), hidden=out.hidden_states[-1].float().cpu(), stats={k: v[0] for k, v in stats.items()})


def main(switch, dtype, D, dt_rank, B, L, opts, out):
    os.environ["PCAD_DEV"] = "1"
    os.environ[switch] = "1"
    import torch
    cfg, sd, ids = setup(int(D), None if dt_rank == "auto" else int(dt_rank), int(B), int(L))
    torch.save(run(cfg, sd, ids, torch.bfloat16 if dtype == "bf16" else torch.float32, json.loads(opts)), out)


if __name__ == "__main__":
    main(*sys.argv[1:])
