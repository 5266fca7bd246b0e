"""-m gpu: the kernel families that only a PCAD_DEV=1 developer switch reaches, against the oracle.

The launch dispatch (scan.hip scan_plan, gemm.hip launch_gemm256_t / launch_gemm_nt, api.hip's layout choices) has rungs that the
default engine never takes at a given shape: the 8-wave 256x256 GEMM, the 256x128 GEMM at large shapes, plain (un-blocked) layouts,
one x | z tensor, the separate conv + x_proj GEMM, the run-time-layout scans.  A switch is read once per process, so each case
starts ONE fresh child (tests/_dev_variant_worker.py, subprocess.run with a time limit, one after another) that sets the switch,
runs a two-layer synthetic model (stress weights, [MASK] at the centre) and saves logits and the last hidden state; this process
compares them with the oracle exactly as tests/test_gpu_launch_forms.py does, at its bars: forward_literal and 1e-4 of max for fp32,
forward_strands(rnd=round_bf16, tie_fold=True) and 3e-2 of max for bf16.

Shapes: the smallest at which the switch still changes the route, followed through the walk of THAT engine.
  * PCAD_GEMM_NOQUAD (the 8-wave 256x256 kernel instead of the 4-wave one): d_model 256, B 4, L 256 - in_proj [2 048, 256] x
    [1 024, 256]^T in whole 256x256 tiles through launch_gemm_nt_two.  The switch does not reach a launch with a fused epilogue, and
    the bf16 default is the norm-folded walk whose in_proj (EPI_SCALE) and out_proj (EPI_RES) both have one, so the bf16 case runs
    under "norm_fold" 0; the fp32 default is unfolded.
  * PCAD_GEMM_NO256 (the 256x128 kernel where launch_gemm_nt would take a 256x256 one: M >= 2048 && N >= 512): only the plain
    out_proj goes through launch_gemm_nt and its N is d_model, so d_model 512, B 4, L 256 - M 2 048, N 512, exactly the
    threshold.  bf16 (folded): the last block's out_proj; fp32: both.  (At d_model 256 no launch of the walk is ever `big`.)
  * the layout switches and PCAD_SCAN_F32_GENERIC at d_model 128, B 3, L 64.
  * PCAD_SCAN_NOPRE96 at dt_rank 80 (Rp 96), B 3, L 77 - and, because L % 8 != 0 takes the run-time-layout scan with or without the
    switch, also at L 80, where the switch is what turns the prefetching walk off.

What the kernel-class counters of pcad_profile_read can show is asserted: with PCAD_PLAIN_LAYOUT, PCAD_PLAIN_XZ or PCAD_NO_CONVX
the fused conv + x_proj kernel is off, so the x_proj GEMM class has launches (the default engine at the same shape has none).
PCAD_GEMM_NOQUAD, PCAD_GEMM_NO256, PCAD_SCAN_F32_GENERIC and PCAD_SCAN_NOPRE96 swap one kernel for another of the SAME class:
their effect cannot be observed that way, only that the result still meets the oracle.

A child that is killed by a signal, aborts or reaches its time limit ends the whole run (pytest.exit): nothing further is started
on that GPU."""
import json
import os
import subprocess
import sys

import pytest
import torch

from _dev_variant_worker import run, setup
from oracle import caduceus_oracle as O

pytestmark = pytest.mark.gpu
WORKER = os.path.join(os.path.dirname(os.path.abspath(__file__)), "_dev_variant_worker.py")
CHILD_LIMIT = 180       # seconds: a child is an interpreter start, one bind and one forward (~15 s)

SMALL = (128, None, 3, 64)              # (d_model, dt_rank (None: auto), B, L)
# (switch, dtype, shape, engine options)
CASES = [("PCAD_GEMM_NOQUAD", "bf16", (256, None, 4, 256), {"norm_fold": 0}),
         ("PCAD_GEMM_NOQUAD", "fp32", (256, None, 4, 256), {}),
         ("PCAD_GEMM_NO256", "bf16", (512, None, 4, 256), {}),
         ("PCAD_GEMM_NO256", "fp32", (512, None, 4, 256), {})]
CASES += [(sw, dt, SMALL, {}) for sw in ("PCAD_PLAIN_LAYOUT", "PCAD_PLAIN_XZ", "PCAD_NO_CONVX") for dt in ("bf16", "fp32")]
CASES += [("PCAD_SCAN_F32_GENERIC", "fp32", SMALL, {}),
          ("PCAD_SCAN_NOPRE96", "bf16", (128, 80, 3, 77), {}),
          ("PCAD_SCAN_NOPRE96", "bf16", (128, 80, 3, 80), {})]
X_PROJ_GEMM = ("PCAD_PLAIN_LAYOUT", "PCAD_PLAIN_XZ", "PCAD_NO_CONVX")      # switches after which x_proj runs as its own GEMM
_ORACLE, _DEFAULT = {}, {}


def oracle(shape, bf16):
    if (shape, bf16) not in _ORACLE:
        cfg, sd, ids = setup(*shape)
        if bf16:
            r = O.forward_strands(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16, tie_fold=True)
        else:
            r = O.forward_literal(ids, O.params_from_state_dict(sd, cfg))
        _ORACLE[(shape, bf16)] = (r["logits"].float(), r["hidden"].float())
    return _ORACLE[(shape, bf16)]


def default_stats(shape, dt):
    """launch counts of the engine WITHOUT a switch (this process), what a switch's effect is read against"""
    if (shape, dt) not in _DEFAULT:
        cfg, sd, ids = setup(*shape)
        _DEFAULT[(shape, dt)] = run(cfg, sd, ids, torch.bfloat16 if dt == "bf16" else torch.float32)["stats"]
    return _DEFAULT[(shape, dt)]


def rel(a, b):
    return ((a - b).abs().max() / b.abs().max()).item()


@pytest.mark.parametrize("switch,dt,shape,opts", CASES, ids=[f"{sw}-{dt}-D{sh[0]}-L{sh[3]}" for sw, dt, sh, _ in CASES])
def test_dev_switch_vs_oracle(switch, dt, shape, opts, tmp_path):
    out = str(tmp_path / "out.pt")
    D, R, B, L = shape
    try:
        p = subprocess.run([sys.executable, WORKER, switch, dt, str(D), "auto" if R is None else str(R), str(B), str(L), json.dumps(opts),
                            out],
                           capture_output=True, text=True, timeout=CHILD_LIMIT)
    except subprocess.TimeoutExpired:
        pytest.exit(f"{switch} {dt}: the child reached its {CHILD_LIMIT} s limit; nothing further is started on this GPU", returncode=3)
    if p.returncode < 0 or p.returncode in (124, 134, 137, 139) or "illegal memory access" in p.stderr:
        pytest.exit(f"{switch} {dt}: the child died with status {p.returncode}; nothing further is started on this GPU\n{p.stderr[-2000:]}",
                    returncode=3)
    assert p.returncode == 0, p.stderr[-4000:]
    got = torch.load(out)
    bf16 = dt == "bf16"
    want_lg, want_h = oracle(shape, bf16)
    assert torch.isfinite(got["logits"]).all() and torch.isfinite(got["hidden"]).all()
    e_l, e_h = rel(got["logits"], want_lg), rel(got["hidden"], want_h)
    print(f"{switch} {dt} {shape} {opts}: logits {e_l:.1e} hidden {e_h:.1e}; launches {got['stats']}")
    bar = 3e-2 if bf16 else 1e-4
    assert e_l <= bar and e_h <= bar, (switch, dt, e_l, e_h)
    if not bf16:
        c = L // 2
        assert torch.equal(got["logits"][:, c, 3:7].argmax(-1), want_lg[:, c, 3:7].argmax(-1))
    if opts.get("norm_fold") == 0:          # the unfolded walk the case is about: no out_proj + residual launch
        assert got["stats"].get("gemm_out_proj_res", 0) == 0, got["stats"]
    if switch in X_PROJ_GEMM:
        assert default_stats(shape, dt).get("gemm_x_proj", 0) == 0, default_stats(shape, dt)
        assert got["stats"].get("gemm_x_proj", 0) > 0, got["stats"]
