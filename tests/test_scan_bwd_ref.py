"""CPU checks behind tests/test_gpu_scan_bwd.py: the reference of tests/scan_bwd_ref.py is the operator the oracle computes and its
autograd gradients are the derivatives (central finite differences in float64), and the C entry pcad_selective_scan_bwd sizes its
scratch and refuses bad arguments before any device work."""
import ctypes as C
import os
import re

import pytest
import torch

import scan_bwd_ref as SB
from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.TRAIN_LIB_PATH):
        engine.build_library()
    return engine.load_train_library()


def test_train_abi_header_signatures_and_library_agree(lib):
    """include/pcad_train.h, engine.TRAIN_SIGNATURES and libpcad_train.so name the same symbols (as tests/test_host.py holds for
    include/pcad.h), and the backward entries live in that library only: libpcad.so's own export list is pinned elsewhere"""
    import subprocess
    hdr = open(os.path.join(ROOT, "include", "pcad_train.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pcad_[a-z0-9_]+)\s*\(", hdr))
    assert declared == set(engine.TRAIN_SIGNATURES) == {"pcad_selective_scan_bwd", "pcad_selective_scan_bwd_scratch_bytes"}
    out = subprocess.run(["nm", "-D", "--defined-only", engine.TRAIN_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("pcad_")} == declared
    assert not declared & set(engine.SIGNATURES)


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("gated", [True, False])
def test_restatement_forward_is_the_oracles_operator(reverse, gated):
    x = SB.inputs(5, 2, 40, 33)
    if not gated:
        x["z"] = None
    got = SB.forward(x, reverse)
    f = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    ref = f(O.selective_scan_fn(f(x["u"]), f(x["delta"]), x["A"], f(x["B"]), f(x["C"]), x["D"], z=f(x["z"]) if gated else None,
                                delta_bias=x["delta_bias"], delta_softplus=True))
    assert SB.metric(got, ref) < 1e-6


@pytest.mark.parametrize("reverse", [False, True])
def test_restatement_gradients_are_the_derivatives(reverse):
    """autograd vs central finite differences of sum(out * dout), float64, (B, E, L) = (1, 64, 9), up to 256 sampled coordinates of
    every input; one coordinate is perturbed per batch copy, so a whole sample costs two forward walks.  Step 1e-6 in float64: the
    truncation (h^2 f''' / 6) and the cancellation (1e-16 / h) are both ~1e-10 of the gradient, held to 1e-6 of its maximum."""
    x = SB.inputs(9, 1, 64, 9)
    g = SB.grads(x, reverse)
    gen = torch.Generator().manual_seed(1)
    eps = 1e-6
    for name in SB.NAMES:
        n = x[name].numel()
        K = min(n, 256)
        idx = torch.randperm(n, generator=gen)[:K]
        batched = {k: (x[k].double().expand(K, *x[k].shape[1:]) if k in ("u", "delta", "B", "C", "z") else x[k].double().expand(K, *x[k].shape))
                   for k in SB.NAMES}
        vals = []
        for sign in (1.0, -1.0):
            t = batched[name].clone().reshape(K, -1)
            t[torch.arange(K), idx] += sign * eps
            out = SB.forward(dict(batched, **{name: t.reshape(batched[name].shape)}), reverse)
            vals.append((out * x["dout"].double()).sum(dim=(1, 2)))
        fd = (vals[0] - vals[1]) / (2 * eps)
        an = g[name].reshape(-1)[idx]
        assert (fd - an).abs().max().item() < 1e-6 * g[name].abs().max().item(), name


def test_fp32_autograd_leaves_the_floor_in_charge():
    """what the bars are made of: fp32 CPU autograd through the restatement is far inside BAR_SCAN on every gradient, and no gradient
    tensor is degenerate"""
    for (Bsz, E, L), reverse in (((2, 128, 40), False), ((3, 64, 65), True)):
        x, g64, dev32 = SB.reference(("floor", Bsz, E, L), lambda: SB.inputs(L, Bsz, E, L), reverse)
        for name in SB.NAMES:
            assert dev32[name] < 3e-6, (name, dev32[name])
            assert g64[name].abs().max().item() > 1.0, name


def test_chunk_constant_matches_the_kernel():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int SCAN_BWD_CHUNK = (\d+);", src).group(1)) == ops.SCAN_BWD_CHUNK


def test_scratch_bytes_positive_and_monotone(lib):
    f = lib.pcad_selective_scan_bwd_scratch_bytes
    base = f(2, 17, 128)
    assert base > 0 and base % 256 == 0
    assert f(3, 17, 128) > base and f(2, 18, 128) > base and f(2, 17, 192) > base
    T = ops.SCAN_BWD_CHUNK
    assert f(2, T + 1, 128) > f(2, T, 128)
    # at least the states at the chunk boundaries and the per-wave partials of dB | dC
    assert f(4, 64, 256) >= 4 * (64 // T - 1) * 16 * 256 * 4 + 4 * 64 * 4 * 32 * 4
    assert f(0, 17, 128) == 0 and f(2, 0, 128) == 0 and f(2, 17, 96) == 0


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null value stands for a tensor"""
    p = 0x10000

    def call(E=128, dout=p, z=p, dz=p, bc=p, dbc=p, dtype=0, scratch=p, nbytes=1 << 30, S=2, L=5):
        return lib.pcad_selective_scan_bwd(p, p, z, E, bc, p, p, p, dout, p, p, dz, dbc, p, p, p, scratch, nbytes, S, L, E, 0, dtype, None)
    inv, wsp = -1, -3
    last = engine.load_library().pcad_last_error          # the message is libpcad.so's, on the calling thread
    assert call(E=96) == inv and b"E" in last()
    assert call(dout=None) == inv and b"dout" in last()
    assert call(dz=None) == inv and b"dz" in last()
    assert call(z=None) == inv and b"dz" in last()
    assert call(dtype=7) == inv and b"dtype" in last()
    assert call(bc=p + 4) == inv and b"bc" in last()
    assert call(dbc=p + 8) == inv and b"dbc" in last()
    assert call(scratch=p + 16) == wsp and call(scratch=None) == wsp and call(nbytes=1024) == wsp
    assert b"scratch" in last()
    # nothing to do: OK before the scratch is looked at
    assert call(S=0, scratch=None, nbytes=0) == 0 and call(L=0, scratch=None, nbytes=0) == 0
