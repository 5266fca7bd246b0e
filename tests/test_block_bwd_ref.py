"""CPU checks behind tests/test_gpu_block_bwd.py: the restatements of tests/block_bwd_ref.py are the operators the oracle computes and
their autograd gradients are the derivatives (central finite differences in float64); include/pcad_bwd.h, engine.BWD_SIGNATURES and
libpcad_bwd.so agree with each other; and the two C entries size their scratch and refuse bad arguments before any device work."""
import os
import re
import subprocess

import pytest
import torch

import block_bwd_ref as BB
import scan_bwd_ref as SB
from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def test_bwd_abi_header_signatures_and_library_agree(lib):
    """include/pcad_bwd.h, engine.BWD_SIGNATURES and libpcad_bwd.so name the same pcad_* symbols - held to each other, not to a list,
    so that a later backward operator is added to all three and to nothing else - and none of them belongs to the other two libraries"""
    hdr = open(os.path.join(ROOT, "include", "pcad_bwd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    declared = set(re.findall(r"\b(pcad_[a-z0-9_]+)\s*\(", hdr))
    assert declared and declared == set(engine.BWD_SIGNATURES)
    out = subprocess.run(["nm", "-D", "--defined-only", engine.BWD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert {ln.split()[-1] for ln in out.splitlines() if ln.split()[-1].startswith("pcad_")} == declared
    assert not declared & set(engine.SIGNATURES) and not declared & set(engine.TRAIN_SIGNATURES)
    for name in declared:
        assert hasattr(lib, name), name


@pytest.mark.parametrize("reverse", [False, True])
def test_conv_restatement_is_the_oracles_operator(reverse):
    c = BB.conv_inputs(3, 2, 37, 24)
    f = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    ref = f(O.causal_conv1d_fn(f(c["x"].transpose(1, 2)), c["w"], c["b"], activation="silu")).transpose(1, 2)
    for dtype in (torch.float64, torch.float32):
        assert SB.metric(BB.conv_forward(c["x"], c["w"], c["b"], reverse, dtype), ref) < 1e-6


@pytest.mark.parametrize("residual", [False, True])
def test_norm_restatement_is_the_oracles_operator(residual):
    c = BB.norm_inputs(4, 7, 48, residual=residual)
    ref_y, ref_r = O.rms_norm_fn(c["x"], c["weight"], None, c["residual"], eps=c["eps"], prenorm=True, residual_in_fp32=True)
    ref_plain = O.rms_norm_fn(c["x"], c["weight"], None, c["residual"], eps=c["eps"])
    for dtype in (torch.float64, torch.float32):
        y, r = BB.norm_forward(c["x"], c["residual"], c["weight"], c["eps"], dtype)
        assert SB.metric(y, ref_y) < 1e-6 and SB.metric(r, ref_r) < 1e-6 and SB.metric(y, ref_plain) < 1e-6


def _finite_differences(c, names, loss, grads):
    """central differences of loss(c) in float64 over every coordinate of the named inputs, step 1e-6 (truncation and cancellation both
    ~1e-10 of the gradient), held to 1e-6 of each gradient's maximum"""
    eps = 1e-6
    for name in names:
        base = c[name].double()
        fd = torch.zeros_like(base).reshape(-1)
        for i in range(base.numel()):
            vals = []
            for sign in (1.0, -1.0):
                t = base.clone().reshape(-1)
                t[i] += sign * eps
                vals.append(loss(dict(c, **{name: t.reshape(base.shape)})))
            fd[i] = (vals[0] - vals[1]) / (2 * eps)
        assert (fd.reshape(base.shape) - grads[name]).abs().max().item() < 1e-6 * grads[name].abs().max().item(), name


@pytest.mark.parametrize("reverse", [False, True])
def test_conv_restatement_gradients_are_the_derivatives(reverse):
    c = BB.conv_inputs(5, 2, 9, 4)
    g = BB.conv_grads(c, reverse)
    _finite_differences(c, ("x", "w", "b"), lambda d: (BB.conv_forward(d["x"], d["w"], d["b"], reverse) * c["dout"].double()).sum().item(), g)


@pytest.mark.parametrize("residual", [False, True])
@pytest.mark.parametrize("prenorm", [False, True])
def test_norm_restatement_gradients_are_the_derivatives(residual, prenorm):
    c = BB.norm_inputs(6, 3, 16, residual=residual, prenorm=prenorm)
    g = BB.norm_grads(c)

    def loss(d):
        y, r = BB.norm_forward(d["x"], d["residual"], d["weight"], d["eps"])
        v = (y * c["dy"].double()).sum()
        return (v + (r * c["dres_out"].double()).sum()).item() if prenorm else v.item()
    _finite_differences(c, ("x", "weight") + (("residual",) if residual else ()), loss, g)


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int CONV_BWD_SEG = (\d+);", src).group(1)) == ops.CONV_BWD_SEG
    assert int(re.search(r"constexpr int NORM_BWD_ROWS = (\d+);", src).group(1)) == ops.NORM_BWD_ROWS


def test_scratch_bytes_monotone_multiples_of_256(lib):
    f, G = lib.pcad_causal_conv1d_silu_bwd_scratch_bytes, ops.CONV_BWD_SEG
    prev = None
    for args in ((1, 1, 8), (2, 1, 8), (2, G, 8), (2, G + 1, 8), (2, G + 1, 128), (3, 2 * G + 5, 128), (3, 2 * G + 5, 2048)):
        n = f(*args)
        assert n > 0 and n % 256 == 0 and (prev is None or n >= prev), args
        prev = n
    assert f(2, G + 1, 128) > f(2, G, 128) and f(3, G, 128) > f(2, G, 128) and f(2, G, 256) > f(2, G, 128)
    assert f(2, G + 1, 128) >= 2 * 2 * 5 * 128 * 4                     # one row of dw | db partials per (strand, segment)
    assert f(0, 5, 128) == 0 and f(2, 0, 128) == 0
    h, Rw = lib.pcad_add_rmsnorm_bwd_scratch_bytes, ops.NORM_BWD_ROWS
    prev = None
    for args in ((1, 8), (Rw, 8), (Rw + 1, 8), (Rw + 1, 384), (2 * Rw + 3, 384), (2 * Rw + 3, 2048), (1 << 33, 2048)):
        n = h(*args)
        assert n > 0 and n % 256 == 0 and (prev is None or n >= prev), args
        prev = n
    assert h(Rw + 1, 384) > h(Rw, 384) and h(Rw, 768) > h(Rw, 384)
    assert h(2 * Rw + 3, 384) >= 3 * 384 * 4                           # one dweight partial row per slab
    assert h(0, 384) == 0


def test_conv_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor"""
    p = 0x10000
    last = engine.load_library().pcad_last_error          # the message is libpcad.so's, on the calling thread

    def call(x=p, ldx=None, w=p, b=p, dout=p, dx=p, dw=p, db=p, scratch=p, nbytes=1 << 30, S=2, L=5, E=128, dtype=0):
        return lib.pcad_causal_conv1d_silu_bwd(x, E if ldx is None else ldx, w, b, dout, dx, dw, db, scratch, nbytes, S, L, E, 0, dtype, None)
    for name in ("x", "w", "b", "dout", "dx", "dw", "db"):
        assert call(**{name: None}) == INV and name.encode() in last(), name
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(E=132, dtype=1) == INV and b"E" in last()           # bf16: 8 elements per 16 bytes
    assert call(E=130, dtype=0) == INV and b"E" in last()           # fp32: 4
    assert call(ldx=130) == INV and b"ldx" in last()
    assert call(ldx=260, dtype=1) == INV and b"ldx" in last()
    assert call(ldx=120) == INV and b"ldx" in last()                # ldx < E
    assert call(x=p + 8) == INV and b"x" in last()
    assert call(dout=p + 4) == INV and b"dout" in last()
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    assert call(ldx=256, nbytes=0) == WSP                           # ldx = 2 E passes every argument check: it gets as far as the scratch
    # nothing to do: OK before the scratch is looked at
    assert call(S=0, scratch=None, nbytes=0) == 0 and call(L=0, scratch=None, nbytes=0) == 0


def test_norm_entry_refuses_bad_arguments_without_a_device(lib):
    p = 0x10000
    last = engine.load_library().pcad_last_error

    def call(x=p, res=p, w=p, dy=p, dres_out=p, dx=p, dres_in=p, dw=p, scratch=p, nbytes=1 << 30, rows=5, D=384, dtype=0, rdt=0):
        return lib.pcad_add_rmsnorm_bwd(x, res, w, dy, dres_out, dx, dres_in, dw, scratch, nbytes, rows, D, 1e-5, dtype, rdt, None)
    for name, word in (("x", b"x"), ("w", b"weight"), ("dy", b"dy"), ("dx", b"dx"), ("dw", b"dweight")):
        assert call(**{name: None}) == INV and word in last(), name
    assert call(dres_in=None) == INV and b"dresidual_in" in last()   # residual_in without dresidual_in
    assert call(res=None) == INV and b"dresidual_in" in last()       # ... and the converse
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(rdt=7) == INV and b"res_dtype" in last()
    assert call(dtype=0, rdt=1) == INV and b"res_dtype" in last()    # an fp32 model keeps an fp32 residual stream
    assert call(D=388) == INV and b"D" in last()
    assert call(D=2056) == INV and b"D" in last() and b"2048" in last()
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    assert call(rows=0, scratch=None, nbytes=0) == 0
    assert call(rows=0, res=None, dres_in=None, dres_out=None, scratch=None, nbytes=0) == 0
