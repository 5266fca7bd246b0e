"""CPU checks behind tests/test_gpu_optim.py: the restatement of tests/optim_ref.py is clip_grad_norm_ + torch.optim.AdamW (float64);
the chunk count and scratch size of libpcad_bwd.so's optimizer entries are the stated formulas; and the entries refuse bad tables and
arguments before any device work (include/pcad_bwd.h)."""
import ctypes as C
import os
import re

import pytest
import torch

import optim_ref as OR
from plantcaduceus_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE
F32, BF16 = 0, 1
P = 0x10000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


@pytest.mark.parametrize("max_norm,grad_scale", [(0.0, 1.0), (1.0, 1.0), (0.5, 0.25), (1e9, 0.25)])
def test_restatement_is_clip_grad_norm_and_torch_adamw(max_norm, grad_scale):
    """5 steps in float64, mixed decay flags, fresh gradients each step: parameters and both moments within 1e-12 of torch's"""
    g = torch.Generator().manual_seed(3)
    shapes = [(7,), (33, 5), (1,), (4, 4, 3), (129,)]
    decay = [True, False, True, True, False]
    hp = dict(lr=3e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.1)
    init = [torch.randn(s, generator=g, dtype=torch.float64) for s in shapes]
    tp = [torch.nn.Parameter(t.clone()) for t in init]
    opt = OR.torch_adamw(tp, decay, **hp)
    mine, m, v = [t.clone() for t in init], [torch.zeros_like(t) for t in init], [torch.zeros_like(t) for t in init]
    for step in range(1, 6):
        grads = [torch.randn(s, generator=g, dtype=torch.float64) * 3 for s in shapes]
        for p, gr in zip(tp, grads):
            p.grad = gr.clone() * grad_scale
        if max_norm > 0:
            total = torch.nn.utils.clip_grad_norm_(tp, max_norm)
        else:
            total = torch.linalg.vector_norm(torch.stack([torch.linalg.vector_norm(p.grad) for p in tp]))
        opt.step()
        norm, coef, finite = OR.adamw_step(mine, grads, m, v, decay, step=step, max_norm=max_norm, grad_scale=grad_scale, **hp)
        assert finite and abs(norm - total.item()) <= 1e-12 * norm
        for i, (a, b) in enumerate(zip(mine, tp)):
            st = opt.state[b]
            assert (a - b.detach()).abs().max().item() < 1e-12, (step, i)
            assert (m[i] - st["exp_avg"]).abs().max().item() < 1e-12 and (v[i] - st["exp_avg_sq"]).abs().max().item() < 1e-12, (step, i)
    if max_norm <= 0:
        assert coef == grad_scale


def test_restatement_skips_a_non_finite_step():
    p, m, v = [torch.ones(3, dtype=torch.float64)], [torch.zeros(3, dtype=torch.float64)], [torch.zeros(3, dtype=torch.float64)]
    g = [torch.tensor([1.0, float("inf"), 0.0], dtype=torch.float64)]
    norm, _, finite = OR.adamw_step(p, g, m, v, [True], 1e-3, 0.9, 0.999, 1e-8, 0.1, 1, 1.0)
    assert not finite and torch.equal(p[0], torch.ones(3, dtype=torch.float64)) and not m[0].any() and not v[0].any()


def test_constants_match_the_header_and_the_kernels():
    hdr = open(os.path.join(ROOT, "include", "pcad_bwd.h")).read()
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    kern = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "optim.hip")).read()
    assert int(re.search(r"#define PCAD_OPTIM_CHUNK (\d+)", hdr).group(1)) == ops.OPTIM_CHUNK == OR.CHUNK
    assert int(re.search(r"constexpr int OPTIM_CHUNK = (\d+);", src).group(1)) == ops.OPTIM_CHUNK
    assert int(re.search(r"#define PCAD_OPTIM_DECAY (\d+)", hdr).group(1)) == ops.OPTIM_DECAY
    assert int(re.search(r"constexpr int FIN_LANES = (\d+);", kern).group(1)) == OR.FIN_LANES
    assert C.sizeof(ops._optim_record_type()) == 64


def rec(param=P, grad=P, master=None, m=P, v=P, n=5, pdt=F32, gdt=F32, flags=0):
    return (param, grad, master, m, v, n, pdt, gdt, flags)


def plan(lib, records, capacity=None):
    """-> (status, chunks, map or None); capacity None: count only"""
    Record = ops._optim_record_type()
    tab = (Record * max(1, len(records)))()
    for r, x in zip(tab, records):
        r.param, r.grad, r.master, r.exp_avg, r.exp_avg_sq, r.n, r.param_dtype, r.grad_dtype, r.flags = x
    chunks = C.c_int64(-7)
    if capacity is None:
        return lib.pcad_optim_plan(C.addressof(tab), len(records), None, 0, C.byref(chunks)), chunks.value, None
    cmap = (C.c_int32 * max(2, 2 * capacity))()
    rc = lib.pcad_optim_plan(C.addressof(tab), len(records), C.addressof(cmap), capacity, C.byref(chunks))
    return rc, chunks.value, list(cmap)


def test_chunk_count_and_scratch_bytes_are_the_formulas(lib):
    """sizes only, no memory: pointers are never dereferenced"""
    Ck = OR.CHUNK
    for sizes in ([0], [1], [Ck - 1], [Ck], [Ck + 1], list(OR.EDGE_SIZES), [3, 0, 0, Ck * 7 + 1, 0, 5], list(range(1, 51)) * 6,
                  [(1 << 31) + 5, 1 << 31, 77, (1 << 30) + Ck - 1]):                       # the last: 5 * 2^30 + ... > 2^32 elements in all
        rc, chunks, _ = plan(lib, [rec(n=n) for n in sizes])
        assert rc == 0 and chunks == OR.chunk_count(sizes), sizes
    assert OR.chunk_count([(1 << 31) + 5, 1 << 31, 77, (1 << 30) + Ck - 1]) == ((1 << 19) + 1) + (1 << 19) + 1 + ((1 << 18) + 1)
    sizes = [5, 0, 2 * Ck + 1, Ck]
    rc, chunks, cmap = plan(lib, [rec(n=n) for n in sizes], capacity=5)
    assert rc == 0 and chunks == 5 and cmap[:10] == [0, 0, 2, 0, 2, 1, 2, 2, 3, 0]       # never straddling: a tensor's chunks are its own
    f = lib.pcad_adamw_step_scratch_bytes
    for chunks in (0, 1, 63, 64, 65, 300, (1 << 20) + 3, (1 << 31) - 1):
        assert f(chunks) == OR.scratch_bytes(chunks) and f(chunks) % 256 == 0 and f(chunks) >= 4 * chunks, chunks
    assert f(-1) == 0


def test_plan_refuses_bad_tables_without_a_device(lib):
    last = engine.load_library().pcad_last_error
    ok = rec()
    for field in ("param", "grad", "m", "v"):
        word = {"m": b"exp_avg", "v": b"exp_avg_sq"}.get(field, field.encode())
        rc, _, _ = plan(lib, [ok, rec(**{field: P + 8})])
        assert rc == INV and word in last() and b"table[1]" in last() and b"aligned" in last(), field
        rc, _, _ = plan(lib, [rec(**{field: None})])
        assert rc == INV and word in last() and b"null" in last(), field
    rc, _, _ = plan(lib, [rec(master=P + 4)])
    assert rc == INV and b"master" in last() and b"aligned" in last()
    rc, _, _ = plan(lib, [ok, ok, rec(n=-1)])
    assert rc == INV and b"table[2].n" in last()
    rc, _, _ = plan(lib, [rec(pdt=7)])
    assert rc == INV and b"param_dtype" in last()
    rc, _, _ = plan(lib, [rec(gdt=2)])
    assert rc == INV and b"grad_dtype" in last()
    rc, _, _ = plan(lib, [rec(pdt=BF16)])                                  # a bf16 param without master
    assert rc == INV and b"master" in last()
    assert plan(lib, [rec(pdt=BF16, master=P, gdt=BF16)])[0] == 0
    assert plan(lib, [rec(pdt=F32, master=P)])[0] == 0                     # an fp32 param may have one
    rc, _, _ = plan(lib, [rec(flags=2)])
    assert rc == INV and b"flags" in last()
    assert plan(lib, [rec(n=0, param=None, grad=None, m=None, v=None, pdt=BF16)])[:2] == (0, 0)     # n == 0: pointers are not looked at
    rc, _, _ = plan(lib, [rec(n=3 * OR.CHUNK)], capacity=2)
    assert rc == INV and b"chunk_capacity" in last()
    rc, _, _ = plan(lib, [rec(n=(1 << 24) * OR.CHUNK)])                    # one chunk more than PCAD_OPTIM_MAX_CHUNKS
    assert rc == INV and b"2^24" in last()
    assert plan(lib, [rec(n=((1 << 24) - 1) * OR.CHUNK)])[:2] == (0, (1 << 24) - 1)


def test_step_entries_refuse_bad_arguments_without_a_device(lib):
    last = engine.load_library().pcad_last_error

    def step(table=P, cmap=P, count=3, chunks=5, state=P, scratch=P, nbytes=1 << 20, lr=1e-3, b1=0.9, b2=0.999, eps=1e-8, wd=0.0, bc1=0.1,
             bc2=0.001, max_norm=1.0, scale=1.0):
        return lib.pcad_adamw_step(table, cmap, count, chunks, state, scratch, nbytes, lr, b1, b2, eps, wd, bc1, bc2, max_norm, scale, None)
    assert step(nbytes=255) == WSP and b"scratch" in last()                # too small
    assert step(chunks=65, nbytes=256) == WSP and step(scratch=P + 16) == WSP and step(scratch=None) == WSP
    assert step(table=None) == INV and b"table" in last()
    assert step(table=P + 8) == INV and b"table" in last()
    assert step(cmap=None) == INV and b"chunk_map" in last()
    assert step(state=None) == INV and b"state" in last()
    assert step(state=P + 4) == INV and b"state" in last()
    assert step(chunks=-1) == INV and step(count=-1) == INV and step(chunks=1 << 24, nbytes=1 << 27) == INV and b"2^24" in last()
    assert step(bc1=0.0) == INV and b"bc1" in last()
    assert step(bc2=1.5) == INV and b"bc2" in last()
    assert step(lr=float("nan")) == INV and b"lr" in last()
    assert step(max_norm=float("inf")) == INV and b"max_norm" in last()
    assert lib.pcad_zero_grads(None, P, 3, 5, None) == INV and b"table" in last()
    assert lib.pcad_zero_grads(P, None, 3, 5, None) == INV and b"chunk_map" in last()
    assert lib.pcad_zero_grads(P, P, 3, -2, None) == INV
    assert lib.pcad_zero_grads(None, None, 0, 0, None) == 0                # nothing to do


def test_ops_plan_matches_the_map_layout():
    tab, cmap = ops.optim_plan([rec(n=OR.CHUNK + 1, flags=1), rec(n=0), rec(n=2, pdt=BF16, master=P)])
    assert len(tab) == 3 * 64 and cmap == [(0, 0), (0, 1), (2, 0)]
