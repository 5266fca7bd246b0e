"""CPU checks of the fp32 main gradients behind tests/test_gpu_linear_wgrad.py and tests/test_gpu_main_grad.py:
include/pcad_bwd.h, engine.BWD_SIGNATURES and libpcad_bwd.so agree on the three pcad_linear_wgrad* names; the entry refuses every bad
argument before any device work and names it; the slab rule and the scratch size are the header's formula; ops.linear_fn without a
main_grad IS F.linear and with one adds dy^T x to it (the addmm path, against float64 autograd); pretrain has the flag and refuses it
with float32."""
import os
import re
import subprocess

import pytest
import torch
import torch.nn.functional as F

from plantcaduceus_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE
NAMES = {"pcad_linear_wgrad_slabs", "pcad_linear_wgrad_scratch_bytes", "pcad_linear_wgrad"}
# (N, K) of in_proj, out_proj, x_proj, dt_proj at l32 and at PlantCAD2 Small
REAL = [(4096, 1024), (1024, 2048), (96, 2048), (2048, 64), (3072, 768), (768, 1536), (80, 1536), (1536, 48)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def test_header_signatures_and_library_name_the_entries(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcad_bwd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcad_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", engine.BWD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert NAMES <= declared and NAMES <= set(engine.BWD_SIGNATURES) and NAMES <= exported
    assert all(hasattr(lib, n) for n in NAMES)
    text = open(os.path.join(ROOT, "include", "pcad_bwd.h")).read()
    assert "one stated exception" in text and "never accumulated" in text        # the header says that this entry adds


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    got = {k: int(re.search(rf"WGRAD_{k} = (\d+)", src).group(1)) for k in ("BN", "BK", "TARGET_BLOCKS", "MAX_SLABS", "SLAB_ROWS")}
    assert got == {"BN": 128, "BK": 128, "TARGET_BLOCKS": 256, "MAX_SLABS": 32, "SLAB_ROWS": 256}      # the numbers the header states


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor"""
    p = 0x10000
    last = engine.load_library().pcad_last_error

    def call(dy=p, lddy=None, x=p, ldx=None, dw=p, lddw=None, M=300, N=96, K=128, acc=1, scratch=p, nbytes=1 << 40):
        return lib.pcad_linear_wgrad(dy, N if lddy is None else lddy, x, K if ldx is None else ldx, dw, K if lddw is None else lddw, M, N, K, acc,
                                     scratch, nbytes, None)
    for name in ("dy", "x", "dw"):
        assert call(**{name: None}) == INV and name.encode() in last(), name
        assert call(**{name: p + 8}) == INV and name.encode() in last() and b"aligned" in last(), name
    for bad in (0, 4, 12, 100, 8200, -8):
        assert call(N=bad, lddy=8208) == INV and b"N " in last(), bad
        assert call(K=bad, ldx=8208, lddw=8208) == INV and b"K " in last(), bad
    assert call(M=-1) == INV and b"M " in last()
    assert call(lddy=100) == INV and b"lddy" in last()              # not a multiple of 8
    assert call(lddy=88) == INV and b"lddy" in last()               # < N
    assert call(ldx=132) == INV and b"ldx" in last()
    assert call(ldx=120) == INV and b"ldx" in last()
    assert call(lddw=130) == INV and b"lddw" in last()              # not a multiple of 4
    assert call(lddw=124) == INV and b"lddw" in last()              # < K
    # (96, 128) at M = 300 is split in two slabs: scratch is needed
    assert lib.pcad_linear_wgrad_scratch_bytes(300, 96, 128) > 0
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    # nothing to do: M == 0 with accumulate is OK before anything is launched, with no scratch at all
    assert call(M=0, acc=1, scratch=None, nbytes=0) == 0
    rows = engine.C.c_int64(7)
    assert lib.pcad_linear_wgrad_slabs(10, 12, 128, engine.C.byref(rows)) == -1 and b"N " in last() and rows.value == 0
    assert lib.pcad_linear_wgrad_slabs(-1, 16, 128, engine.C.byref(rows)) == -1 and b"M " in last()
    assert lib.pcad_linear_wgrad_scratch_bytes(10, 12, 128) == 0


def formula(M, N, K):
    """include/pcad_bwd.h: -> (slabs, rows_per_slab, scratch bytes)"""
    if M == 0:
        return 0, 0, 0
    tiles = -(-N // 128) * -(-K // 128)
    want = min(32, max(1, 256 // tiles))
    rows = -(-(-(-M // want)) // 256) * 256
    slabs = -(-M // rows)
    return slabs, rows, (-(-(slabs * N * K * 4) // 256) * 256 if slabs > 1 else 0)


def test_slabs_and_scratch_are_the_documented_formula(lib):
    seen = set()
    for N, K in REAL + [(8, 8), (96, 128), (136, 72), (8192, 8192)]:
        for M in (0, 1, 255, 256, 257, 8191, 8192, 8193, 65536, 43 * 8192 * 2, 2 ** 31 // N + 1, 2 ** 33):
            slabs, rows = ops.linear_wgrad_slabs(M, N, K)
            nb = lib.pcad_linear_wgrad_scratch_bytes(M, N, K)
            assert (slabs, rows, nb) == formula(M, N, K), (M, N, K)
            assert nb % 256 == 0 and (M == 0 or (rows % 256 == 0 and (slabs - 1) * rows < M <= slabs * rows and slabs <= 32))
            seen.add(slabs)
    # the fat products are not split at all, the skinny ones are
    assert ops.linear_wgrad_slabs(65536, 4096, 1024) == (1, 65536) and lib.pcad_linear_wgrad_scratch_bytes(65536, 4096, 1024) == 0
    assert ops.linear_wgrad_slabs(65536, 96, 2048) == (16, 4096) and ops.linear_wgrad_slabs(65536, 2048, 64) == (16, 4096)
    assert ops.linear_wgrad_slabs(257, 96, 128) == (2, 256)
    assert {0, 1, 2, 16, 32} <= seen


def test_linear_fn_without_main_grad_is_f_linear():
    g = torch.Generator().manual_seed(0)
    x = torch.randn(3, 5, 16, generator=g, requires_grad=True)
    w = torch.nn.Parameter(torch.randn(24, 16, generator=g))
    y, ref = ops.linear_fn(x, w), F.linear(x, w)
    assert torch.equal(y, ref) and type(y.grad_fn) is type(ref.grad_fn)
    y.sum().backward()
    gx, gw = x.grad.clone(), w.grad.clone()
    x.grad = w.grad = None
    ref.sum().backward()
    assert torch.equal(gx, x.grad) and torch.equal(gw, w.grad)
    # a main_grad changes nothing while autograd does not record, or for a frozen weight
    w.main_grad = torch.zeros(24, 16)
    with torch.no_grad():
        assert ops.linear_fn(x, w).grad_fn is None
    w.requires_grad_(False)
    assert type(ops.linear_fn(x, w).grad_fn) is type(ref.grad_fn) and bool((w.main_grad == 0).all())


@pytest.mark.parametrize("shape", [(36, 128), (128, 4), (40, 128)])
def test_linear_fn_with_main_grad_on_cpu_is_the_addmm_path(shape, caplog):
    """float64 throughout: the main gradient after two backwards is start + twice float64 autograd's weight gradient, dx is autograd's,
    and the weight's .grad stays None.  On the CPU every shape takes the addmm path, the kernel's own (40, 128) included."""
    N, K = shape
    g = torch.Generator().manual_seed(1)
    x = torch.randn(2, 9, K, generator=g, dtype=torch.float64, requires_grad=True)
    w = torch.nn.Parameter(torch.randn(N, K, generator=g, dtype=torch.float64))
    dy = torch.randn(2, 9, N, generator=g, dtype=torch.float64)
    (F.linear(x, w) * dy).sum().backward()
    gx, gw = x.grad.clone(), w.grad.clone()
    x.grad = w.grad = None
    start = torch.randn(N, K, generator=g, dtype=torch.float64)
    w.main_grad = start.clone()
    ops._wgrad_fallback_logged.clear()
    with caplog.at_level("DEBUG", logger="plantcaduceus_amd.ops"):
        for _ in range(2):
            y = ops.linear_fn(x, w)
            assert type(y.grad_fn).__name__ == "_LinearMainGradFnBackward" and torch.equal(y, F.linear(x, w))
            (y * dy).sum().backward()
    assert w.grad is None
    assert (x.grad - 2 * gx).abs().max().item() < 1e-12
    assert (w.main_grad - (start + 2 * gw)).abs().max().item() < 1e-12
    assert sum("linear_fn" in r.getMessage() for r in caplog.records) == 1          # once per shape, at debug level


def test_wgrad_kernel_takes():
    assert all(ops.wgrad_kernel_takes(N, K) for N, K in REAL + [(8, 8), (8192, 8192), (40, 128), (128, 8)])
    assert not any(ops.wgrad_kernel_takes(N, K) for N, K in [(36, 128), (128, 4), (8200, 8), (8, 0), (12, 16)])


def test_pretrain_has_the_flag_and_refuses_it_with_float32(tmp_path):
    from plantcaduceus_amd import pretrain
    base = ["--dataset_name", str(tmp_path), "--output_dir", str(tmp_path / "out")]
    assert pretrain.build_parser().parse_args(base).fp32_grad_accumulation is False
    a = pretrain.build_parser().parse_args(base + ["--fp32_grad_accumulation"])
    assert a.fp32_grad_accumulation is True and a.dtype == "float32"
    with pytest.raises(SystemExit) as e:
        pretrain.train(a)
    assert "--fp32_grad_accumulation" in str(e.value) and "bfloat16" in str(e.value)
    with pytest.raises(SystemExit) as e:
        pretrain.main(base + ["--do_train", "--fp32_grad_accumulation", "--dtype", "float32"])
    assert "--fp32_grad_accumulation" in str(e.value)
