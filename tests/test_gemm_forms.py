"""CPU checks behind tests/test_gpu_gemm_forms.py: the blocked layout the operator wrappers make is the one csrc/common.hpp states, the
integer operands of tests/gemm_ref.py give products that no summation order can change, each fault a GEMM kernel could have shows in
them, the shapes of the GPU cases run the kernels the GPU file names (tests/launch_forms.py gemm_kernel, the restatement of
csrc/gemm.hip's dispatch), and the entries refuse what the launchers cannot do before a device is needed.

Sensitivity, measured here (share of the outputs of the touched 256 x 128 tile - or of the whole product where it is smaller - that a
modelled fault changes; needed: one half):
    one 64-column K-tile of A taken from the previous output tile, or from another K-tile (K = 64, 192)   99.1 %
    lo . lo added, A read in W's part order, the third part dropped (Ko = 64, 192)                         98.7 .. 99.6 %
    rows rotated inside an 8-row block                                                                    99.1 %
    rscale of row + 1, of row + 16                                                                        98.7 % (every output but the zeros)
    16-column groups exchanged across nsplit = 128, 192, 80                                               99.0 .. 99.1 %"""
import pytest
import torch

import gemm_ref as G
import launch_forms as F
from plantcaduceus_amd import engine, ops

BF, F32 = torch.bfloat16, torch.float32
NT, Q, R = F.GEMM_NT, F.GEMM_256Q, F.GEMM_256R


@pytest.mark.parametrize("dt,rows,cols", [(BF, 37, 192), (F32, 37, 96), (BF, 300, 64), (F32, 13, 160)])
def test_to_blocked_is_blocked_off(dt, rows, cols):
    """rows not a multiple of 8, a piece count that is no power of two (192 bf16 columns: 3 pieces; 160 fp32 columns: 5)"""
    esz = 2 if dt == BF else 4
    pieces = cols * esz // 128
    x = (torch.arange(rows * cols) % 251).view(rows, cols).to(dt)          # < 256: exact in bf16; 251 is prime to every stride here
    flat = ops.to_blocked(x, pad_value=-1.0).reshape(-1)
    rows8 = (rows + 7) // 8 * 8
    assert flat.numel() == rows8 * cols
    r, c = torch.meshgrid(torch.arange(rows8), torch.arange(cols), indexing="ij")
    off = G.blocked_off(r, c * esz, pieces)
    assert off.min() == 0 and off.max() == rows8 * cols * esz - esz and off.unique().numel() == rows8 * cols
    got = flat[(off // esz).reshape(-1)].view(rows8, cols)
    assert torch.equal(got[:rows], x) and (got[rows:] == -1).all()
    assert torch.equal(ops.from_blocked(ops.to_blocked(x), rows), x)


def test_integer_products_do_not_depend_on_the_order():
    """fp32 matmul on the CPU, the same with K permuted and with K cut into partial sums added in reverse: all equal float64 exactly,
    at the largest K the method is used for and in the three-product form"""
    M, N, K = 48, 40, G.INT_MAX_K
    assert 27 * K < 2 ** 24
    a, w = G.ints(1, M, K), G.ints(2, N, K)
    assert a.abs().max() == 3 and a.unique().numel() == 7 and torch.equal(a, a.bfloat16().float())
    ref = G.product(a, w)
    perm = torch.randperm(K, generator=torch.Generator().manual_seed(3))
    assert torch.equal((a @ w.t()).double(), ref)
    assert torch.equal((a[:, perm] @ w[:, perm].t()).double(), ref)
    parts = [a[:, k:k + 64] @ w[:, k:k + 64].t() for k in range(0, K, 64)]
    assert torch.equal(sum(reversed(parts)).double(), ref)
    Ko = 512
    a2, w2 = G.ints(4, M, 2 * Ko), G.ints(5, N, 2 * Ko)
    ref3 = G.split_product(a2, w2, Ko)
    ah, al, wh, wl = a2[:, :Ko], a2[:, Ko:], w2[:, :Ko], w2[:, Ko:]
    assert torch.equal((ah @ wh.t() + al @ wh.t() + ah @ wl.t()).double(), ref3)
    assert torch.equal((ah @ wl.t() + (al @ wh.t() + ah @ wh.t())).double(), ref3)
    assert ref3.abs().max() < 2 ** 24 and torch.equal(G.stored(ref3, F32).double(), ref3)


def _changed(bad, ref, rows=slice(None), cols=slice(None)):
    return (bad[rows, cols] != ref[rows, cols]).double().mean().item()


def _fault_rows():
    out = []
    # a stale K-tile: the ring slot still holds the K-tile of the block's previous output tile (K = 64: one K-tile per output tile), or
    # another K-tile of the same rows
    M, N = 512, 128
    for K in (64, 192):
        a, w = G.ints(10 + K, M, K), G.ints(11 + K, N, K)
        ref = G.product(a, w)
        prev = torch.cat([torch.arange(256, 512), torch.arange(0, 256)])
        for kt in range(K // 64):
            out.append((f"K={K}: K-tile {kt} of the previous output tile", _changed(G.stale_k_tile(a, w, kt, prev), ref, slice(256, 512))))
        if K > 64:
            bad = a.clone()
            bad[:, 64:128] = a[:, 0:64]
            out.append((f"K={K}: K-tile 1 read from K-tile 0", _changed(G.product(bad, w), ref)))
    # the split form's parts
    for Ko in (64, 192):
        a2, w2 = G.ints(20 + Ko, 256, 2 * Ko), G.ints(21 + Ko, 128, 2 * Ko)
        ref = G.split_product(a2, w2, Ko)
        for why, parts in (("lo . lo added", ((0, 0), (1, 0), (0, 1), (1, 1))), ("A in W's part order", ((0, 0), (0, 0), (1, 1))),
                           ("third part dropped", ((0, 0), (1, 0)))):
            out.append((f"Ko={Ko}: {why}", _changed(G.split_product(a2, w2, Ko, parts), ref)))
    # addresses and scales
    a, w = G.ints(30, 300, 64), G.ints(31, 384, 64)
    ref = G.product(a, w)
    for by in (1, 7):
        out.append((f"rows rotated by {by} inside 8-row blocks", _changed(G.rows_rotated(ref, by), ref, slice(0, 296))))
    rs = G.rscale(300 + 16).double()
    for d in (1, 16):
        assert (rs[d:d + 300] != rs[:300]).all()
        out.append((f"rscale of row + {d}", _changed(ref * rs[d:d + 300, None], ref * rs[:300, None])))
    for nsplit in (128, 192, 80):
        ex = G.groups_exchanged(ref, nsplit)
        n = min(nsplit, 384 - nsplit) // 16 * 16
        out.append((f"16-column groups exchanged across nsplit = {nsplit}", min(_changed(ex, ref, cols=slice(0, n)),
                                                                                _changed(ex, ref, cols=slice(nsplit, nsplit + n)))))
    return out


def test_every_modelled_fault_shows():
    """A condition on the inputs, not a measurement: each fault changes at least half of the outputs of the tile it touches"""
    rows = _fault_rows()
    for why, share in rows:
        print(f"fault: {why}: changes {100 * share:.1f} % of the touched outputs")
    assert len(rows) == 18 and all(share >= 0.5 for _, share in rows), [r for r in rows if r[1] < 0.5]


def test_rscale_period_is_coprime_to_the_tile_strides():
    e = torch.log2(G.rscale(7 * 256)).long()
    assert e.min() == -3 and e.max() == 3 and torch.equal(e[:7], torch.arange(-3, 4))
    for stride in (16, 128, 256):
        assert (e[stride:] != e[:-stride]).all()


def test_shapes_give_the_stated_kernels():
    """the (form, shape) -> kernel table of tests/test_gpu_gemm_forms.py, and the tile counts of its hand-over cases on 256 CUs"""
    K = F.gemm_kernel
    for esz in (2, 4):
        kc = 128 // esz
        assert K("xproj", 65829, 96, esz, kc, kc) == NT and F.gemm_tiles(NT, 65829, 96) == 258
        assert K("plain", 300, 384, esz, 2 * kc, 2 * kc) == NT
        assert K("plain", 2100, 528, esz, kc, kc) == R and K("plain", 2048, 512, esz, 3 * kc, 3 * kc) == Q
        assert K("plain", 33280, 512, esz, kc, kc) == Q and F.gemm_tiles(Q, 33280, 512) == 260
        assert K("plain", 33300, 528, esz, kc, kc) == R and F.gemm_tiles(R, 33300, 528) == 393
        assert K("plain", 2040, 512, esz, kc, kc) == NT and K("plain", 2048, 504, esz, kc, kc) == NT          # below either threshold
        for M, N in ((256, 256), (2304, 768), (66048, 512)):
            assert K("residual", M, N, esz, kc, kc) == Q
        assert F.gemm_tiles(Q, 66048, 512) == 516 and K("residual", 300, 256, esz, kc, kc) is None
        for M, N, ns in ((256, 256, 128), (512, 512, 192), (8448, 2048, 1024)):
            assert K("two", M, N, esz, 3 * kc + 64, 3 * kc, nsplit=ns) == Q == K("two", M, N, esz, 3 * kc + 64, 3 * kc, nsplit=ns, epilogue=True)
        assert F.gemm_tiles(Q, 8448, 2048) == 264
        assert K("two", 2100, 384, esz, 2 * kc + 64, 2 * kc, nsplit=192) == R and K("two", 40, 176, esz, 2 * kc + 64, 2 * kc, nsplit=80) == R
        assert K("two", 512, 512, esz, kc, kc, nsplit=80) == R                       # whole tiles, split off the 64-column groups
        assert K("two", 300, 512, esz, kc, kc, nsplit=256, epilogue=True) is None    # rscale needs the 4-wave kernel
    assert K("plain", 2048, 512, 2, 384, 384, osz=4) == Q and K("plain", 300, 384, 2, 128, 128, osz=4) == NT      # ksplit: bf16 -> fp32
    assert K("two", 8448, 2048, 2, 192, 128, osz=4, nsplit=1024) == Q and K("two", 2100, 384, 2, 192, 128, osz=4, nsplit=192) == R
    assert K("two", 512, 512, 2, 128, 128, osz=4, nsplit=192, epilogue=True) is None           # no rscale with fp32 outputs of bf16
    for tiles in (258, 260, 264, 393, 516):
        assert tiles > F.gemm_persistent_grid(256, tiles) == 256
    assert F.gemm_k_tiles(192, 2) == 3 == F.gemm_k_tiles(96, 4)


def test_entries_refuse_before_a_device_is_needed():
    """PCAD_ERR_INVALID for what the launchers cannot do, null and misaligned tensors; the addresses are never dereferenced"""
    lib = engine.load_library()
    p = dict(A=0x10000, W=0x20000, C=0x30000, C2=0x40000, C3=0x50000, rscale=0x60000)
    calls = G.refusals(p)
    assert len(calls) == 6 and {c[1] for c in calls} == {n for n in engine.SIGNATURES if n.startswith("pcad_gemm_nt_") and
                                                         n.split("_")[-1] in ("engine", "xproj", "two")}
    for why, fn, args in calls:
        assert getattr(lib, fn)(*args, None) == -1, (why, fn)
        assert fn in lib.pcad_last_error().decode(), lib.pcad_last_error()
    BFc, F32c = 1, 0
    bad = [
        ("null A", "pcad_gemm_nt_engine", (None, 64, p["W"], 64, p["C"], 256, 256, 256, 64, 0, 0, BFc, BFc)),
        ("null C2", "pcad_gemm_nt_xproj", (p["A"], 64, p["W"], 64, p["C"], 64, None, 32, 64, 256, 96, 64, 0, 0, BFc)),
        ("null ssq", "pcad_gemm_nt_residual_engine", (p["A"], 64, p["W"], 64, p["C"], p["C2"], None, 256, 256, 64, 0, 0, BFc)),
        ("misaligned A", "pcad_gemm_nt_engine", (p["A"] + 8, 64, p["W"], 64, p["C"], 256, 256, 256, 64, 0, 0, BFc, BFc)),
        ("misaligned C1", "pcad_gemm_nt_two", (p["A"], 64, p["W"], 64, p["C"] + 8, p["C2"], 128, None, 256, 256, 64, 0, 0, 0, BFc, BFc)),
        ("misaligned C2", "pcad_gemm_nt_xproj", (p["A"], 64, p["W"], 64, p["C"], 64, p["C2"] + 4, 32, 64, 256, 96, 64, 0, 0, BFc)),
        ("misaligned res", "pcad_gemm_nt_residual_engine", (p["A"], 64, p["W"], 64, p["C"], p["C2"] + 8, p["C3"], 256, 256, 64, 0, 0, BFc)),
        ("bad dtype", "pcad_gemm_nt_engine", (p["A"], 64, p["W"], 64, p["C"], 256, 256, 256, 64, 0, 0, 2, 2)),
        ("bf16 result of fp32 operands", "pcad_gemm_nt_engine", (p["A"], 32, p["W"], 32, p["C"], 256, 256, 256, 32, 0, 0, F32c, BFc)),
        ("K not whole K-tiles", "pcad_gemm_nt_two", (p["A"], 48, p["W"], 48, p["C"], p["C2"], 128, None, 256, 256, 48, 0, 0, 0, BFc, BFc)),
        ("lda shorter than K", "pcad_gemm_nt_engine", (p["A"], 64, p["W"], 128, p["C"], 256, 256, 256, 128, 0, 0, BFc, BFc)),
        ("blocked A with rows of half a piece", "pcad_gemm_nt_engine", (p["A"], 96, p["W"], 64, p["C"], 256, 256, 256, 64, 1, 0, BFc, BFc)),
        ("nsplit off the 16-column groups", "pcad_gemm_nt_xproj", (p["A"], 64, p["W"], 64, p["C"], 72, p["C2"], 24, 72, 256, 96, 64, 0, 0, BFc)),
        ("partial tiles in the residual form", "pcad_gemm_nt_residual_engine", (p["A"], 64, p["W"], 64, p["C"], p["C2"], p["C3"], 300, 256, 64, 0, 0, BFc)),
    ]
    for why, fn, args in bad:
        assert getattr(lib, fn)(*args, None) == -1, (why, fn)
