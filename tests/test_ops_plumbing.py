"""The plumbing between the operators of plantcaduceus_amd.ops and the C ABI, on CPU tensors: no GPU, no library.  The guard kit's
checker is what every poisoned GPU test trusts to notice a store outside an output - here it is shown to notice one."""
import pytest
import torch

from plantcaduceus_amd import ops

NAN = float("nan")
GEOMETRIES = ("row", "lines", "optim")
DTYPES = (torch.float32, torch.bfloat16)
SHAPE = (3, 8)


def _guarded(geometry, dtype):
    t, whole = ops._guarded(SHAPE, dtype, "cpu", geometry)
    g = ops._guard_elems(SHAPE, geometry)
    assert t.shape == SHAPE and t.dtype == dtype and whole.numel() == t.numel() + 2 * g and g > 0
    assert t.data_ptr() == whole.data_ptr() + g * whole.element_size()          # the output is the middle of the buffer
    return t, whole, g


def test_guard_geometries():
    assert [ops._guard_elems(SHAPE, g) for g in GEOMETRIES] == [8, 64, ops.OPTIM_GUARD]
    assert ops._guard_elems((3, 65), "lines") == 128 and ops._guard_elems((7,), "row") == 7
    assert ops.WGRAD_GUARD == ops.GUARD == float(torch.tensor(ops.GUARD, dtype=torch.bfloat16))     # one sentinel, exact in bf16


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("geometry", GEOMETRIES)
def test_guarded_output(geometry, dtype):
    t, whole, g = _guarded(geometry, dtype)
    assert bool(torch.isnan(t).all())
    assert bool((whole[:g] == ops.GUARD).all()) and bool((whole[g + t.numel():] == ops.GUARD).all())
    assert ops._guards_intact([(t, whole)]) is True
    t.copy_(torch.arange(t.numel(), dtype=torch.float32).view(SHAPE))           # writing every element of the output itself
    assert ops._guards_intact([(t, whole)]) is True
    assert ops._guards_intact([(t, whole), (torch.empty(SHAPE), None)]) is True  # an unguarded output has nothing to check


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
@pytest.mark.parametrize("geometry", GEOMETRIES)
@pytest.mark.parametrize("where", ("before", "after"))
def test_one_write_outside_is_noticed(where, geometry, dtype):
    t, whole, g = _guarded(geometry, dtype)
    whole[g - 1 if where == "before" else g + t.numel()] = 0.0                   # the sentinel element next to the output
    assert ops._guards_intact([(t, whole)]) is False
    fresh = _guarded(geometry, dtype)
    assert ops._guards_intact([fresh[:2], (t, whole)]) is False                  # one broken buffer among intact ones


def test_unguarded_output_is_plain_empty():
    t, whole = ops._guarded(SHAPE, torch.float32, "cpu", "row", poison=False)
    assert whole is None and t.shape == SHAPE and t.is_contiguous()


def test_two_dimensional_frame():
    """linear_wgrad's frame: the output is a strided view inside a 2-D buffer of sentinels"""
    whole = torch.full((3 + 2, 8 + 8), ops.WGRAD_GUARD)
    run = whole[1:4, 4:12]
    run.fill_(NAN)
    assert ops._guards_intact([(run, whole)]) is True
    for r, c in ((0, 5), (4, 5), (2, 3), (2, 12)):                               # above, below, left, right
        broken = whole.clone()
        broken[r, c] = 1.0
        assert ops._guards_intact([(broken[1:4, 4:12], broken)]) is False


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_guarded_copy_and_copy_back(dtype):
    src = torch.arange(24, dtype=torch.float32).view(2, 3, 4).to(dtype)
    c, whole = ops._guarded_copy(src)
    assert c.shape == src.shape and torch.equal(c, src) and ops._guards_intact([(c, whole)])
    assert whole.numel() == src.numel() + 2 * ops.OPTIM_GUARD
    back = []
    keep, none = ops._guarded_copies([src, None], back)
    blank, = ops._guarded_copies([src], back, blank=True)
    assert none is None and torch.equal(keep, src) and bool(torch.isnan(blank).all()) and len(back) == 2
    a, b = src.clone(), src.clone()
    back = []
    ca, cb = ops._guarded_copies([a, b], back)
    ca.mul_(2)
    cb.fill_(7)
    assert torch.equal(a, src) and torch.equal(b, src)                           # the run touched the copies only
    assert ops._copy_back(back) is True
    assert torch.equal(a, src * 2) and bool((b == 7).all())
    back[1][2][-1] = 0.0                                                         # the last sentinel behind b's copy
    assert ops._copy_back(back) is False


def test_optional_pointer():
    t = torch.zeros(4)
    assert ops._ptr(None) is None and ops._ptr(t) == t.data_ptr() and ops._ptr(t[1:]) == t.data_ptr() + 4


@pytest.mark.parametrize("nb", (0, 1, 257))
@pytest.mark.parametrize("poison", (False, True))
def test_scratch(nb, poison):
    buf, addr = ops._scratch(nb, "cpu", poison)
    assert buf.dtype == torch.uint8 and addr % 256 == 0 and addr >= buf.data_ptr()
    assert buf.data_ptr() + buf.numel() - addr >= nb
    if poison:
        assert bool((buf == 0xFF).all())
        assert bool(torch.isnan(buf[:256].view(torch.float32)).all()) and bool(torch.isnan(buf[:256].view(torch.bfloat16)).all())


def test_padded_dt_rank():
    for R in range(1, 161):
        assert ops.padded_dt_rank(R) == (64 if R <= 64 else (R + 31) // 32 * 32), R
    for R in range(1, 97):
        assert ops.padded_dt_rank(R) == (64 if R <= 64 else 96), R


@pytest.mark.parametrize("dtype", DTYPES, ids=("fp32", "bf16"))
def test_pack_x_proj(dtype):
    R, E = 5, 64
    Rp = ops.padded_dt_rank(R)
    w = torch.randn(R + 32, E, generator=torch.Generator().manual_seed(0))
    p = ops.pack_x_proj(w, R, Rp, E, dtype, "cpu")
    assert p.shape == (Rp + 32, E) and p.dtype == dtype
    assert torch.equal(p[:R], w[:R].to(dtype)) and bool((p[R:Rp] == 0).all()) and torch.equal(p[Rp:], w[R:].to(dtype))


@pytest.mark.parametrize("E,dtype", ((32, torch.float32), (64, torch.bfloat16)), ids=("fp32", "bf16"))
@pytest.mark.parametrize("rows", (1, 8, 13))
def test_blocked_round_trip(rows, E, dtype):
    x = torch.randn(rows, E, generator=torch.Generator().manual_seed(rows)).to(dtype)
    xb = ops.to_blocked(x, pad_value=-3.0)
    rows8 = (rows + 7) // 8 * 8
    assert xb.shape == (rows8 // 8, 1, 8, E) and xb.is_contiguous()              # one 128-byte piece per row at these widths
    assert torch.equal(ops.from_blocked(xb, rows), x)
    got, pad = ops._split_blocked(xb, rows)
    assert torch.equal(got, x) and pad.shape == (rows8 - rows, E) and bool((pad == -3.0).all())
    with pytest.raises(ValueError):
        ops.to_blocked(x[:, :E // 2])                                            # half a line per row
