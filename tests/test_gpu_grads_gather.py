"""-m gpu: every gradient of a parameter set into one fp32 buffer in one launch (ops.grads_gather on include/pcad_bwd.h pcad_grads_gather;
DESIGN.md §4r), and optim.AdamW's step through that buffer (`reducer=`), at a world of one in-process.

Operator.  tests/test_gpu_optim.py's shapes, each with fp32 and with bf16 gradients: n = 0, 1, 7, 8, 9, C - 1, C, C + 1, 3 C + 5
(C = ops.OPTIM_CHUNK) as single-tensor tables, together in one table that mixes both gradient dtypes, 300 tensors of 1 .. 50 elements, and
the mixed table as sub-views 16 bytes into larger buffers.  The operation is exact (bf16 -> fp32 loses nothing), so every assertion is bit
equality: `flat` is the padded concatenation of g.float(); the padding is still +0; run into a buffer of sentinels instead, the padding
and the tail are still sentinels (never written); the gradients are untouched; the poison form's sentinels around `flat` are intact;
a second call gives the same bits.

Optimizer.  AdamW(reducer=GradReducer(None, ...)) against plain AdamW on copies, 5 steps with fresh gradients, clipping on.  fp32
parameters and gradients: the two paths run the same kernels on the same (dtype pair, chunk map), hence the same summation order -
master, m, v, norm and coef are bit-equal.  bf16: the norm's vector width follows the gradient dtype (csrc/optim.hip sumsq_chunk), which
is bf16 on one path and fp32 on the other, so the paths are NOT compared with each other: the flat path's norm is held to the float64
norm at optim_ref.norm_bar (1.61e-6 relative) and param == master.to(bfloat16) bit for bit.  One inf in one gradient:
nothing changes and `skipped` goes 0 -> 1."""
import functools

import pytest
import torch

import optim_ref as OR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
C = OR.CHUNK
SENTINEL = -1024.0
SINGLE = [f"single-{k}-{n}" for k in ("f", "b") for n in OR.EDGE_SIZES]
CASES = SINGLE + ["mixed", "many-f", "many-b", "sub"]


def tables(name):
    """-> (sizes, gradient dtypes, sub) of the named case"""
    if name.startswith("single"):
        _, k, n = name.split("-")
        return [int(n)], [F32 if k == "f" else BF], False
    if name in ("mixed", "sub"):
        sizes = list(OR.EDGE_SIZES) * 2
        return sizes, [(F32, BF)[(i + i // len(OR.EDGE_SIZES)) % 2] for i in range(len(sizes))], name == "sub"
    return [1 + i % 50 for i in range(300)], [F32 if name == "many-f" else BF] * 300, False


def alloc(t, sub, wholes):
    if not sub:
        return t.to(DEV)
    pad = 16 // t.element_size()
    whole = torch.full((t.numel() + 2 * pad,), SENTINEL, dtype=t.dtype, device=DEV)
    whole[pad:pad + t.numel()] = t.to(DEV)
    wholes.append((whole, pad, t.numel()))
    return whole[pad:pad + t.numel()]


@functools.lru_cache(maxsize=None)
def case(name):
    """the named table gathered three times (poison form into zeros, plain form into zeros, plain form into sentinels), once for all tests"""
    from plantcaduceus_amd import ops
    sizes, gdts, sub = tables(name)
    g = torch.Generator().manual_seed(len(name) + sum(sizes) % 97)
    wholes, grads, cpu = [], [], []
    for n, dt in zip(sizes, gdts):
        c = (torch.randn(n, generator=g) * 3).to(dt)
        if n > 2:
            c[1], c[n - 1] = -0.0, float("inf")                                  # bit patterns a copy must keep
        cpu.append(c)
        grads.append(alloc(c, sub, wholes))
    f = lambda n: alloc(torch.zeros(n), sub, wholes)
    table = ops.OptimTable([f(n) for n in sizes], grads, [None] * len(sizes), [f(n) for n in sizes], [f(n) for n in sizes], [True] * len(sizes))
    offsets, total = table.flat_plan()
    dev_off = table.flat_offsets()
    flats = [torch.zeros(total + 4, device=DEV), torch.zeros(total + 4, device=DEV), torch.full((total + 4,), SENTINEL, device=DEV)]
    intact = ops.grads_gather(table, flats[0], dev_off, poison=True)
    assert ops.grads_gather(table, flats[1], dev_off) is None
    ops.grads_gather(table, flats[2], dev_off)
    torch.cuda.synchronize()
    expect = torch.zeros(total + 4)
    pad = torch.ones(total + 4, dtype=torch.bool)
    for o, c in zip(offsets, cpu):
        expect[o:o + c.numel()] = c.float()
        pad[o:o + c.numel()] = False
    return dict(sizes=sizes, offsets=offsets, total=total, chunks=table.chunks, flats=[x.cpu() for x in flats], expect=expect, pad=pad, intact=intact,
                sources=all(torch.equal(d.cpu(), c) for d, c in zip(grads, cpu)),
                surroundings=all(bool((w[:p] == SENTINEL).all()) and bool((w[p + n:] == SENTINEL).all()) for w, p, n in wholes))


def bits(t):
    return t.view(torch.int32)


@pytest.mark.parametrize("name", CASES)
def test_flat_is_the_padded_concatenation(name):
    c = case(name)
    up = [(n + 3) // 4 * 4 for n in c["sizes"]]
    assert c["offsets"] == [sum(up[:i]) for i in range(len(up))] and c["total"] == sum(up) and c["chunks"] == OR.chunk_count(c["sizes"])
    print(f"{name}: {len(c['sizes'])} tensors, {c['total']} elements, {c['chunks']} chunks, {int(c['pad'].sum()) - 4} padding elements")
    assert torch.equal(bits(c["flats"][0]), bits(c["expect"]))                   # every bit, -0 and inf included
    assert bool((bits(c["flats"][0])[c["pad"]] == 0).all())                      # the padding and the tail are still +0


@pytest.mark.parametrize("name", CASES)
def test_padding_and_tail_are_never_written_and_sources_stay(name):
    c = case(name)
    into_sentinels = c["flats"][2]
    assert bool((into_sentinels[c["pad"]] == SENTINEL).all())
    assert torch.equal(bits(into_sentinels[~c["pad"]]), bits(c["expect"][~c["pad"]]))
    assert c["sources"] and c["surroundings"]


@pytest.mark.parametrize("name", CASES)
def test_poison_sentinels_intact_and_two_calls_equal(name):
    c = case(name)
    assert c["intact"] is True
    assert torch.equal(bits(c["flats"][0]), bits(c["flats"][1]))


def test_wrapper_refuses_a_short_buffer_and_foreign_offsets():
    from plantcaduceus_amd import ops
    z = lambda n: torch.zeros(n, device=DEV)
    table = ops.OptimTable([z(10), z(5)], [torch.ones(10, device=DEV), torch.ones(5, device=DEV)], [None, None], [z(10), z(5)], [z(10), z(5)], [True, True])
    assert table.flat_plan() == ([0, 12], 20)
    with pytest.raises(ValueError, match="at least 20"):
        ops.grads_gather(table, z(19), table.flat_offsets())
    with pytest.raises(ValueError, match="offsets"):
        ops.grads_gather(table, z(24), table.flat_offsets().to(torch.int32))
    # offsets that are not this buffer's (a slice that would end past flat_elems, a slice that is not 4-aligned): the chunk is not written
    flat = torch.full((20,), SENTINEL, device=DEV)
    ops.grads_gather(table, flat, torch.tensor([0, 16], dtype=torch.int64, device=DEV))
    assert bool((flat[:10] == 1).all()) and bool((flat[10:] == SENTINEL).all())
    flat.fill_(SENTINEL)
    ops.grads_gather(table, flat, torch.tensor([2, 12], dtype=torch.int64, device=DEV))
    assert bool((flat[:12] == SENTINEL).all()) and bool((flat[12:17] == 1).all()) and bool((flat[17:] == SENTINEL).all())


# ---- the optimizer through the buffer, a world of one ---------------------------------------------------------------------------
SIZES = (1, 7, 8, 9, C - 1, C, C + 1, 3 * C + 5, 0, 300)
STEPS = 5


def optimizers(dtype, seed=3):
    from plantcaduceus_amd import ddp, optim
    g = torch.Generator().manual_seed(seed)
    init = [torch.randn(n, generator=g).to(dtype) for n in SIZES]
    named = lambda: [(f"t{i}.weight" if i % 3 else f"t{i}.bias", torch.nn.Parameter(t.clone().to(DEV))) for i, t in enumerate(init)]
    kw = dict(lr=1e-2, weight_decay=0.1, max_grad_norm=1.0, grad_scale=0.5)
    return optim.AdamW(named(), **kw), optim.AdamW(named(), reducer=ddp.GradReducer(None, DEV), **kw), g


def set_grads(opts, gen, dtype, scale=3.0):
    grads = [(torch.randn(n, generator=gen) * scale).to(dtype) for n in SIZES]
    for opt in opts:
        for p, gr in zip(opt.params, grads):
            if p.grad is None:
                p.grad = gr.clone().to(DEV)
            else:
                p.grad.copy_(gr)
    return grads


def test_fp32_flat_path_is_bit_equal_to_the_plain_step():
    plain, flat, gen = optimizers(F32)
    assert plain.reducer is None and plain._flat_table is None and flat.reducer.total == sum((n + 3) // 4 * 4 for n in SIZES)
    for t in range(STEPS):
        set_grads((plain, flat), gen, F32)
        plain.step()
        flat.step()
        plain.zero_grad()
        flat.zero_grad()
        a, b = plain.state(), flat.state()
        print(f"step {t + 1}: norm {a['norm']:.7f} / {b['norm']:.7f} coef {a['coef']:.8f} / {b['coef']:.8f}")
        assert a == b and a["finite"] == 1 and a["norm"] > 1.0                   # clipping is active
        for x, y in zip(plain.params + plain.exp_avg + plain.exp_avg_sq, flat.params + flat.exp_avg + flat.exp_avg_sq):
            assert torch.equal(x, y)
        assert all(not bool(p.grad.any()) for p in flat.params)                  # zero_grad still runs on the parameters' own gradients
    assert plain.state_dict()["step"] == flat.state_dict()["step"] == STEPS
    assert bool((flat.reducer.flat[flat.reducer.total:] == 0).all())


def test_bf16_flat_path_norm_and_rounded_masters():
    _, flat, gen = optimizers(BF)
    bar = OR.norm_bar(flat.table().chunks)
    assert abs(bar - 1.61e-6) < 1e-8
    for t in range(STEPS):
        grads = set_grads((flat,), gen, BF)
        flat.step()
        st = flat.state()
        norm64 = OR.grad_norm(grads, 0.5)
        rel = abs(st["norm"] - norm64) / norm64
        print(f"step {t + 1}: norm {st['norm']:.7f} float64 {norm64:.7f} relative {rel:.2e} [bar {bar:.2e}]")
        assert rel <= bar and st["finite"] == 1
        for o, gr in zip(flat.table().flat_plan()[0], grads):
            assert torch.equal(flat.reducer.grads[o:o + gr.numel()].cpu(), gr.float())          # the step saw the gradients' exact values
        for p, m in zip(flat.params, flat.master):
            assert p.dtype == BF and m.dtype == F32 and torch.equal(p, m.to(BF))
        flat.zero_grad()
    assert any(bool(m.any()) for m in flat.exp_avg)


@pytest.mark.parametrize("dtype", [F32, BF])
def test_one_inf_skips_the_step(dtype):
    _, flat, gen = optimizers(dtype)
    set_grads((flat,), gen, dtype)
    flat.step()
    flat.zero_grad()
    assert flat.state()["skipped"] == 0
    before = [t.clone() for t in flat.params + flat.exp_avg + flat.exp_avg_sq + [m for m in flat.master if m is not None]]
    set_grads((flat,), gen, dtype)
    flat.params[4].grad[C - 2] = float("inf")
    flat.step()
    st = flat.state()
    after = flat.params + flat.exp_avg + flat.exp_avg_sq + [m for m in flat.master if m is not None]
    assert st["finite"] == 0 and st["skipped"] == 1 and all(torch.equal(x, y) for x, y in zip(before, after))
