"""-m gpu: the fused optimizer step at operator level (ops.adamw_step / ops.zero_grads on include/pcad_bwd.h pcad_adamw_step /
pcad_zero_grads) against the float64 restatement of tests/optim_ref.py.

Tensor sizes sit at the chunk and vector edges (optim_ref.EDGE_SIZES, C = ops.OPTIM_CHUNK): as single-tensor tables, together in one
table of mixed dtypes (fp32 / bf16 parameter x fp32 / bf16 gradient) and decay flags, as one table of 300 tensors of 1..50 elements, and
as sub-views 16 bytes into larger buffers.  Five steps with fresh random gradients each, lr 1e-2, weight decay 0.1.

Bars.  master, exp_avg, exp_avg_sq against float64: 4 x the distance torch's own fp32 CPU AdamW(foreach=False) has to float64 on the
same inputs, floored at 2 fp32 ulp of max |p|.  norm against the float64 norm, relative: optim_ref.norm_bar(chunks), from the depth of
the reduction - 1.61e-6 for every table here (at most 300 chunks: one serial addition per lane in the finalising block).
Everything else is bit equality.  Every case prints its figures before it asserts.

Observed on an MI355X, worst over the cases [bar; torch's own distance]: master 9.2e-7 [3.7e-6; 9.2e-7], exp_avg 2.1e-7 [6.3e-7; 1.6e-7],
exp_avg_sq 2.9e-8 [4.8e-7; 3.3e-8] (all three in the mixed and 300-tensor tables), norm 9.1e-8 relative [1.61e-6]; the whole file runs in 6 s."""
import functools

import numpy as np
import pytest
import torch

import optim_ref as OR

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
C = OR.CHUNK
HP = dict(lr=1e-2, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
GUARD = -1024.0
KINDS = {"ff": (F32, F32), "bb": (BF, BF), "fb": (F32, BF), "bf": (BF, F32)}      # parameter dtype, gradient dtype
STEPS = 5


class Set:
    """a parameter set on the device (each tensor optionally a view 16 bytes into a larger buffer of sentinels) and the table over it"""

    def __init__(self, sizes, kinds, seed, sub=False):
        from plantcaduceus_amd import ops
        g = torch.Generator().manual_seed(seed)
        self.sizes, self.kinds, self.sub = list(sizes), list(kinds), sub
        self.decay = [i % 3 != 0 for i in range(len(sizes))]
        self.wholes = []
        self.init, self.param, self.grad, self.master, self.m, self.v = [], [], [], [], [], []
        for n, kind in zip(sizes, kinds):
            pdt, gdt = KINDS[kind]
            p0 = torch.randn(n, generator=g).to(pdt)
            self.init.append(p0.float())                                         # the master starts as the parameter's value
            self.param.append(self._alloc(p0))
            self.grad.append(self._alloc(torch.zeros(n, dtype=gdt)))
            self.master.append(self._alloc(p0.float()) if pdt == BF else None)
            self.m.append(self._alloc(torch.zeros(n)))
            self.v.append(self._alloc(torch.zeros(n)))
        self.table = ops.OptimTable(self.param, self.grad, self.master, self.m, self.v, self.decay)
        self.gen = g

    def _alloc(self, t):
        if not self.sub:
            return t.to(DEV)
        pad = 16 // t.element_size()
        whole = torch.full((t.numel() + 2 * pad,), GUARD, dtype=t.dtype, device=DEV)
        whole[pad:pad + t.numel()] = t.to(DEV)
        self.wholes.append((whole, pad, t.numel()))
        return whole[pad:pad + t.numel()]

    def surroundings_intact(self):
        return all(bool((w[:pad] == GUARD).all()) and bool((w[pad + n:] == GUARD).all()) for w, pad, n in self.wholes)

    def fresh_grads(self, scale=3.0):
        """-> the CPU gradients (in their dtype) now also in the device gradient tensors, whose storage stays"""
        out = []
        for n, kind, gd in zip(self.sizes, self.kinds, self.grad):
            g = (torch.randn(n, generator=self.gen) * scale).to(KINDS[kind][1])
            gd.copy_(g)
            out.append(g)
        return out

    def masters(self):
        return [(ms if ms is not None else p).detach().cpu().clone() for ms, p in zip(self.master, self.param)]

    def snapshot(self):
        return [t.detach().cpu().clone() for col in (self.param, self.m, self.v) for t in col] + self.masters()


def step(s, t, max_norm=0.0, grad_scale=1.0, poison=False):
    from plantcaduceus_amd import ops
    return ops.adamw_step(s.table, HP["lr"], HP["beta1"], HP["beta2"], HP["eps"], HP["weight_decay"], t, max_norm, grad_scale, poison=poison)


def worst(got, ref):
    return max([(a.double() - b.double()).abs().max().item() for a, b in zip(got, ref) if a.numel()] or [0.0])


def trajectory(sizes, kinds, seed, sub=False, max_norm=0.0, grad_scale=1.0, poison=False):
    """STEPS steps on the device, in the float64 restatement and in torch's fp32 CPU AdamW(foreach=False) on the same inputs.
    -> figures: per quantity the worst |device - float64| and |torch fp32 - float64| over all steps and tensors, max |p|, the worst
    relative norm error, whether the bf16 parameters were the rounded masters after every step, guards and surroundings"""
    s = Set(sizes, kinds, seed, sub)
    p64, m64, v64 = [t.double() for t in s.init], [torch.zeros_like(t, dtype=torch.float64) for t in s.init], \
        [torch.zeros_like(t, dtype=torch.float64) for t in s.init]
    tp = [torch.nn.Parameter(t.clone()) for t in s.init]
    opt = OR.torch_adamw(tp, s.decay, foreach=False, **HP)
    fig = dict(dev={"p": 0.0, "m": 0.0, "v": 0.0}, torch={"p": 0.0, "m": 0.0, "v": 0.0}, maxp=0.0, norm_rel=0.0, rounded=True, guards=True,
               chunks=s.table.chunks, states=[])
    for t in range(1, STEPS + 1):
        grads = s.fresh_grads()
        ok = step(s, t, max_norm, grad_scale, poison)
        fig["guards"] = fig["guards"] and (ok is None or ok)
        norm, coef, _ = OR.adamw_step(p64, grads, m64, v64, s.decay, step=t, max_norm=max_norm, grad_scale=grad_scale, **HP)
        for p, g in zip(tp, grads):
            p.grad = g.float() * grad_scale
        if max_norm > 0:
            torch.nn.utils.clip_grad_norm_(tp, max_norm, foreach=False)
        opt.step()
        st = s.table.read_state()
        fig["states"].append((st, norm, coef))
        if norm > 0:
            fig["norm_rel"] = max(fig["norm_rel"], abs(st["norm"] - norm) / norm)
        for q, got, ref, tor in (("p", s.masters(), p64, [p.detach() for p in tp]),
                                 ("m", [x.cpu() for x in s.m], m64, [opt.state[p]["exp_avg"] if p in opt.state else torch.zeros_like(p) for p in tp]),
                                 ("v", [x.cpu() for x in s.v], v64, [opt.state[p]["exp_avg_sq"] if p in opt.state else torch.zeros_like(p) for p in tp])):
            fig["dev"][q] = max(fig["dev"][q], worst(got, ref))
            fig["torch"][q] = max(fig["torch"][q], worst(tor, ref))
        fig["maxp"] = max([fig["maxp"]] + [p.abs().max().item() for p in p64 if p.numel()])
        for p, ms in zip(s.param, s.master):
            if ms is not None:
                fig["rounded"] = fig["rounded"] and torch.equal(p, ms.to(BF))
    fig["surroundings"] = s.surroundings_intact()
    fig["final"] = s.snapshot()
    return fig


@functools.lru_cache(maxsize=None)
def case(name, sub=False, poison=False):
    """every table of the case set, run once and shared by the tests that read it"""
    if name.startswith("single"):
        _, kind, n = name.split("-")
        return trajectory([int(n)], [kind], 100 + int(n) % 97, sub=sub, max_norm=1.0, poison=poison)
    if name == "mixed":
        kinds = [("ff", "bb", "fb", "bf")[i % 4] for i in range(2 * len(OR.EDGE_SIZES))]
        return trajectory(list(OR.EDGE_SIZES) * 2, kinds, 7, sub=sub, max_norm=1.0, grad_scale=0.25, poison=poison)
    if name == "many":
        g = torch.Generator().manual_seed(11)
        sizes = torch.randint(1, 51, (300,), generator=g).tolist()
        return trajectory(sizes, [("ff", "bb")[i % 2] for i in range(300)], 12, sub=sub, max_norm=0.0, poison=poison)
    raise KeyError(name)


def check_accuracy(tag, fig):
    ulp = float(np.spacing(np.float32(fig["maxp"]))) if fig["maxp"] > 0 else 0.0
    line = []
    for q in ("p", "m", "v"):
        bar = max(4 * fig["torch"][q], 2 * ulp)
        line.append(f"{q} {fig['dev'][q]:.3e} [bar {bar:.3e}; torch fp32 {fig['torch'][q]:.3e}]")
    nbar = OR.norm_bar(fig["chunks"])
    print(f"{tag}: " + "; ".join(line) + f"; max |p| {fig['maxp']:.3f} ulp {ulp:.2e}; norm rel {fig['norm_rel']:.2e} [bar {nbar:.2e}]; chunks {fig['chunks']}")
    for q in ("p", "m", "v"):
        assert fig["dev"][q] <= max(4 * fig["torch"][q], 2 * ulp), (tag, q)
    assert fig["norm_rel"] <= nbar, tag
    assert fig["rounded"], tag                 # a bf16 param is master.to(bfloat16) bit for bit after every step
    for st, norm, coef in fig["states"]:
        assert st["finite"] == 1 and st["skipped"] == 0
        if np.isfinite(coef):
            assert abs(st["coef"] - coef) <= 4 * 2.0 ** -24 * abs(coef) + nbar * abs(coef), (tag, st, coef)


@pytest.mark.parametrize("n", OR.EDGE_SIZES)
@pytest.mark.parametrize("kind", ["ff", "bb"])
def test_single_tensor_tables(kind, n):
    check_accuracy(f"single {kind} n={n}", case(f"single-{kind}-{n}"))


def test_mixed_table():
    """all edge sizes twice, the four dtype pairs and both decay flags in one table; grad_scale 1/4 with clipping at 1"""
    check_accuracy("mixed", case("mixed"))


def test_table_of_300_small_tensors():
    fig = case("many")
    assert fig["chunks"] == 300
    check_accuracy("300 tensors", fig)
    for st, norm, coef in fig["states"]:
        assert st["coef"] == 1.0               # max_norm <= 0: coef == grad_scale exactly


@pytest.mark.parametrize("n", OR.EDGE_SIZES[:-1])
@pytest.mark.parametrize("kind", ["ff", "bb"])
def test_sub_views_16_bytes_into_a_larger_buffer(kind, n):
    """the same results as the plain allocation, bit for bit, and the bytes around every tensor untouched"""
    fig = case(f"single-{kind}-{n}", sub=True)
    check_accuracy(f"sub-view {kind} n={n}", fig)
    assert fig["surroundings"]
    plain = case(f"single-{kind}-{n}")
    assert all(torch.equal(a, b) for a, b in zip(fig["final"], plain["final"]))


def test_clipping_is_the_unclipped_update_of_the_rescaled_gradients():
    """max_norm below the norm: the same bits as max_norm <= 0 on gradients multiplied by the reported coef (the kernel's own first
    operation, g = coef * grad in fp32).  max_norm <= 0: coef == grad_scale exactly, also for a grad_scale that is no power of two"""
    sizes, kinds = [C + 1, 9, 3 * C + 5, 7], ["ff", "ff", "ff", "ff"]
    a, b = Set(sizes, kinds, 21), Set(sizes, kinds, 21)
    for t in range(1, 4):
        grads = a.fresh_grads()
        norm = OR.grad_norm(grads)
        step(a, t, max_norm=norm / 3)
        st = a.table.read_state()
        want = (norm / 3) / (norm + 1e-6)
        print(f"step {t}: norm {st['norm']:.6f} float64 {norm:.6f}; coef {st['coef']:.8f} float64 {want:.8f}")
        assert st["coef"] < 0.34 and abs(st["coef"] - want) <= (OR.norm_bar(a.table.chunks) + 4 * 2.0 ** -24) * want
        for gd, g in zip(b.grad, grads):
            gd.copy_(g.to(DEV) * st["coef"])
        step(b, t, max_norm=0.0)
        assert b.table.read_state()["coef"] == 1.0
        assert all(torch.equal(x, y) for x, y in zip(a.snapshot(), b.snapshot())), t
    a.fresh_grads()
    step(a, 4, max_norm=-1.0, grad_scale=1.0 / 3.0)
    assert a.table.read_state()["coef"] == float(np.float32(1.0 / 3.0))


def test_non_finite_gradients_skip_the_step():
    """one inf in one gradient of the 300-tensor table: every master, m, v and param bit-unchanged, finite 0, skipped 0 -> 1; the next
    clean step applies"""
    g = torch.Generator().manual_seed(11)
    sizes = torch.randint(1, 51, (300,), generator=g).tolist()
    s = Set(sizes, [("ff", "bb")[i % 2] for i in range(300)], 31)
    s.fresh_grads()
    step(s, 1, max_norm=1.0)
    st = s.table.read_state()
    assert st["finite"] == 1 and st["skipped"] == 0
    before = s.snapshot()
    s.fresh_grads()
    s.grad[137][sizes[137] // 2] = float("inf")
    step(s, 2, max_norm=1.0)
    st = s.table.read_state()
    print(f"inf step: {st}")
    assert st["finite"] == 0 and st["skipped"] == 1
    assert all(torch.equal(x, y) for x, y in zip(before, s.snapshot()))
    s.fresh_grads()
    s.grad[5][0] = float("nan")
    step(s, 3, max_norm=1.0)
    st = s.table.read_state()
    assert st["finite"] == 0 and st["skipped"] == 2
    assert all(torch.equal(x, y) for x, y in zip(before, s.snapshot()))
    s.fresh_grads()
    step(s, 4, max_norm=1.0)
    st = s.table.read_state()
    after = s.snapshot()
    assert st["finite"] == 1 and st["skipped"] == 2
    assert all(not torch.equal(x, y) for x, y in zip(before[300:], after[300:]))          # every m, v and master of the set moved


@pytest.mark.parametrize("name", ["mixed", "many"])
def test_reproducible_and_memory_safe(name):
    """two runs from equal states give equal bits; under poison - every output between sentinels, the scratch NaN-filled - the sentinels
    are intact and no result changes"""
    first = case(name)
    again = _rerun(name)
    assert all(torch.equal(a, b) for a, b in zip(first["final"], again["final"]))
    assert [s[0] for s in first["states"]] == [s[0] for s in again["states"]]
    poisoned = _rerun(name, poison=True)
    assert poisoned["guards"]
    assert all(torch.equal(a, b) for a, b in zip(first["final"], poisoned["final"]))
    assert [s[0] for s in first["states"]] == [s[0] for s in poisoned["states"]]


def _rerun(name, poison=False):
    return case.__wrapped__(name, False, poison)


@pytest.mark.parametrize("sub", [False, True])
def test_zero_grads(sub):
    from plantcaduceus_amd import ops
    sizes = list(OR.EDGE_SIZES[:-1] if sub else OR.EDGE_SIZES) * 2
    kinds = [("ff", "bb", "fb", "bf")[i % 4] for i in range(len(sizes))]
    s = Set(sizes, kinds, 41, sub=sub)
    s.fresh_grads()
    before = [t.detach().cpu().clone() for col in (s.param, s.m, s.v) for t in col]
    ops.zero_grads(s.table)
    assert all(not bool(g.any()) for g in s.grad)
    assert all(torch.equal(g.view(torch.int16 if g.dtype == BF else torch.int32), torch.zeros_like(g).view(torch.int16 if g.dtype == BF else torch.int32))
               for g in s.grad)                                                   # +0, not -0
    assert s.surroundings_intact()
    assert all(torch.equal(x, y) for x, y in zip(before, [t.detach().cpu() for col in (s.param, s.m, s.v) for t in col]))
    s.fresh_grads()
    assert ops.zero_grads(s.table, poison=True) is True
    assert all(not bool(g.any()) for g in s.grad) and s.surroundings_intact()
