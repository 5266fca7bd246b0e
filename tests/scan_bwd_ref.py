"""The reference of the selective scan's backward (test helper; no tests here): a torch restatement of include/pcad_train.h
pcad_selective_scan_bwd's forward formulas, differentiated by torch.autograd on the CPU.

    d_t = softplus(delta_t + bias)  (v > 20: v);  h = exp(d_t A) h + d_t u_t B_t;  y_t = <h, C_t> + D u_t;  out = y silu(z)  (z None: y)

Upstream layout: u, delta, z (B, E, L); A (E, 16); B, C (B, 16, L); D, bias (E).  `reverse` walks right to left (by flipping).  The
restatement runs in the dtype it is asked for: float64 is the reference, float32 through the identical code measures what fp32
arithmetic alone costs (the bars below).  A, D and bias may carry a leading batch dimension (the finite-difference check perturbs
one coordinate per batch copy)."""
import torch

import scan_ref as R

NAMES = ("u", "delta", "A", "B", "C", "D", "z", "delta_bias")


def inputs(seed, Bsz, E, L, bf=False):
    """tests/test_gpu_ops.py _scan_inputs, plus a seeded dout; bf: every tensor a bf16 call stores in bf16 is rounded first (fp32
    tensors holding bf16 values), so that the reference sees the kernel's operands"""
    g = torch.Generator().manual_seed(seed)
    N = R.N
    u = torch.randn(Bsz, E, L, generator=g)
    delta = torch.randn(Bsz, E, L, generator=g) * 0.5 - 3.0
    A = -torch.exp(torch.log(torch.arange(1, N + 1).float())[None, :] + 0.3 * torch.randn(E, N, generator=g))
    Bm = torch.randn(Bsz, N, L, generator=g)
    Cm = torch.randn(Bsz, N, L, generator=g)
    D = torch.rand(E, generator=g) + 0.5
    z = torch.randn(Bsz, E, L, generator=g)
    db = torch.randn(E, generator=g)
    dout = torch.randn(Bsz, E, L, generator=g)
    r = R.bf16 if bf else R.ident
    return dict(u=r(u), delta=r(delta), A=A, B=r(Bm), C=r(Cm), D=D, z=r(z), delta_bias=db, dout=r(dout))


def forward(x, reverse=False, dtype=torch.float64, keep=None):
    """x: dict of NAMES (D / z / delta_bias may be None) -> out (B, E, L) in `dtype`.  keep: a dict that receives the time step
    d = softplus(delta + bias) (B, E, L) as a graph node (its gradient is the formulas' dd_t)."""
    f = (lambda t: t.flip(-1)) if reverse else R.ident
    c = lambda t: None if t is None else t.to(dtype)
    u, delta, Bm, Cm, z = (None if x[k] is None else f(c(x[k])) for k in ("u", "delta", "B", "C", "z"))
    A, D, bias = c(x["A"]), c(x["D"]), c(x["delta_bias"])
    Bsz, E, L = u.shape
    pre = delta if bias is None else delta + bias[..., None]
    d = torch.where(pre > 20, pre, torch.log1p(torch.exp(torch.clamp(pre, max=20.0))))
    if keep is not None:
        d.retain_grad()
        keep["d"] = d
    h = torch.zeros(Bsz, E, R.N, dtype=dtype)
    ys = []
    for t in range(L):
        dl = d[:, :, t]
        h = torch.exp(dl[..., None] * A) * h + (dl * u[:, :, t])[..., None] * Bm[:, None, :, t]
        y = (h * Cm[:, None, :, t]).sum(-1)
        ys.append(y if D is None else y + D * u[:, :, t])
    y = torch.stack(ys, dim=-1)
    if z is not None:
        y = y * (z * torch.sigmoid(z))
    return f(y)


def grads(x, reverse=False, dtype=torch.float64):
    """-> dict name -> gradient of sum(out * dout) (None for an input that is None), plus "dd": the gradient of the time step,
    walk order undone (B, E, L)"""
    leaves = {k: (None if x[k] is None else x[k].detach().to(dtype).requires_grad_(True)) for k in NAMES}
    keep = {}
    out = forward(leaves, reverse, dtype, keep)
    (out * x["dout"].to(dtype)).sum().backward()
    g = {k: (None if leaves[k] is None else leaves[k].grad.detach()) for k in NAMES}
    g["dd"] = keep["d"].grad.flip(-1) if reverse else keep["d"].grad
    return g


def metric(got, ref):
    """max |got - ref| / max |ref| over every element.  A reference that is zero throughout (dA at L = 1: h_{-1} = 0) has no scale:
    there the gradient must be zero exactly, and the metric is 0 or inf."""
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    top = ref.abs().max().item()
    if top == 0.0:
        return 0.0 if bool((got == 0).all()) else float("inf")
    return (got - ref).abs().max().item() / top


def reference(key, make, reverse):
    """(float64 gradients, fp32-autograd deviation per gradient) of the inputs `make()` builds; cached per `key`, computed once"""
    def run():
        x = make()
        g64, g32 = grads(x, reverse, torch.float64), grads(x, reverse, torch.float32)
        return x, g64, {k: metric(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return R.cached(("scan_bwd", key, reverse), run)


def bar(name, dev32, stored_bf16):
    """the bar of one gradient tensor: max(BAR_SCAN of the dtype the tensor is stored in, 8 x what fp32 CPU autograd through the same
    restatement deviates from float64)"""
    return max(R.BAR_SCAN[bool(stored_bf16)], R.ORACLE_FACTOR * dev32[name])
