"""The references of the conv and RMSNorm backward operators and of the graphs composed from them (test helper; no tests here): torch
restatements of include/pcad_bwd.h's forward formulas, differentiated by torch.autograd on the CPU.

    conv   a_t = b + sum_k w[k] x[t-3+k]  (reverse: x[t+3-k]),  rows outside [0, L) zero;  out = a sig(a)        x [S, L, E] token-major
    norm   r = x + residual  (residual None: x);  y = r rsqrt(mean(r^2) + eps) w;  the prenorm output is r       x [..., D]

The restatements run in the dtype they are asked for: float64 is the reference, float32 through the identical code measures what fp32
arithmetic alone costs (the bars: scan_bwd_ref.bar).  `mamba_inner` and `block` are graphs over an operator set K, so that the same
lines run on the restatements here and on plantcaduceus_amd.ops on the GPU."""
import math

import torch
import torch.nn.functional as F

import scan_bwd_ref as SB
import scan_ref as R


# ---- the two operators --------------------------------------------------------------------------------------------------------------
def conv_forward(x, w, b, reverse=False, dtype=torch.float64):
    """x [S, L, E], w [E, 4], b [E] -> [S, L, E] in `dtype`; reverse: the anti-causal conv (the causal one on the flipped rows, flipped back)"""
    f = (lambda t: t.flip(1)) if reverse else R.ident
    x, w, b = f(x.to(dtype)), w.to(dtype), b.to(dtype)
    S, L, E = x.shape
    xp = torch.cat([torch.zeros(S, 3, E, dtype=dtype), x], dim=1)           # row t of x is row t + 3 of xp
    a = b.expand(S, L, E)
    for k in range(4):
        a = a + w[:, k] * xp[:, k:k + L]
    return f(a * torch.sigmoid(a))


def norm_forward(x, residual, weight, eps, dtype=torch.float64):
    """-> (y, r): the normalised rows and the prenorm output, both in `dtype`, nothing rounded"""
    r = x.to(dtype) if residual is None else x.to(dtype) + residual.to(dtype)
    y = r * torch.rsqrt(r.pow(2).mean(-1, keepdim=True) + eps) * weight.to(dtype)
    return y, r


def _leaf(t, dtype):
    return None if t is None else t.detach().clone().to(dtype).requires_grad_(True)


def conv_grads(c, reverse=False, dtype=torch.float64):
    """c: dict(x, w, b, dout) -> dict(x, w, b): gradients of sum(out * dout)"""
    lv = {k: _leaf(c[k], dtype) for k in ("x", "w", "b")}
    (conv_forward(lv["x"], lv["w"], lv["b"], reverse, dtype) * c["dout"].to(dtype)).sum().backward()
    return {k: v.grad for k, v in lv.items()}


def norm_grads(c, dtype=torch.float64):
    """c: dict(x, residual or None, weight, dy, dres_out or None, eps) -> dict(x, residual (None without one), weight): gradients of
    sum(y * dy) + sum(r * dres_out)"""
    lv = {k: _leaf(c[k], dtype) for k in ("x", "residual", "weight")}
    y, r = norm_forward(lv["x"], lv["residual"], lv["weight"], c["eps"], dtype)
    loss = (y * c["dy"].to(dtype)).sum()
    if c["dres_out"] is not None:
        loss = loss + (r * c["dres_out"].to(dtype)).sum()
    loss.backward()
    return {k: (None if v is None else v.grad) for k, v in lv.items()}


def conv_inputs(seed, S, L, E, bf=False):
    """bf: what a bf16 call stores in bf16 (x, dout) is rounded first, so that the reference sees the kernel's operands; taps and bias are fp32"""
    g = torch.Generator().manual_seed(seed)
    r = R.bf16 if bf else R.ident
    return dict(x=r(torch.randn(S, L, E, generator=g)), w=(torch.rand(E, 4, generator=g) * 2 - 1) * 0.5,
                b=(torch.rand(E, generator=g) * 2 - 1) * 0.5, dout=r(torch.randn(S, L, E, generator=g)))


def norm_inputs(seed, rows, D, residual=True, prenorm=True, bf=False, res_bf=False, eps=1e-5):
    """res_bf: the residual stream is stored in bf16 too (residual_in_fp32=False on a bf16 model)"""
    g = torch.Generator().manual_seed(seed)
    r, rr = (R.bf16 if bf else R.ident), (R.bf16 if res_bf else R.ident)
    return dict(x=r(torch.randn(rows, D, generator=g)), residual=rr(torch.randn(rows, D, generator=g) * 2.0) if residual else None,
                weight=torch.rand(D, generator=g) + 0.5, dy=r(torch.randn(rows, D, generator=g)),
                dres_out=rr(torch.randn(rows, D, generator=g)) if prenorm else None, eps=eps)


def reference(key, make, grads):
    """(inputs, float64 gradients, fp32-autograd deviation per gradient) of the inputs `make()` builds; cached per `key`, computed once"""
    def run():
        c = make()
        g64, g32 = grads(c, torch.float64), grads(c, torch.float32)
        return c, g64, {k: SB.metric(g32[k], g64[k]) for k in g64 if g64[k] is not None}
    return R.cached(("block_bwd", key), run)


# ---- composed graphs ----------------------------------------------------------------------------------------------------------------
MAMBA_PARAMS = ("conv_w", "conv_b", "x_proj", "dt_proj", "out_proj", "A", "D", "delta_bias")


def mamba_params(seed, Dm, E, Rk):
    """One Mamba's parameters with the init ranges of plantcaduceus_amd.checkpoint.synthetic_state_dict (tests/test_gpu_ops.py
    _mamba_params), as a dict of fp32 tensors: A = -exp(A_log) and delta_bias = dt_proj's bias as mamba_inner_fn takes them"""
    g = torch.Generator().manual_seed(seed)

    def U(shape, bound):
        return (torch.rand(shape, generator=g) * 2 - 1) * bound
    dt = torch.exp(torch.rand(E, generator=g) * (math.log(0.1) - math.log(1e-3)) + math.log(1e-3)).clamp_min(1e-4)
    A_log = torch.log(torch.arange(1, 17, dtype=torch.float32).repeat(E, 1)) + 0.3 * torch.randn(E, 16, generator=g)
    return dict(in_proj=U((2 * E, Dm), Dm ** -0.5), conv_w=U((E, 4), 0.5), conv_b=U((E,), 0.5), x_proj=U((Rk + 32, E), E ** -0.5),
                dt_proj=U((E, Rk), Rk ** -0.5), delta_bias=dt + torch.log(-torch.expm1(-dt)), A=-torch.exp(A_log), A_log=A_log,
                D=torch.rand(E, generator=g) + 0.5, out_proj=U((Dm, E), E ** -0.5), norm_w=torch.rand(Dm, generator=g) + 0.5)


class CpuOps:
    """the operator set of the restatements, in one dtype"""

    def __init__(self, dtype):
        self.dtype = dtype

    def mamba_inner(self, xz, p, reverse):
        """include/pcad_bwd.h's conv, F.linear, scan_bwd_ref.forward, F.linear: mamba_inner_fn's chain, nothing rounded.  xz (B, 2E, L)"""
        E, Rk = p["conv_w"].shape[0], p["dt_proj"].shape[1]
        xc = conv_forward(xz[:, :E].transpose(1, 2), p["conv_w"], p["conv_b"], reverse, self.dtype)            # (B, L, E)
        x_dbl = F.linear(xc, p["x_proj"])
        delta = F.linear(x_dbl[..., :Rk], p["dt_proj"]).transpose(1, 2)
        y = SB.forward(dict(u=xc.transpose(1, 2), delta=delta, A=p["A"], B=x_dbl[..., Rk:Rk + 16].transpose(1, 2),
                            C=x_dbl[..., Rk + 16:].transpose(1, 2), D=p["D"], z=xz[:, E:], delta_bias=p["delta_bias"]), reverse, self.dtype)
        return F.linear(y.transpose(1, 2), p["out_proj"])

    def rms_norm_prenorm(self, x, weight, residual, eps):
        return norm_forward(x, residual, weight, eps, self.dtype)


class GpuOps:
    """the same operator set on plantcaduceus_amd.ops"""

    def __init__(self, ops):
        self.ops = ops

    def mamba_inner(self, xz, p, reverse):
        return self.ops.mamba_inner_fn(xz, p["conv_w"].unsqueeze(1), p["conv_b"], p["x_proj"], p["dt_proj"], p["out_proj"], None, p["A"], None,
                                       None, D=p["D"], delta_bias=p["delta_bias"], delta_softplus=True, reverse=reverse)

    def rms_norm_prenorm(self, x, weight, residual, eps):
        return self.ops.rms_norm_fn(x, weight, None, residual, eps, prenorm=True, residual_in_fp32=True)


def block(K, p, hidden, residual, eps=1e-5):
    """One Caduceus block as the reference composes it (BiMambaWrapper with tied weights under a fused add + norm):
    hidden, residual (B, L, Dm) -> (mixer output, residual stream)"""
    h, res = K.rms_norm_prenorm(hidden, p["norm_w"], residual, eps)
    xz = F.linear(h, p["in_proj"]).transpose(1, 2)                                                             # (B, 2E, L)
    return K.mamba_inner(xz, p, False) + K.mamba_inner(xz, p, True), res


def graph_reference(key, make, run):
    """make() -> dict of fp32 CPU tensors; run(K, leaves) -> scalar loss over the tensors of `leaves` (every floating tensor of make() is
    a leaf).  -> (inputs, float64 gradients, fp32-autograd deviation per gradient), cached per `key`"""
    def go():
        c = make()
        res = []
        for dtype in (torch.float64, torch.float32):
            lv = {k: _leaf(v, dtype) for k, v in c.items()}
            run(CpuOps(dtype), lv).backward()
            res.append({k: v.grad for k, v in lv.items() if v.grad is not None})
        return c, res[0], {k: SB.metric(res[1][k], res[0][k]) for k in res[0]}
    return R.cached(("block_graph", key), go)
