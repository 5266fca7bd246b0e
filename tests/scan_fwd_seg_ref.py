"""The segmented training forward of the selective scan restated in torch (test helper; no tests here): the three phases of
include/pcad_bwd.h pcad_selective_scan_fwd_seg written out as the kernels of csrc/scan_fwd_seg.hip walk them, in the dtype asked for
(float64 by default), on scan_bwd_ref's operands and layouts, so that tests/test_scan_fwd_seg.py can hold the arithmetic of the segment
hand-overs to scan_bwd_ref.forward (the plain recurrence) on the CPU.

    phase 1  per segment g < G - 1, from h = 0 up: e_g, Dsum_g = sum d_s
    phase 2  H_0 = 0, H_{g+1} = P_g H_g + e_g ascending, P_g = exp2(A log2(e) Dsum_g)
    phase 3  per segment, from H_g: h_s = exp2(d_s log2(e) A) h_{s-1} + d_s u_s B_s;  y_s = D u_s + sum_n h_s[n] C_s[n] in index order;
             out_s = y_s silu(z_s)

The cut rule is scan_bwd_seg_ref.seg_steps, the backward's.  `drop` (tests): "P" leaves P_g out of phase 2 (P_g = 1), "H" starts every
segment from zero - what a broken kernel would compute."""
import math

import torch

import scan_bwd_seg_ref as SS

LOG2E = math.log2(math.e)


def forward(x, G, reverse=False, dtype=torch.float64, drop=None):
    """x: scan_bwd_ref.inputs' dict (D / z / delta_bias may be None) -> out (B, E, L) in `dtype`, as scan_bwd_ref.forward returns it,
    computed in G segments"""
    f = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    c = lambda t: None if t is None else t.to(dtype)
    u, delta, Bm, Cm, z = (None if x[k] is None else f(c(x[k])) for k in ("u", "delta", "B", "C", "z"))
    A, D, bias = c(x["A"]), c(x["D"]), c(x["delta_bias"])
    Bsz, E, L = u.shape
    N = A.shape[1]
    pre = delta if bias is None else delta + bias[:, None]
    d = torch.where(pre > 20, pre, torch.log1p(torch.exp(torch.clamp(pre, max=20.0))))
    Dv = torch.zeros(E, dtype=dtype) if D is None else D
    log2e = torch.tensor(LOG2E, dtype=dtype)

    def step(h, s):                                                            # one walk step of either walking kernel
        d2 = d[:, :, s] * log2e
        return torch.exp2(d2[..., None] * A) * h + (d[:, :, s] * u[:, :, s])[..., None] * Bm[:, None, :, s]

    steps = SS.seg_steps(L, G)
    Ge = -(-L // steps)
    rng = [(k * steps, min(L, (k + 1) * steps)) for k in range(Ge)]
    zero = torch.zeros(Bsz, E, N, dtype=dtype)
    # phase 1
    e, dsum = [None] * Ge, [None] * Ge
    for k, (s0, s1) in enumerate(rng[:-1]):
        h, ds = zero.clone(), torch.zeros(Bsz, E, dtype=dtype)
        for s in range(s0, s1):
            ds = ds + d[:, :, s]
            h = step(h, s)
        e[k], dsum[k] = h, ds
    # phase 2
    H = [zero.clone()]
    for k in range(Ge - 1):
        P = torch.ones_like(zero) if drop == "P" else torch.exp2((dsum[k] * log2e)[..., None] * A)
        H.append(P * H[k] + e[k])
    if drop == "H":
        H = [zero.clone() for _ in H]
    # phase 3
    out = torch.zeros_like(u)
    for k, (s0, s1) in enumerate(rng):
        h = H[k]
        for s in range(s0, s1):
            h = step(h, s)
            y = Dv * u[:, :, s]
            for n in range(N):
                y = y + h[:, :, n] * Cm[:, n, s, None]
            out[:, :, s] = y
    if z is not None:
        out = out * (z * torch.sigmoid(z))
    return f(out)
