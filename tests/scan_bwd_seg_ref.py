"""The segmented backward of the selective scan restated in torch (test helper; no tests here): the three phases of
include/pcad_bwd.h pcad_selective_scan_bwd_seg written out by hand - no autograd - in the dtype asked for (float64 by default), on
scan_bwd_ref's operands and layouts, so that tests/test_scan_bwd_seg.py can hold the arithmetic of the segment hand-overs to
scan_bwd_ref.grads (autograd through the plain recurrence) on the CPU.

    phase 1  per segment g, from h = 0 up: e_g, Dsum_g (g < G - 1); from kc = 0 down: kappa_g (g > 0);  P_g = exp(A Dsum_g)
    phase 2  H_0 = 0, H_{g+1} = P_g H_g + e_g ascending;  K_{G-1} = 0, K_{g-1} = P_g K_g + kappa_g descending
    phase 3  per segment: the states from H_g, the adjoint from K_g, the formulas of include/pcad_train.h; dA, dD and dbias as
             per-segment partials added in index order

`drop` (tests): "H", "K" or "P" leaves that hand-over out (H_g = 0, K_g = 0, P_g = 1 in phase 2) - what a broken kernel would compute."""
import torch

CHUNK = 8       # plantcaduceus_amd.ops.SCAN_BWD_CHUNK (held to it in tests/test_scan_bwd_seg.py)


def seg_steps(L, G):
    """steps per segment: CHUNK ceil(ceil(L / G) / CHUNK)"""
    per = -(-L // G)
    return CHUNK * (-(-per // CHUNK))


def grads(x, G, reverse=False, dtype=torch.float64, drop=None):
    """x: scan_bwd_ref.inputs' dict (D / z / delta_bias may be None) -> dict name -> gradient of sum(out * dout), as scan_bwd_ref.grads
    returns them (None for an input that is None), computed in G segments"""
    f = (lambda t: t.flip(-1)) if reverse else (lambda t: t)
    c = lambda t: None if t is None else t.to(dtype)
    u, delta, Bm, Cm, z, g = (None if x[k] is None else f(c(x[k])) for k in ("u", "delta", "B", "C", "z", "dout"))
    A, D, bias = c(x["A"]), c(x["D"]), c(x["delta_bias"])
    Bsz, E, L = u.shape
    N = A.shape[1]
    pre = delta if bias is None else delta + bias[:, None]
    d = torch.where(pre > 20, pre, torch.log1p(torch.exp(torch.clamp(pre, max=20.0))))
    dsig = torch.where(pre > 20, torch.ones_like(pre), torch.sigmoid(pre))
    if z is not None:
        sg = torch.sigmoid(z)
        dy = g * z * sg
    else:
        dy = g
    Dv = torch.zeros(E, dtype=dtype) if D is None else D
    a = lambda s: torch.exp(d[:, :, s, None] * A)                              # (B, E, N)
    inj = lambda s: (d[:, :, s] * u[:, :, s])[..., None] * Bm[:, None, :, s]  # d_s u_s B_s

    steps = seg_steps(L, G)
    Ge = -(-L // steps)
    rng = [(k * steps, min(L, (k + 1) * steps)) for k in range(Ge)]
    zero = torch.zeros(Bsz, E, N, dtype=dtype)
    # phase 1
    e, kappa, P = [None] * Ge, [None] * Ge, [None] * Ge
    for k, (s0, s1) in enumerate(rng):
        if k + 1 < Ge:
            h = zero.clone()
            for s in range(s0, s1):
                h = a(s) * h + inj(s)
            e[k] = h
            P[k] = torch.exp(A * d[:, :, s0:s1].sum(-1)[..., None])
        if k > 0:
            kc = zero.clone()
            for s in range(s1 - 1, s0 - 1, -1):
                kc = a(s) * (dy[:, :, s, None] * Cm[:, None, :, s] + kc)
            kappa[k] = kc
    if drop == "P":
        P = [None if p is None else torch.ones_like(p) for p in P]
    # phase 2
    H, K = [zero.clone()], [None] * Ge
    for k in range(Ge - 1):
        H.append(P[k] * H[k] + e[k])
    K[Ge - 1] = zero.clone()
    for k in range(Ge - 1, 0, -1):
        K[k - 1] = (P[k] * K[k] if k + 1 < Ge else zero) + kappa[k]
    if drop == "H":
        H = [zero.clone() for _ in H]
    if drop == "K":
        K = [zero.clone() for _ in K]
    # phase 3
    du, dd, dz = torch.zeros_like(u), torch.zeros_like(u), torch.zeros_like(u)
    dB, dC = torch.zeros_like(Bm), torch.zeros_like(Cm)
    pA, pD, pb = [], [], []
    for k, (s0, s1) in enumerate(rng):
        h, hp, hs = H[k], {}, {}
        for s in range(s0, s1):
            hp[s] = h
            h = a(s) * h + inj(s)
            hs[s] = h
            if z is not None:
                y = (h * Cm[:, None, :, s]).sum(-1) + Dv * u[:, :, s]
                dz[:, :, s] = g[:, :, s] * y * (sg[:, :, s] * (1 + z[:, :, s] * (1 - sg[:, :, s])))
        kc, dA_k = K[k], zero.clone()
        for s in range(s1 - 1, s0 - 1, -1):
            an = a(s)
            ah = an * hp[s]
            kk = dy[:, :, s, None] * Cm[:, None, :, s] + kc
            dC[:, :, s] = (dy[:, :, s, None] * hs[s]).sum(1)
            dB[:, :, s] = (kk * (d[:, :, s] * u[:, :, s])[..., None]).sum(1)
            du[:, :, s] = dy[:, :, s] * Dv + d[:, :, s] * (kk * Bm[:, None, :, s]).sum(-1)
            dd[:, :, s] = (kk * (A * ah + u[:, :, s, None] * Bm[:, None, :, s])).sum(-1) * dsig[:, :, s]
            dA_k = dA_k + kk * (d[:, :, s, None] * ah)
            kc = an * kk
        pA.append(dA_k.sum(0))
        pD.append((dy[:, :, s0:s1] * u[:, :, s0:s1]).sum((0, 2)))
        pb.append(dd[:, :, s0:s1].sum((0, 2)))
    tot = lambda parts: torch.stack(parts).sum(0)
    return {"u": f(du), "delta": f(dd), "A": tot(pA), "B": f(dB), "C": f(dC), "D": None if D is None else tot(pD),
            "z": None if z is None else f(dz), "delta_bias": None if bias is None else tot(pb)}
