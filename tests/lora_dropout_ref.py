"""Restatements for the LoRA dropout tests: the Philox4x32-10 generator and the keep mask in numpy, and the arithmetic
of one adapted projection - forward and hand-written backward - in torch on the CPU with an explicit mask, in any float dtype."""
import numpy as np
import torch

M0, M1 = 0xD2511F53, 0xCD9E8D57
W0, W1 = 0x9E3779B9, 0xBB67AE85
MASK32 = np.uint64(0xFFFFFFFF)


def philox4x32_10(counter, key):
    """counter: 4 arrays (or ints) of uint32 values, key: 2 -> 4 uint32 arrays.  Vectorised over the arrays' common shape."""
    c = [np.asarray(v, dtype=np.uint64) & MASK32 for v in counter]
    c = list(np.broadcast_arrays(*c))
    k0, k1 = int(key[0]) & 0xFFFFFFFF, int(key[1]) & 0xFFFFFFFF
    for _ in range(10):
        p0 = np.uint64(M0) * c[0]
        p1 = np.uint64(M1) * c[2]
        c = [(p1 >> np.uint64(32)) ^ c[1] ^ np.uint64(k0), p1 & MASK32, (p0 >> np.uint64(32)) ^ c[3] ^ np.uint64(k1), p0 & MASK32]
        k0, k1 = (k0 + W0) & 0xFFFFFFFF, (k1 + W1) & 0xFFFFFFFF
    return [v.astype(np.uint32) for v in c]


def threshold(p: float) -> int:
    """T = floor(p 65536 + 0.5); 65536 (p too close to 1) is refused"""
    T = int(np.floor(float(p) * 65536.0 + 0.5))
    if not 0 <= T <= 65535:
        raise ValueError(f"p={p}: T={T} outside [0, 65535]")
    return T


def keep_scale(p: float) -> np.float32:
    """c = 65536 / (65536 - T) as fp32"""
    return np.float32(65536.0) / np.float32(65536 - threshold(p))


def keep_mask(M: int, K: int, p: float, seed: int, stream: int) -> np.ndarray:
    """bool [M, K]: keep(m, k) of the normative mask; K % 8 == 0"""
    assert K % 8 == 0
    T = threshold(p)
    m = np.arange(M, dtype=np.uint64)[:, None]
    k8 = np.arange(K // 8, dtype=np.uint64)[None, :]
    w = philox4x32_10((k8, m, stream & 0xFFFFFFFF, (stream >> 32) & 0xFFFFFFFF), (seed & 0xFFFFFFFF, (seed >> 32) & 0xFFFFFFFF))
    h = np.empty((M, K // 8, 8), dtype=np.uint32)
    for i in range(8):
        h[:, :, i] = (w[i >> 1] >> np.uint32(16 * (i & 1))) & np.uint32(0xFFFF)
    return (h >= T).reshape(M, K)


def down(x, A, keep, c):
    """t = c (keep x) A^T in A's dtype"""
    return float(c) * ((x.to(A.dtype) * keep.to(A.dtype)) @ A.t())


def down_bwd(x, A, u, dx0, keep, c):
    """-> (dx = dx0 + c keep (u A) in dx0's dtype - a dropped element keeps dx0's value -, dA = c u^T (keep x)) computed in A's dtype"""
    kf = keep.to(A.dtype)
    dA = float(c) * (u.t() @ (x.to(A.dtype) * kf))
    add = float(c) * (u @ A)
    dx = torch.where(keep, (dx0.to(A.dtype) + add).to(dx0.dtype), dx0)
    return dx, dA


def linear_forward(x, W, A, B, scale, keep, c):
    """y = x W^T + scale (t B^T) with t = down(...): the unmerged form, everything in x's dtype (float64 in the checks)"""
    t = down(x, A, keep, c)
    return x @ W.t() + float(scale) * (t @ B.t()), t


def linear_backward(x, W, A, B, scale, keep, c, g):
    """the hand-written backward of §4u in the operands' dtype -> (dx, dA, dB)"""
    t = down(x, A, keep, c)
    u = float(scale) * (g @ B)
    dB = float(scale) * (g.t() @ t)
    dx, dA = down_bwd(x, A, u, g @ W, keep, c)
    return dx, dA, dB


def stream_id(step: int, layer: int, direction: int, module: int) -> int:
    """the model's stream formula: step 2^16 + (layer 2 + dir) 3 + module; module indexes ("in_proj", "x_proj", "out_proj")"""
    return step * 65536 + (layer * 2 + direction) * 3 + module


# ---- the whole fine-tuning model in the UNMERGED form, its masks taken from keep_mask (pool_bwd_ref.model_forward's twin) ---------------
MODULES = ("in_proj", "x_proj", "out_proj")


def model_forward(lv, sd, config, ids, labels, problem_type, p, seed, step, pooling="mean", scale=4.0, dtype=torch.float64):
    """lv: the trainable tensors (pool_bwd_ref.factor_name, "score.weight") in `dtype`; sd: the frozen trunk.  Every adapted projection
    is x W^T + scale (c (keep x) A^T) B^T with keep = keep_mask(rows, K, p, seed, stream_id(step, layer, dir, module)), the rows of
    x [2B, L, K] in index order.  -> (loss, logits) in `dtype`, nothing rounded"""
    import torch.nn.functional as F
    import block_bwd_ref as BB
    import pool_bwd_ref as PB
    import scan_bwd_ref as SB
    from plantcaduceus_amd.checkpoint import EMB_KEY, NORMF_KEY, layer_keys, norm_key
    t = lambda k: sd[k].to(dtype)
    c = float(keep_scale(p))

    def lin(x, W, i, d, mod):
        A, Bf = lv[PB.factor_name(i, ("fwd", "rev")[d], mod, "A")], lv[PB.factor_name(i, ("fwd", "rev")[d], mod, "B")]
        S, L, K = x.shape
        keep = torch.from_numpy(keep_mask(S * L, K, p, seed, stream_id(step, i, d, MODULES.index(mod)))).view(S, L, K)
        return F.linear(x, W) + scale * ((c * ((x * keep.to(dtype)) @ A.t())) @ Bf.t())

    comp = torch.tensor(config.complement_list()[:8], dtype=torch.long)
    ids = ids.long()
    B, L = ids.shape
    h, res = t(EMB_KEY)[torch.cat([ids, comp[ids.flip(1)]], dim=0)], None
    for i in range(config.n_layer):
        hn, res = BB.norm_forward(h, res, t(norm_key(i)), config.norm_epsilon, dtype)
        tied, outs = layer_keys(i, "fwd"), []
        for d, direction in enumerate(("fwd", "rev")):
            k = layer_keys(i, direction)
            E, Rk = sd[k["conv_w"]].shape[0], sd[k["dt_w"]].shape[1]
            xz = lin(hn, t(tied["in_proj"]), i, d, "in_proj")
            xc = BB.conv_forward(xz[..., :E], t(k["conv_w"]).reshape(E, -1), t(k["conv_b"]), bool(d), dtype)
            x_dbl = lin(xc, t(k["x_proj"]), i, d, "x_proj")
            delta = F.linear(x_dbl[..., :Rk], t(k["dt_w"])).transpose(1, 2)
            y = SB.forward(dict(u=xc.transpose(1, 2), delta=delta, A=-torch.exp(t(k["A_log"])), B=x_dbl[..., Rk:Rk + 16].transpose(1, 2),
                                C=x_dbl[..., Rk + 16:].transpose(1, 2), D=t(k["D"]), z=xz[..., E:].transpose(1, 2), delta_bias=t(k["dt_b"])),
                           bool(d), dtype)
            outs.append(lin(y.transpose(1, 2), t(tied["out_proj"]), i, d, "out_proj"))
        h = outs[0] + outs[1]
    logits, _ = PB.head(h, res, t(NORMF_KEY), lv["score.weight"], B, L, pooling, config.norm_epsilon, dtype)
    return (PB.task_loss(logits, labels, problem_type) if labels is not None else None), logits


def model_reference(trainables, sd, config, ids, labels, problem_type, p, seed, step):
    """-> (float64 loss, float64 gradients per name, fp32-autograd deviation per gradient) of the unmerged graph"""
    import scan_bwd_ref as SB
    res = []
    for dtype in (torch.float64, torch.float32):
        lv = {k: v.detach().clone().to(dtype).requires_grad_(True) for k, v in trainables.items()}
        loss, _ = model_forward(lv, sd, config, ids, labels, problem_type, p, seed, step, dtype=dtype)
        loss.backward()
        res.append((loss.detach(), {k: v.grad for k, v in lv.items()}))
    return res[0][0], res[0][1], {k: SB.metric(res[1][1][k], res[0][1][k]) for k in res[0][1]}
