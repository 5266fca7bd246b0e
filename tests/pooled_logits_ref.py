"""The reference of the score head on cached pooled vectors (test helper; no tests here): include/pcad_bwd.h pcad_pooled_logits and
pcad_pooled_logits_bwd restated in float64 on the CPU.

    logits[b, n]     = round(round(round(pooled[b, 0] . W[n]) + round(pooled[b, 1] . W[n])) / 2)      (bf: roundings to bf16, else none)
    dscore_w[n, :]   = 1/2 sum_b dlogits[b, n] (pooled[b, 0, :] + pooled[b, 1, :])
    dpooled[b, s, :] = 1/2 sum_n dlogits[b, n] W[n, :]                                              (the same for both strands)

The backward is written out as the header's formulas, not taken from autograd: tests/test_pooled_logits_ref.py holds the forward to
tests/seqcls_ref.py's head and the formulas to central finite differences of the unrounded forward."""
import math

import torch

import scan_ref as R


def logits(pooled, score_w, bf=False, dtype=torch.float64):
    """pooled [B, 2, D], score_w [NL, D] (already rounded to the model dtype where that matters) -> logits [B, NL] in `dtype`"""
    rnd = (lambda y: R.bf16(y.float()).to(dtype)) if bf else (lambda y: y)
    p, W = pooled.to(dtype), score_w.to(dtype)
    a0, a1 = rnd(p[:, 0] @ W.t()), rnd(p[:, 1] @ W.t())
    return rnd(rnd(a0 + a1) / 2)


def backward(pooled, score_w, dlogits, dtype=torch.float64):
    """-> (dscore_w [NL, D], dpooled [B, 2, D]) in `dtype`: every rounding of the forward is the identity in the derivative"""
    p, W, g = pooled.to(dtype), score_w.to(dtype), dlogits.to(dtype)
    dscore_w = 0.5 * (g.t() @ (p[:, 0] + p[:, 1]))
    half = 0.5 * (g @ W)
    return dscore_w, torch.stack([half, half], dim=1)


def inputs(seed, B, D, NL, bf=False):
    """pooled vectors of order one (what norm_f's pooled rows are), a score weight that gives logits of a few units (rounded to bf16
    with bf, as the kernel is handed it) and a cotangent"""
    g = torch.Generator().manual_seed(seed)
    r = R.bf16 if bf else R.ident
    return dict(pooled=r(torch.randn(B, 2, D, generator=g)), score_w=r(torch.randn(NL, D, generator=g) * (3.0 / math.sqrt(D))),
                dlogits=torch.randn(B, NL, generator=g), bf=bf)


def head_only_adamw(feats, labels, batches, score0, lr, weight_decay=0.01, max_norm=1.0, bf=False):
    """The frozen-trunk run restated in float64: cross entropy of `logits` on the cached rows of each micro-batch, clip_grad_norm_ and
    AdamW (optim_ref.adamw_step) on the score weight alone.  feats [N, 2, D], labels int64 [N], batches: one index array per step.
    -> the step losses"""
    import optim_ref as OR
    p = [score0.detach().double().clone()]
    m, v = [torch.zeros_like(p[0])], [torch.zeros_like(p[0])]
    out = []
    for step, idx in enumerate(batches):
        idx = torch.as_tensor(idx, dtype=torch.long)
        W = R.bf16(p[0].float()).double() if bf else p[0]
        x, y = feats[idx].double(), labels[idx]
        lg = logits(x, W, bf)
        out.append(torch.nn.functional.cross_entropy(lg, y).item())
        dlg = (torch.softmax(lg, dim=1) - torch.nn.functional.one_hot(y, lg.shape[1]).double()) / len(idx)
        dW, _ = backward(x, W, dlg)
        OR.adamw_step(p, [dW], m, v, [True], lr, 0.9, 0.999, 1e-8, weight_decay, step + 1, max_norm=max_norm)
    return out
