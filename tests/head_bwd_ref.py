"""The reference of the loss head's backward (test helper; no tests here): a torch restatement of norm_f -> RC re-assembly -> tied RCPS
LM head -> weighted cross entropy in the 2B-strand form, differentiated by torch.autograd on the CPU.

    v = h + res                       rows (b, t) of the forward strand and (B + b, L-1-t) of the rc strand, h / res [2B*L, D]
    o = v rsqrt(mean(v^2) + eps) w    (bf: rounded to bf16 with a straight-through derivative, as include/pcad_bwd.h states)
    lg[b, t] = o[b, t] . Emb^T + o[B + b, L-1-t] . Emb[comp]^T
    nll = logsumexp(lg) - lg[label]   at the labelled positions: label != ignore_index, 0 <= label < 8
    sums[b, 0] = sum_t wt nll

The restatement runs in the dtype it is asked for: float64 is the reference, float32 through the identical code measures what fp32
arithmetic alone costs (the bars: scan_bwd_ref.bar).  `grads` differentiates  sum_b dsum[b] sums[b, 0] + sum dnll nll;  with
`kernel_logits` it is the vector-Jacobian product of the head graph with the cotangent formed in float64 from those logits."""
import math

import torch

import scan_bwd_ref as SB
import scan_ref as R

COMP = [0, 1, 2, 6, 5, 4, 3, 7]
SEG = 64                 # positions per block of the kernel (ops.LOSS_SEG; pinned by tests/test_head_bwd_ref.py)
NAMES = ("h", "res", "norm_weight", "emb")


def labelled_mask(labels, ignore_index=-100):
    """the positions the loss head evaluates: ignore_index and negative labels are ignored, any other label outside [0, 8) contributes
    nothing either"""
    labels = labels.long()
    return (labels != ignore_index) & (labels >= 0) & (labels < 8)


def _st_round(y):
    """round to bf16 (through fp32, as the kernel's product is), identity in the derivative"""
    return y + (R.bf16(y.detach().float()).to(y.dtype) - y.detach())


def head_logits(h, res, norm_weight, emb, B, L, eps, dtype=torch.float64, comp=COMP, bf=False):
    """-> [B, L, 8] in `dtype`.  h, res [2B*L, D] (or [2B, L, D])"""
    D = h.shape[-1]
    v = (h.to(dtype) + res.to(dtype)).reshape(2 * B, L, D)
    o = v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * norm_weight.to(dtype)
    if bf:
        o = _st_round(o)
    e = emb.to(dtype)
    return o[:B] @ e.t() + o[B:].flip(1) @ e[torch.tensor(comp, dtype=torch.long)].t()


def token_nll(lg, labels, ignore_index=-100):
    """[B, L] in lg's dtype: the cross entropy over all 8 logits, 0 where the position is not labelled"""
    m = labelled_mask(labels, ignore_index)
    nll = -torch.log_softmax(lg, dim=-1).gather(-1, labels.long().clamp(0, 7).unsqueeze(-1)).squeeze(-1)
    return torch.where(m, nll, torch.zeros_like(nll))


def _leaf(t, dtype):
    return t.detach().clone().to(dtype).requires_grad_(True)


def grads(c, dtype=torch.float64, kernel_logits=None):
    """c: the dict of `inputs`.  -> dict(h, res, norm_weight, emb): the gradients of sum_b dsum[b] sums[b, 0] + sum dnll nll.
    kernel_logits [B, L, 8]: the cotangent of the logits is formed (in float64) from these instead of the restatement's own, and the
    result is the vector-Jacobian product of the head graph with it."""
    lv = {k: _leaf(c[k], dtype) for k in NAMES}
    B, L = c["B"], c["L"]
    lg = head_logits(lv["h"], lv["res"], lv["norm_weight"], lv["emb"], B, L, c["eps"], dtype, bf=c["bf"])
    wt = torch.ones(B, L, dtype=dtype) if c["loss_weights"] is None else c["loss_weights"].to(dtype)
    up = c["dsum"].to(dtype)[:, None] * wt + (c["dnll"].to(dtype) if c["dnll"] is not None else 0.0)
    if kernel_logits is None:
        loss = (up * token_nll(lg, c["labels"], c["ignore_index"])).sum()
    else:
        m = labelled_mask(c["labels"], c["ignore_index"])
        onehot = torch.nn.functional.one_hot(c["labels"].long().clamp(0, 7), 8).to(dtype)
        dlg = (up * m.to(dtype))[..., None] * (torch.softmax(kernel_logits.to(dtype), -1) - onehot)
        loss = (lg * dlg).sum()
    loss.backward()
    return {k: v.grad for k, v in lv.items()}


def make_labels(g, B, L, mode):
    """mode 'all': every position labelled;  'some': about 15 % - every window keeps at least one labelled position and, where the
    window has more than one segment, segment 1 of window 0 has none;  'mixed': 'some' plus a window without labels (B >= 2), negative
    labels and one label of 9 (which contributes nothing)"""
    lab = torch.randint(0, 8, (B, L), generator=g)
    if mode == "all":
        return lab.to(torch.int32)
    keep = torch.rand(B, L, generator=g) < 0.15
    for b in range(B):
        keep[b, (7 * b + 3) % min(L, SEG)] = True
    if L > SEG:
        keep[0, SEG:2 * SEG] = False
    lab = torch.where(keep, lab, torch.full_like(lab, -100))
    if mode == "mixed":
        if B >= 2:
            lab[1] = -100
        flat = lab.view(-1)
        idx = torch.nonzero(flat >= 0).view(-1)
        if idx.numel() >= 3:
            flat[idx[1]] = -1
            flat[idx[-1]] = -7
            flat[idx[idx.numel() // 2]] = 9
        for b in range(B):
            if b != 1 or B < 2:
                lab[b, (7 * b + 3) % min(L, SEG)] = (b + 3) % 8
    return lab.to(torch.int32)


def inputs(seed, B, L, D, labels="some", weights=False, dnll=False, bf=False, res_bf=False, eps=1e-5):
    """bf: what a bf16 call stores in bf16 (h, the embedding; res_bf: the residual stream too) is rounded first, so that the reference
    sees the kernel's operands.  Value ranges as tests/test_gpu_mlm_loss.py: logits of a few units."""
    g = torch.Generator().manual_seed(seed)
    r, rr = (R.bf16 if bf else R.ident), (R.bf16 if res_bf else R.ident)
    rows = 2 * B * L
    c = dict(h=r(torch.randn(rows, D, generator=g)), res=rr(torch.randn(rows, D, generator=g) * 0.5 + 0.25),
             norm_weight=torch.rand(D, generator=g) + 0.5, emb=r(torch.randn(8, D, generator=g) * (3.0 / math.sqrt(D))),
             labels=make_labels(g, B, L, labels),
             loss_weights=torch.tensor([0.0, 0.1, 1.0, 2.5])[torch.randint(0, 4, (B, L), generator=g)] if weights else None,
             dsum=torch.rand(B, generator=g) + 0.5, dnll=torch.randn(B, L, generator=g) if dnll else None,
             B=B, L=L, eps=eps, ignore_index=-100, bf=bf)
    return c


def reference(key, make):
    """(inputs, float64 gradients, fp32-autograd deviation per gradient) of the inputs `make()` builds; cached per `key`, computed once"""
    def run():
        c = make()
        g64, g32 = grads(c, torch.float64), grads(c, torch.float32)
        return c, g64, {k: SB.metric(g32[k], g64[k]) for k in g64}
    return R.cached(("head_bwd", key), run)
