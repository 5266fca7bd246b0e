"""The reference of the pooled classification head's backward (test helper; no tests here): tests/seqcls_ref.py's forward - norm_f,
per-strand pooling, score, (fwd + rc) / 2 with the rounding points of DESIGN.md §4f - restated as one torch graph in the 2B-strand form
and differentiated by torch.autograd on the CPU.

    v = h + res                       rows b L + p of the forward strand and (B + b) L + p of the rc strand, h / res [2B*L, D]
    o = v rsqrt(mean(v^2) + eps) w    (bf: rounded to bf16, as every rounding below, with a straight-through derivative)
    pooled[b, s] = mean over the strand's own rows (sum / L, rounded once) | row 0 | row L-1
    logits[b, n] = round(round(round(pooled[b, 0] . W[n]) + round(pooled[b, 1] . W[n])) / 2)

The restatement runs in the dtype it is asked for: float64 is the reference, float32 through the identical code measures what fp32
arithmetic alone costs (the bars: scan_bwd_ref.bar).  `grads` differentiates sum(dlogits * logits); with `kernel_pooled` the score
head reads those pooled vectors (straight through), which is what pcad_pooled_head_bwd is handed."""
import math

import torch
import torch.nn.functional as F

import block_bwd_ref as BB
import scan_bwd_ref as SB
import scan_ref as R
from plantcaduceus_amd.checkpoint import EMB_KEY, NORMF_KEY, layer_keys, norm_key

SEG = 64                 # rows per block of the kernel (ops.POOL_BWD_SEG; pinned by tests/test_pool_bwd_ref.py)
NAMES = ("h", "res", "norm_weight", "score_w")
POOLINGS = ("mean", "first", "last")


def _st_round(y):
    """round to bf16 (through fp32, as the kernel's value is), identity in the derivative"""
    return y + (R.bf16(y.detach().float()).to(y.dtype) - y.detach())


def head(h, res, norm_weight, score_w, B, L, pooling, eps, dtype=torch.float64, bf=False, kernel_pooled=None):
    """-> (logits [B, NL], pooled [B, 2, D]) in `dtype`.  h, res [2B*L, D] (or [2B, L, D])"""
    rnd = _st_round if bf else (lambda y: y)
    D = h.shape[-1]
    v = (h.to(dtype) + res.to(dtype)).reshape(2 * B, L, D)
    o = rnd(v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + eps) * norm_weight.to(dtype))
    if pooling == "mean":
        p = rnd(o.sum(1) / L)
    elif pooling == "first":
        p = o[:, 0]
    elif pooling == "last":
        p = o[:, L - 1]
    else:
        raise ValueError(pooling)
    pooled = torch.stack([p[:B], p[B:]], dim=1)                     # [B, 2, D]: each strand pooled over its own rows
    if kernel_pooled is not None:
        pooled = pooled + (kernel_pooled.to(dtype) - pooled).detach()
    W = score_w.to(dtype)
    a0, a1 = rnd(pooled[:, 0] @ W.t()), rnd(pooled[:, 1] @ W.t())
    return rnd(rnd(a0 + a1) / 2), pooled


def _leaf(t, dtype):
    return t.detach().clone().to(dtype).requires_grad_(True)


def grads(c, dtype=torch.float64, kernel_pooled=None):
    """c: the dict of `inputs`.  -> dict(h, res, norm_weight, score_w): the gradients of sum(dlogits * logits)"""
    lv = {k: _leaf(c[k], dtype) for k in NAMES}
    lg, _ = head(lv["h"], lv["res"], lv["norm_weight"], lv["score_w"], c["B"], c["L"], c["pooling"], c["eps"], dtype, c["bf"], kernel_pooled)
    (lg * c["dlogits"].to(dtype)).sum().backward()
    return {k: v.grad for k, v in lv.items()}


def inputs(seed, B, L, D, NL, pooling="mean", bf=False, res_bf=False, eps=1e-5):
    """bf: what a bf16 call stores in bf16 (h, the score weight; res_bf: the residual stream too) is rounded first, so that the
    reference sees the kernel's operands.  Logits of a few units."""
    g = torch.Generator().manual_seed(seed)
    r, rr = (R.bf16 if bf else R.ident), (R.bf16 if res_bf else R.ident)
    rows = 2 * B * L
    return dict(h=r(torch.randn(rows, D, generator=g)), res=rr(torch.randn(rows, D, generator=g) * 0.5 + 0.25),
                norm_weight=torch.rand(D, generator=g) + 0.5, score_w=r(torch.randn(NL, D, generator=g) * (3.0 / math.sqrt(D))),
                dlogits=torch.randn(B, NL, generator=g), B=B, L=L, NL=NL, pooling=pooling, eps=eps, bf=bf)


def reference(key, make):
    """(inputs, float64 gradients, fp32-autograd deviation per gradient) of the inputs `make()` builds; cached per `key`, computed once"""
    def run():
        c = make()
        g64, g32 = grads(c, torch.float64), grads(c, torch.float32)
        return c, g64, {k: SB.metric(g32[k], g64[k]) for k in g64}
    return R.cached(("pool_bwd", key), run)


# ---- the whole fine-tuning model: model_bwd_ref's block with per-direction merged weights, and the pooled head ---------------------------
TARGETS = ("in_proj", "x_proj", "out_proj")
TASKS = {"classification": (2, "single_label_classification"), "regression": (1, "regression"), "multi_label": (5, "multi_label_classification")}


def factor_name(i, direction, mod, ab):
    return f"caduceus.backbone.layers.{i}.mixer.submodule.mamba_{direction}.{mod}.lora_{ab}.weight"


def task_loss(logits, labels, problem_type):
    """HF's loss of *ForSequenceClassification on the logits, in their dtype"""
    if problem_type == "regression":
        return F.mse_loss(logits.squeeze(), labels.squeeze().to(logits.dtype))
    if problem_type == "single_label_classification":
        return F.cross_entropy(logits, labels.view(-1).long())
    return F.binary_cross_entropy_with_logits(logits, labels.to(logits.dtype))


def model_forward(lv, sd, config, ids, labels, problem_type, pooling="mean", scale=4.0, dtype=torch.float64):
    """lv: the trainable tensors (every factor under `factor_name`, "score.weight") in `dtype`; sd: the frozen trunk's state dict.
    -> (loss, logits [B, NL]) in `dtype`, nothing rounded"""
    K = BB.CpuOps(dtype)
    t = lambda k: sd[k].to(dtype)
    comp = torch.tensor(config.complement_list()[:8], dtype=torch.long)
    ids = ids.long()
    B, L = ids.shape
    S = torch.cat([ids, comp[ids.flip(1)]], dim=0)
    h, res = t(EMB_KEY)[S], None
    for i in range(config.n_layer):
        hn, res = K.rms_norm_prenorm(h, t(norm_key(i)), res, config.norm_epsilon)
        tied = layer_keys(i, "fwd")
        outs = []
        for direction, reverse in (("fwd", False), ("rev", True)):
            k = layer_keys(i, direction)
            E = sd[k["conv_w"]].shape[0]
            merged = {m: t(tied[m] if m != "x_proj" else k[m]) + scale * lv[factor_name(i, direction, m, "B")] @ lv[factor_name(i, direction, m, "A")]
                      for m in TARGETS}
            p = dict(conv_w=t(k["conv_w"]).reshape(E, -1), conv_b=t(k["conv_b"]), x_proj=merged["x_proj"], dt_proj=t(k["dt_w"]),
                     delta_bias=t(k["dt_b"]), A=-torch.exp(t(k["A_log"])), D=t(k["D"]), out_proj=merged["out_proj"])
            outs.append(K.mamba_inner(F.linear(hn, merged["in_proj"]).transpose(1, 2), p, reverse))
        h = outs[0] + outs[1]
    logits, _ = head(h, res, t(NORMF_KEY), lv["score.weight"], B, L, pooling, config.norm_epsilon, dtype)
    return (task_loss(logits, labels, problem_type) if labels is not None else None), logits


def model_reference(key, trainables, sd, config, ids, labels, problem_type, pooling="mean"):
    """trainables: name -> fp32 tensor.  (float64 loss and logits, float64 gradients per name, fp32-autograd deviation per gradient)"""
    def go():
        res = []
        for dtype in (torch.float64, torch.float32):
            lv = {k: _leaf(v, dtype) for k, v in trainables.items()}
            loss, logits = model_forward(lv, sd, config, ids, labels, problem_type, pooling, dtype=dtype)
            loss.backward()
            res.append((loss.detach(), logits.detach(), {k: v.grad for k, v in lv.items()}))
        return res[0][0], res[0][1], res[0][2], {k: SB.metric(res[1][2][k], res[0][2][k]) for k in res[0][2]}
    return R.cached(("seqcls_model", key), go)
