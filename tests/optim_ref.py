"""Restatement of the optimizer step of csrc/optim.hip (include/pcad_bwd.h pcad_adamw_step) in plain torch, in any float
dtype: clip_grad_norm_'s rule on grad_scale * grad, then torch.optim.AdamW's arithmetic, a non-finite norm skipping the step.  Also the
sizing formulas and the case sets that tests/test_optim_ref.py (CPU) and tests/test_gpu_optim.py share."""
import math

import torch

CHUNK = 4096                 # include/pcad_bwd.h PCAD_OPTIM_CHUNK
FIN_LANES = 1024             # csrc/optim.hip: lanes of the block that adds the chunks' partial sums
EDGE_SIZES = (0, 1, 7, 8, 9, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5)


def chunk_count(sizes, chunk=CHUNK):
    return sum(-(-n // chunk) for n in sizes)


def scratch_bytes(chunks):
    return 0 if chunks <= 0 else (4 * chunks + 255) // 256 * 256


def grad_norm(grads, grad_scale=1.0):
    """the float64 total norm of grad_scale * grad"""
    return math.sqrt(sum(float((g.double() * grad_scale).pow(2).sum()) for g in grads))


def clip_coef(norm, max_norm, grad_scale=1.0):
    return grad_scale * (min(1.0, max_norm / (norm + 1e-6)) if max_norm > 0 else 1.0)


def adamw_step(params, grads, exp_avgs, exp_avg_sqs, decay, lr, beta1, beta2, eps, weight_decay, step, max_norm=0.0, grad_scale=1.0):
    """one step in place on lists of tensors of one float dtype; -> (norm, coef, finite)"""
    norm = grad_norm(grads, grad_scale)
    if not math.isfinite(norm):
        return norm, float("nan"), False
    coef = clip_coef(norm, max_norm, grad_scale)
    bc1, bc2 = 1.0 - beta1 ** step, 1.0 - beta2 ** step
    for p, g0, m, v, d in zip(params, grads, exp_avgs, exp_avg_sqs, decay):
        g = coef * g0.to(p.dtype)
        if d:
            p.mul_(1.0 - lr * weight_decay)
        m.mul_(beta1).add_(g, alpha=1.0 - beta1)
        v.mul_(beta2).add_(g * g, alpha=1.0 - beta2)
        p.sub_((lr / bc1) * m / (v.sqrt() / math.sqrt(bc2) + eps))
    return norm, coef, True


def torch_adamw(params, decay, lr, beta1, beta2, eps, weight_decay, **kw):
    """torch.optim.AdamW over `params` with weight decay only where `decay` says so"""
    groups = [{"params": [p for p, d in zip(params, decay) if d], "weight_decay": weight_decay},
              {"params": [p for p, d in zip(params, decay) if not d], "weight_decay": 0.0}]
    return torch.optim.AdamW([g for g in groups if g["params"]], lr=lr, betas=(beta1, beta2), eps=eps, **kw)


def norm_bar(chunks, chunk=CHUNK):
    """relative bar of the fp32 norm against float64, from the depth of the reduction.  Every fp32 addition of non-negative terms adds at
    most 2^-24 relative error to the sum, so a sum that passed through `depth` additions is within depth * 2^-24: a lane's serial walk
    (chunk / 256 additions over fp32 gradients, the longer of the two dtypes), 6 butterfly levels and 4 wave sums in the block, then
    ceil(chunks / 1024) serial additions, 6 levels and 16 wave sums in the finalising block.  The scaling of an
    element and its squaring add 3 (the scaled value's rounding counts twice in the square), the gradient's own rounding none (the
    float64 norm is taken of the same stored values); the square root halves the relative error and rounds once."""
    depth = (chunk // 256 + 6 + 4) + (-(-max(chunks, 1) // FIN_LANES) + 6 + 16) + 3
    return (depth / 2 + 1) * 2.0 ** -24
