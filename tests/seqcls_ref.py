"""The pooled classification head restated on CPU (test helper): the recalled Caduceus remote code's
    hs = stack([H[..., :D], flip(H[..., D:], dims=[1, 2])], -1); pooled = pool(hs, 1); logits = (score(p0) + score(p1)) / 2
with the rounding points of DESIGN.md §4f, applied to hidden states (the oracle's, or this engine's own).  Shared by
tests/test_gpu_seqcls.py and tests/test_gpu_launch_forms.py."""
import torch


def rnd(x, dtype):
    return x.to(dtype).float() if dtype == torch.bfloat16 else x.float()


def pool_strands(hs_f, hs_r, pooling, dtype):
    """hs_*: [B, L, D] fp32 values already rounded to `dtype` -> pooled [B, 2, D] fp32 (mean: fp64 sum / L, rounded once)."""
    out = []
    for hs in (hs_f, hs_r):
        if pooling == "mean":
            out.append(rnd((hs.double().sum(1) / hs.shape[1]).float(), dtype))
        elif pooling == "max":
            out.append(hs.max(1).values)
        elif pooling == "first":
            out.append(hs[:, 0])
        else:
            out.append(hs[:, -1])
    return torch.stack(out, 1)


def score_ref(pooled, W, dtype):
    W = rnd(W.float(), dtype).double()
    a0 = rnd((pooled[:, 0].double() @ W.T).float(), dtype)
    a1 = rnd((pooled[:, 1].double() @ W.T).float(), dtype)
    return rnd(rnd(a0 + a1, dtype) / 2, dtype)


def head_ref(H, W, pooling, dtype):
    """The recalled remote code on an RCPS hidden state H [B, L, 2D] (values in `dtype`)."""
    D = H.shape[-1] // 2
    H = H.float().cpu()
    pooled = pool_strands(H[..., :D], torch.flip(H[..., D:], dims=[1, 2]), pooling, dtype)
    return score_ref(pooled, W.cpu(), dtype), pooled
