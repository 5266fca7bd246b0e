"""The whole-model reference of the trainable masked LM (test helper; no tests here): the 2B-strand form of DESIGN.md §1 as one torch
graph over block_bwd_ref's operator restatements and head_bwd_ref's head, differentiated by torch.autograd on the CPU.

    S = [ids ; comp[flip(ids)]]     h = Emb[S]
    per layer:  hn, res = add + norm(h, res);  xz = in_proj(hn);  h = mamba_inner(xz, mamba_fwd, walk ->) + mamba_inner(xz, mamba_rev, walk <-)
    lg = head(h, res)     nll = cross entropy at the labelled positions     loss = sum(w nll) / sum(w)

Parameters are the tensors of a state dict with the reference's key names; a tied pair (mamba_rev's in_proj / out_proj, the LM head)
is ONE leaf under its first name, so its gradient is the sum of both uses."""
import torch
import torch.nn.functional as F

import block_bwd_ref as BB
import head_bwd_ref as HB
import scan_bwd_ref as SB
import scan_ref as R
from plantcaduceus_amd.checkpoint import EMB_KEY, LMHEAD_KEY, NORMF_KEY, layer_keys, norm_key


def tied_alias(config):
    """state-dict key -> the key of the leaf that holds it"""
    alias = {LMHEAD_KEY: EMB_KEY}
    for i in range(config.n_layer):
        f, r = layer_keys(i, "fwd"), layer_keys(i, "rev")
        alias[r["in_proj"]] = f["in_proj"]
        alias[r["out_proj"]] = f["out_proj"]
    return alias


def leaves(sd, config, dtype, rnd=R.ident):
    """one leaf per untied tensor of the state dict (rounded by rnd first: what a bf16 model stores)"""
    alias = tied_alias(config)
    return {k: rnd(v.float()).to(dtype).requires_grad_(True) for k, v in sd.items() if k not in alias}


def _mamba(lv, keys):
    E = lv[keys["conv_w"]].shape[0]
    return dict(conv_w=lv[keys["conv_w"]].reshape(E, -1), conv_b=lv[keys["conv_b"]], x_proj=lv[keys["x_proj"]], dt_proj=lv[keys["dt_w"]],
                delta_bias=lv[keys["dt_b"]], A=-torch.exp(lv[keys["A_log"]]), D=lv[keys["D"]])


def forward(lv, config, ids, labels, loss_weights=None, ignore_index=-100, dtype=torch.float64):
    """lv: `leaves`.  -> dict(logits [B, L, 8], nll [B, L], sums0 [B] = sum w nll, sumw [B], loss), all in `dtype`"""
    K = BB.CpuOps(dtype)
    comp = torch.tensor(config.complement_list()[:8], dtype=torch.long)
    ids = ids.long()
    B, L = ids.shape
    S = torch.cat([ids, comp[ids.flip(1)]], dim=0)
    h, res = lv[EMB_KEY][S], None
    for i in range(config.n_layer):
        kf, kr = layer_keys(i, "fwd"), layer_keys(i, "rev")
        hn, res = K.rms_norm_prenorm(h, lv[norm_key(i)], res, config.norm_epsilon)
        xz = F.linear(hn, lv[kf["in_proj"]]).transpose(1, 2)
        pf, pr = _mamba(lv, kf), _mamba(lv, kr)
        pf["out_proj"] = pr["out_proj"] = lv[kf["out_proj"]]
        h = K.mamba_inner(xz, pf, False) + K.mamba_inner(xz, pr, True)
    lg = HB.head_logits(h, res, lv[NORMF_KEY], lv[EMB_KEY], B, L, config.norm_epsilon, dtype, comp=comp.tolist())
    nll = HB.token_nll(lg, labels, ignore_index)
    m = HB.labelled_mask(labels, ignore_index).to(dtype)
    w = m if loss_weights is None else loss_weights.to(dtype) * m
    s0, sw = (w * nll).sum(1), w.sum(1)
    return dict(logits=lg, nll=nll, sums0=s0, sumw=sw, loss=s0.sum() / sw.sum())


def reference(key, sd, config, ids, labels, loss_weights, rnd=R.ident):
    """(float64 forward values, float64 gradients per leaf key, fp32-autograd deviation per gradient) of the loss; cached per `key`"""
    def go():
        res = []
        for dtype in (torch.float64, torch.float32):
            lv = leaves(sd, config, dtype, rnd)
            out = forward(lv, config, ids, labels, loss_weights, dtype=dtype)
            out["loss"].backward()
            res.append(({k: v.detach() for k, v in out.items()}, {k: v.grad for k, v in lv.items()}))
        return res[0][0], res[0][1], {k: SB.metric(res[1][1][k], res[0][1][k]) for k in res[0][1]}
    return R.cached(("model_bwd", key), go)
