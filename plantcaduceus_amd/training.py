"""A trainable CaduceusForMaskedLM: the model's forward with labels composed from the differentiable operators of `ops`, so that
`loss.backward()` runs on this project's backward kernels.

    S = [ids ; comp[flip(ids)]]                                  the 2B-strand form
    h = F.embedding(S, emb)
    per layer   hn, res = ops.rms_norm_fn(h, norm.weight, residual=res, prenorm=True)                  pcad_add_rmsnorm(_bwd)
                xz      = F.linear(hn, in_proj.weight)                                                 stock PyTorch-ROCm
                h       = ops.mamba_inner_fn(xz, mamba_fwd...) + ops.mamba_inner_fn(xz, mamba_rev..., reverse=True)
    sums = ops.mlm_loss_head_fn(h, res, norm_f.weight, emb, comp, labels, loss_weights)                pcad_loss_head(_bwd)
    loss = sums[:, 0].sum() / sums[:, 1].sum()

The module tree is `modeling_caduceus`'s parameter holders, so `state_dict()` has the reference's key names and loads into
`CaduceusForMaskedLM` (and a snapshot of it loads here); the ties are shared storage.  There is no CPU path, and no gradient
checkpointing or LoRA wrapping here: autograd keeps, per layer, what the operators save (DESIGN.md §4n lists it).  The optimizer is
`plantcaduceus_amd.optim.AdamW`, the training command `plantcaduceus_amd.pretrain`."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn

from . import ops
from .checkpoint import load_state_dict, resolve_snapshot
from .configuration_caduceus import CaduceusConfig, config_from_dict
from .engine import _DT, _require_gpu
from .modeling_caduceus import _LMHead, _MixerModel


@dataclass
class MaskedLMTrainingOutput:
    loss: torch.Tensor           # scalar: sum(w nll) / sum(w) over the batch's labelled positions (nan without any), differentiable
    sums: torch.Tensor           # fp32 [B, 4]: sum w nll, sum w, labelled positions, arg-max hits per window
    token_nll: Optional[torch.Tensor] = None      # fp32 [B, L] (return_token_nll): 0 at ignored positions, differentiable


class _Backbone(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.backbone = _MixerModel(cfg)


class TrainableCaduceusForMaskedLM(nn.Module):
    """`TrainableCaduceusForMaskedLM(config, dtype=torch.float32, device="cuda")`: parameters under the reference's names with
    requires_grad=True; `forward(input_ids, labels, loss_weights=None)` -> `.loss`, `.sums` (and `.token_nll` with return_token_nll=True)."""

    def __init__(self, config: CaduceusConfig, dtype: torch.dtype = torch.float32, device="cuda"):
        super().__init__()
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}: the kernels compute in bf16 or fp32")
        config.check_supported()
        if not getattr(config, "bidirectional_weight_tie", True):
            raise NotImplementedError("bidirectional_weight_tie=False: the trainable model composes the tied form only")
        if config.padded_vocab_size != 8:
            raise NotImplementedError(f"padded vocabulary of {config.padded_vocab_size} rows: the loss head evaluates 8")
        self.config = config
        self.caduceus = _Backbone(config)
        self.lm_head = _LMHead(config)
        self.tie_weights()
        self.to(device=device, dtype=dtype)
        for p in self.parameters():
            p.requires_grad_(True)

    def tie_weights(self):
        """the LM head is the embedding; mamba_rev's in_proj / out_proj are mamba_fwd's (the holders tie those when they are built)"""
        self.lm_head.lm_head.weight = self.caduceus.backbone.embeddings.word_embeddings.embedding.weight

    @classmethod
    def from_pretrained(cls, pretrained_model_name_or_path, config=None, torch_dtype=None, dtype=None, device="cuda", **kwargs):
        """A snapshot directory or hub id, read by the loader of the inference classes (config.json + safetensors / bin with the
        reference's key names; tied keys restored)."""
        hub_kw = {k: kwargs[k] for k in ("revision", "cache_dir", "local_files_only", "token") if k in kwargs}
        path = resolve_snapshot(pretrained_model_name_or_path, **hub_kw)
        if config is None:
            with open(os.path.join(path, "config.json")) as f:
                config = config_from_dict(json.load(f))
        want = dtype if dtype is not None else torch_dtype
        if isinstance(want, str):
            want = getattr(torch, want) if want != "auto" else None
        model = cls(config, dtype=want or torch.float32, device=device)
        model.load_state_dict(load_state_dict(path))
        return model

    def forward(self, input_ids, labels, loss_weights=None, ignore_index: int = -100, return_token_nll: bool = False) -> MaskedLMTrainingOutput:
        cfg = self.config
        emb = self.caduceus.backbone.embeddings.word_embeddings.embedding.weight
        _require_gpu(emb, "the model")
        _require_gpu(input_ids, "input_ids")
        _require_gpu(labels, "labels")
        if loss_weights is not None:
            _require_gpu(loss_weights, "loss_weights")
        if input_ids.dim() != 2 or labels.shape != input_ids.shape:
            raise ValueError(f"input_ids and labels must be [B, L], got {tuple(input_ids.shape)} and {tuple(labels.shape)}")
        comp_list = cfg.complement_list()[:8]
        comp = torch.tensor(comp_list, dtype=torch.long, device=emb.device)
        ids = input_ids.long()
        strands = torch.cat([ids, comp[ids.flip(1)]], dim=0)                     # [2B, L]
        h, res = F.embedding(strands, emb), None
        eps = cfg.norm_epsilon
        for blk in self.caduceus.backbone.layers:
            hn, res = ops.rms_norm_fn(h, blk.norm.weight, None, res, eps, prenorm=True, residual_in_fp32=cfg.residual_in_fp32)
            bi = blk.mixer.submodule
            xz = F.linear(hn, bi.mamba_fwd.in_proj.weight).transpose(1, 2)       # (2B, 2E, L); in_proj is tied
            h = self._inner(xz, bi.mamba_fwd, False) + self._inner(xz, bi.mamba_rev, True)
        sums, nll = ops.mlm_loss_head_fn(h, res, self.caduceus.backbone.norm_f.weight, emb, comp_list, labels, loss_weights, ignore_index, eps,
                                         return_nll=True)
        return MaskedLMTrainingOutput(loss=sums[:, 0].sum() / sums[:, 1].sum(), sums=sums,      # on the device; 0 / 0 = nan
                                      token_nll=nll if return_token_nll else None)

    @staticmethod
    def _inner(xz, m, reverse: bool):
        return ops.mamba_inner_fn(xz, m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.out_proj.weight, None,
                                  -torch.exp(m.A_log.float()), None, None, D=m.D.float(), delta_bias=m.dt_proj.bias.float(),
                                  delta_softplus=True, reverse=reverse)
