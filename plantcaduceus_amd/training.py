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
`CaduceusForMaskedLM` (and a snapshot of it loads here); the ties are shared storage.  There is no CPU path.  By default autograd
keeps, per layer, what the operators save (DESIGN.md §4n lists it); with `gradient_checkpointing=True` each block keeps only its
inputs `h` and `res` and its forward is run again inside the backward, on the same operators and to the same bits.
The optimizer is `plantcaduceus_amd.optim.AdamW`, the training command `plantcaduceus_amd.pretrain`.

`TrainableCaduceusForSequenceClassification` is the fine-tuning form: the same trunk frozen, one LoRA factor pair per
(layer, direction, target module), a trained `score` head, and the pooled head's backward kernel (`ops.pooled_head_fn`).  The
per-direction in_proj / out_proj factors untie the two directions, so its block is composed here from the single operators:

    per layer   hn, res = ops.rms_norm_fn(h, norm.weight, residual=res, prenorm=True)
      per direction d   xz  = ops.lora_linear_fn(hn, in_proj_d)            x, z = xz halves
                        xc  = ops.causal_conv1d_dir(x, conv_d, reverse=d)
                        xdb = ops.lora_linear_fn(xc, x_proj_d)             delta = F.linear(xdb[:R], dt_proj_d)
                        y   = ops.selective_scan_fn(xc, delta, A_d, B, C, D_d, z, dt_bias_d, reverse=d)
                        o_d = ops.lora_linear_fn(y, out_proj_d)
                h = o_fwd + o_rev
    logits = ops.pooled_head_fn(h, res, norm_f.weight, score, pooling)     loss: HF's, by problem_type, in torch on the fp32 logits

`save_adapter` writes PEFT's layout (plantcaduceus_amd.adapters); the training command is `plantcaduceus_amd.lora_predict train`."""
from __future__ import annotations

import json
import os
from dataclasses import dataclass
from typing import Optional

import torch
import torch.nn.functional as F
from torch import nn
from torch.utils.checkpoint import checkpoint

from . import ops
from .checkpoint import load_state_dict, resolve_snapshot
from .configuration_caduceus import CaduceusConfig, config_from_dict
from .engine import _DT, _require_gpu
from .modeling_caduceus import _LMHead, _MixerModel, _Weight


@dataclass
class MaskedLMTrainingOutput:
    loss: torch.Tensor           # scalar: sum(w nll) / sum(w) over the batch's labelled positions (nan without any), differentiable
    sums: torch.Tensor           # fp32 [B, 4]: sum w nll, sum w, labelled positions, arg-max hits per window
    token_nll: Optional[torch.Tensor] = None      # fp32 [B, L] (return_token_nll): 0 at ignored positions, differentiable


class _Backbone(nn.Module):
    def __init__(self, cfg):
        super().__init__()
        self.backbone = _MixerModel(cfg)


def stored_bytes_per_strand_position(config, dtype: torch.dtype, *, lora: bool, gradient_checkpointing: bool = False) -> int:
    """Bytes autograd keeps per strand position for the whole depth, by the formulas of DESIGN.md: per layer
    ((2D + 8E)e + D r) for the masked LM (§4n), ((2D + 10E + 2(R + 32))e + D r) for the LoRA model (§4p); e is the model dtype's size,
    r the residual's (4 with residual_in_fp32 or an fp32 model).  With gradient_checkpointing each layer keeps its inputs, D(e + r),
    and one block at a time is live in the plain form (§4q).  Host arithmetic: a window of length L has 2L strand positions."""
    if dtype not in _DT:
        raise ValueError(f"unsupported dtype {dtype}: the kernels compute in bf16 or fp32")
    D, E, R, n = int(config.d_model), int(config.d_inner), int(config.dt_rank), int(config.n_layer)
    e = torch.empty((), dtype=dtype).element_size()
    r = 4 if (config.residual_in_fp32 or dtype == torch.float32) else e
    plain = ((2 * D + 10 * E + 2 * (R + 32)) * e if lora else (2 * D + 8 * E) * e) + D * r
    return n * D * (e + r) + plain if gradient_checkpointing else n * plain


class _Recompute:
    """What both trainable models share: the switch, and running a block as one checkpointed unit.  A unit goes through
    torch.utils.checkpoint's saved-tensor hooks (use_reentrant=False): its forward runs once in grad mode - the composed form of the
    operators, whose bits the plain model produces - and keeps only the unit's arguments; the first gradient that reaches the unit
    runs the forward again from them and hands the autograd nodes of the first pass the tensors they saved.  Every Function of `ops`
    saves through save_for_backward, so nothing escapes the hooks.  With grad mode off, or with nothing in or before the unit requiring
    grad, no operator saves anything and nothing is run twice."""

    is_gradient_checkpointing = False

    def gradient_checkpointing_enable(self, gradient_checkpointing_kwargs=None):
        if gradient_checkpointing_kwargs:
            raise NotImplementedError("gradient_checkpointing_kwargs: the units are fixed (one block each, DESIGN.md §4q)")
        self.is_gradient_checkpointing = True

    def gradient_checkpointing_disable(self):
        self.is_gradient_checkpointing = False

    def _run_block(self, blk, h, res):
        if self.is_gradient_checkpointing and torch.is_grad_enabled():
            return checkpoint(self._block, blk, h, res, use_reentrant=False, preserve_rng_state=False)
        return self._block(blk, h, res)

    scan_bwd_segments = 1

    def _set_scan_bwd_segments(self, segments):
        """scan_bwd_segments (1, 2..64 or "auto"): how many segments every scan's BACKWARD cuts a strand into.  An
        attribute of the model that every scan call reads, so a block that gradient checkpointing runs again uses the same value."""
        self.scan_bwd_segments = ops._check_segments(segments)

    scan_fwd_segments = 1

    def _set_scan_fwd_segments(self, segments):
        """scan_fwd_segments (1, 2..64 or "auto"): how many segments every scan's FORWARD cuts a strand into.  An attribute
        as scan_bwd_segments is: a block that gradient checkpointing runs again reads the same value, so it computes the same bits."""
        self.scan_fwd_segments = ops._check_segments(segments)


class TrainableCaduceusForMaskedLM(_Recompute, nn.Module):
    """`TrainableCaduceusForMaskedLM(config, dtype=torch.float32, device="cuda", gradient_checkpointing=False, scan_bwd_segments=1, scan_fwd_segments=1)`: parameters under the
    reference's names with requires_grad=True; `forward(input_ids, labels, loss_weights=None)` -> `.loss`, `.sums` (and `.token_nll` with return_token_nll=True).
    scan_bwd_segments (1, 2..64 or "auto"): the segmented backward of every selective scan; the forward's bits do not depend on it.
    scan_fwd_segments (1, 2..64 or "auto"): the segmented forward of every selective scan; 1 changes no bit, above 1 the scans'
    outputs differ by fp32 rounding and are reproducible for a given value."""

    def __init__(self, config: CaduceusConfig, dtype: torch.dtype = torch.float32, device="cuda", gradient_checkpointing: bool = False,
                 scan_bwd_segments=1, scan_fwd_segments=1):
        super().__init__()
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}: the kernels compute in bf16 or fp32")
        config.check_supported()
        if not getattr(config, "bidirectional_weight_tie", True):
            raise NotImplementedError("bidirectional_weight_tie=False: the trainable model composes the tied form only")
        if config.padded_vocab_size != 8:
            raise NotImplementedError(f"padded vocabulary of {config.padded_vocab_size} rows: the loss head evaluates 8")
        self.config = config
        self.is_gradient_checkpointing = bool(gradient_checkpointing)
        self._set_scan_bwd_segments(scan_bwd_segments)
        self._set_scan_fwd_segments(scan_fwd_segments)
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
    def from_pretrained(cls, pretrained_model_name_or_path, config=None, torch_dtype=None, dtype=None, device="cuda",
                        gradient_checkpointing: bool = False, scan_bwd_segments=1, scan_fwd_segments=1, **kwargs):
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
        model = cls(config, dtype=want or torch.float32, device=device, gradient_checkpointing=gradient_checkpointing,
                    scan_bwd_segments=scan_bwd_segments, scan_fwd_segments=scan_fwd_segments)
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
            h, res = self._run_block(blk, h, res)
        sums, nll = ops.mlm_loss_head_fn(h, res, self.caduceus.backbone.norm_f.weight, emb, comp_list, labels, loss_weights, ignore_index, eps,
                                         return_nll=True)
        return MaskedLMTrainingOutput(loss=sums[:, 0].sum() / sums[:, 1].sum(), sums=sums,      # on the device; 0 / 0 = nan
                                      token_nll=nll if return_token_nll else None)

    def _block(self, blk, h, res):
        """one block, (h, res) -> (h, res): the unit gradient checkpointing keeps the inputs of"""
        cfg = self.config
        hn, res = ops.rms_norm_fn(h, blk.norm.weight, None, res, cfg.norm_epsilon, prenorm=True, residual_in_fp32=cfg.residual_in_fp32)
        bi = blk.mixer.submodule
        xz = ops.linear_fn(hn, bi.mamba_fwd.in_proj.weight).transpose(1, 2)      # (2B, 2E, L); in_proj is tied
        return self._inner(xz, bi.mamba_fwd, False) + self._inner(xz, bi.mamba_rev, True), res

    def _inner(self, xz, m, reverse: bool):
        return ops.mamba_inner_fn(xz, m.conv1d.weight, m.conv1d.bias, m.x_proj.weight, m.dt_proj.weight, m.out_proj.weight, None,
                                  -torch.exp(m.A_log.float()), None, None, D=m.D.float(), delta_bias=m.dt_proj.bias.float(),
                                  delta_softplus=True, reverse=reverse, scan_bwd_segments=self.scan_bwd_segments,
                                  scan_fwd_segments=self.scan_fwd_segments)


# ---- fine-tuning: frozen trunk + LoRA factors + score -----------------------------------------------------------------
PROBLEM_TYPES = ("regression", "single_label_classification", "multi_label_classification")
ADAPTER_PREFIX = "base_model.model."


@dataclass
class SequenceClassificationTrainingOutput:
    loss: Optional[torch.Tensor]     # scalar (labels given): HF's loss by problem_type on the fp32 logits, differentiable
    logits: torch.Tensor             # fp32 [B, num_labels]


def sequence_classification_loss(logits: torch.Tensor, labels: torch.Tensor, problem_type: str, num_labels: int) -> torch.Tensor:
    """HF's loss of `*ForSequenceClassification` (CaduceusForSequenceClassification.loss_from_logits with gradients): MSE on the
    squeezed logits, cross-entropy, or BCE-with-logits"""
    labels = labels.to(logits.device)
    if problem_type == "regression":
        if num_labels == 1:
            return F.mse_loss(logits.squeeze(), labels.squeeze().to(logits.dtype))
        return F.mse_loss(logits, labels.to(logits.dtype))
    if problem_type == "single_label_classification":
        return F.cross_entropy(logits.view(-1, num_labels), labels.view(-1).long())
    return F.binary_cross_entropy_with_logits(logits, labels.to(logits.dtype))


class TrainableCaduceusForSequenceClassification(_Recompute, nn.Module):
    """The trunk under the reference's key names, frozen; `lora_A` / `lora_B` fp32 parameters per (layer, direction, target module)
    under PEFT's names (`...mamba_fwd.in_proj.lora_A.weight`), initialised as PEFT does (A: kaiming_uniform(a=sqrt(5)) = U(+-1/sqrt(in)),
    B: 0); `score.weight` fp32 [num_labels, d_model], initialised as nn.Linear, handed to the kernel rounded to the model dtype with a
    straight-through gradient.  The weights the factors merge into are kept in fp32 whatever the model dtype, so that the merged weight
    is rounded once (adapters.merge_lora).  train_lora=False: the factors exist but do not require grad - the frozen-trunk mode, which
    is what the reference's pinned fast path trains.
    lora_dropout=p > 0: in training mode with grad enabled every adapted projection runs the UNMERGED form
    `ops.lora_dropout_linear_fn`, whose branch input is dropped out by a mask that is a pure function of (`dropout_seed`, stream, row,
    column) with stream = dropout_step 2^16 + (layer 2 + dir) 3 + module; `forward` reads `dropout_step` once, hands it to the blocks
    and increments it after a training forward.  Under `no_grad` or `eval()` the merged call runs, without dropout.
    gradient_checkpointing=True: each block keeps only its inputs and is run again in the backward; same bits.
    scan_bwd_segments (1, 2..64 or "auto"): the segmented backward of every selective scan; no forward bit depends on it.
    scan_fwd_segments (1, 2..64 or "auto"): the segmented forward of every selective scan, with or without grad; 1 changes no bit.
    `forward(input_ids, labels=None)` -> `.loss`, `.logits`.  With train_lora=False the trunk's output of a window never changes:
    `pooled_features(input_ids)` runs it once on the inference engine (`feature_engine`) and `forward(pooled=..., labels=...)` is the
    score head on such cached rows (`ops.pooled_logits_fn`)."""

    def __init__(self, config: CaduceusConfig, num_labels: int, problem_type: str, pooling_strategy: str = "mean",
                 dtype: torch.dtype = torch.float32, device="cuda", r: int = 8, lora_alpha: float = 32,
                 target_modules=("x_proj", "in_proj", "out_proj"), train_lora: bool = True, seed: int = 0,
                 gradient_checkpointing: bool = False, lora_dropout: float = 0.0, scan_bwd_segments=1,
                 scan_fwd_segments=1):
        super().__init__()
        from .adapters import TARGETS
        if dtype not in _DT:
            raise ValueError(f"unsupported dtype {dtype}: the kernels compute in bf16 or fp32")
        config.check_supported()
        if not getattr(config, "bidirectional_weight_tie", True):
            raise NotImplementedError("bidirectional_weight_tie=False: the trainable model starts from the tied form only")
        if pooling_strategy not in ops.TRAINABLE_POOLING:
            raise NotImplementedError(f"pooling_strategy {pooling_strategy!r} has no backward: trainable poolings are {ops.TRAINABLE_POOLING} "
                                      "(the gradient of max pooling needs a tie rule nothing pins; inference keeps it)")
        if problem_type not in PROBLEM_TYPES:
            raise ValueError(f"problem_type must be one of {PROBLEM_TYPES}, got {problem_type!r}")
        bad = [t for t in target_modules if t not in TARGETS]
        if bad or int(r) < 1 or int(num_labels) < 1:
            raise ValueError(f"target_modules must be among {TARGETS}, r and num_labels >= 1 (got {list(target_modules)}, r={r}, num_labels={num_labels})")
        self.config, self.num_labels, self.problem_type, self.pooling_strategy = config, int(num_labels), problem_type, pooling_strategy
        self.dtype, self.r, self.lora_alpha, self.train_lora = dtype, int(r), float(lora_alpha), bool(train_lora)
        self.target_modules = tuple(sorted(target_modules))
        self.is_gradient_checkpointing = bool(gradient_checkpointing)
        self._set_scan_bwd_segments(scan_bwd_segments)
        self._set_scan_fwd_segments(scan_fwd_segments)
        self.lora_dropout, self.dropout_seed, self.dropout_step = float(lora_dropout), 0, 0
        ops.lora_dropout_threshold(self.lora_dropout)
        self.caduceus = _Backbone(config)
        if self.lora_dropout > 0:                                # the masked kernels' limits hold for every adapted projection, or nothing is built
            for mod in self.target_modules:
                ops.lora_dropout_limits(getattr(self.caduceus.backbone.layers[0].mixer.submodule.mamba_fwd, mod).weight.shape[1], self.r,
                                        self.lora_dropout)
        self.to(dtype=dtype)
        g = torch.Generator().manual_seed(int(seed))            # the factors' and the head's initial values
        for blk in self.caduceus.backbone.layers:
            for m in (blk.mixer.submodule.mamba_fwd, blk.mixer.submodule.mamba_rev):
                for mod in TARGETS:
                    holder = getattr(m, mod)
                    holder.weight.data = holder.weight.data.float()          # the tied pair is one Parameter: converted once, shared still
                    if mod in self.target_modules:
                        out_f, in_f = holder.weight.shape
                        holder.lora_A = _Weight(self.r, in_f)
                        holder.lora_B = _Weight(out_f, self.r)
                        with torch.no_grad():
                            holder.lora_A.weight.copy_((torch.rand((self.r, in_f), generator=g) * 2 - 1) / in_f ** 0.5)
                            holder.lora_B.weight.zero_()
        self._feature_engine, self.feature_windows = None, 0     # feature_engine() / pooled_features(): the frozen-trunk mode on cached features
        self.score = _Weight(self.num_labels, config.d_model)
        with torch.no_grad():                                                # nn.Linear's reset_parameters: U(+-1/sqrt(in))
            self.score.weight.copy_((torch.rand((self.num_labels, config.d_model), generator=g) * 2 - 1) / config.d_model ** 0.5)
        self.to(device=device)
        for name, p in self.named_parameters():
            p.requires_grad_(name == "score.weight" or (self.train_lora and ".lora_" in name))

    @classmethod
    def from_pretrained(cls, base_snapshot, num_labels: int, problem_type: str, **kwargs):
        """The trunk from a base snapshot directory or hub id (config.json + weights under the reference's key names)."""
        hub_kw = {k: kwargs.pop(k) for k in ("revision", "cache_dir", "local_files_only", "token") if k in kwargs}
        path = resolve_snapshot(base_snapshot, **hub_kw)
        with open(os.path.join(path, "config.json")) as f:
            config = config_from_dict(json.load(f))
        model = cls(config, num_labels, problem_type, **kwargs)
        model.load_trunk({k: v for k, v in load_state_dict(path).items() if k.startswith("caduceus.")})
        return model

    def load_trunk(self, sd):
        """the frozen trunk's tensors (reference key names); factors and score are left as they are"""
        missing, unexpected = self.load_state_dict(sd, strict=False)
        missing = [k for k in missing if ".lora_" not in k and k != "score.weight"]
        if missing or unexpected:
            raise ValueError(f"trunk state dict does not fit: missing {missing[:4]}, unexpected {list(unexpected)[:4]}")

    def adapter_state_dict(self):
        """PEFT's adapter tensors: every factor and the score head under `base_model.model.`, fp32 on the CPU"""
        return {ADAPTER_PREFIX + k: p.detach().to("cpu", torch.float32).contiguous() for k, p in self.named_parameters()
                if ".lora_" in k or k == "score.weight"}

    def save_adapter(self, path: str, base_model_name_or_path: Optional[str]):
        """adapter_config.json + adapter_model.safetensors in the layout adapters.audit_adapter accepts"""
        from safetensors.torch import save_file
        from .adapters import ADAPTER_CONFIG
        os.makedirs(path, exist_ok=True)
        cfg = {"base_model_name_or_path": base_model_name_or_path, "r": self.r,
               "lora_alpha": int(self.lora_alpha) if float(self.lora_alpha).is_integer() else self.lora_alpha, "lora_dropout": self.lora_dropout,
               "target_modules": list(self.target_modules), "task_type": "SEQ_CLS", "modules_to_save": ["classifier", "score"],
               "peft_type": "LORA", "bias": "none", "inference_mode": True}
        with open(os.path.join(path, ADAPTER_CONFIG), "w") as f:
            json.dump(cfg, f, indent=2)
        save_file(self.adapter_state_dict(), os.path.join(path, "adapter_model.safetensors"), metadata={"format": "pt"})

    def load_adapter_weights(self, path: str):
        """read `save_adapter`'s directory back into the factors and the score head (audited against this model's r and targets)"""
        from .adapters import audit_adapter, read_adapter_config, read_adapter_weights
        cfg = read_adapter_config(path)
        if cfg["r"] != self.r or float(cfg["lora_alpha"]) != self.lora_alpha or tuple(cfg["target_modules"]) != self.target_modules:
            raise ValueError(f"{path}: r / lora_alpha / target_modules {cfg['r']} / {cfg['lora_alpha']} / {cfg['target_modules']} are not this "
                             f"model's {self.r} / {self.lora_alpha} / {list(self.target_modules)}")
        sd = read_adapter_weights(path)
        audit_adapter(sd, cfg, n_layer=self.config.n_layer, d_model=self.config.d_model)
        own = dict(self.named_parameters())
        want = {k for k in own if ".lora_" in k or k == "score.weight"}
        got = {k[len(ADAPTER_PREFIX):] if k.startswith(ADAPTER_PREFIX) else k: v for k, v in sd.items()}
        if set(got) != want:
            raise ValueError(f"{path}: adapter tensors do not match this model's (e.g. {sorted(set(got) ^ want)[:3]})")
        with torch.no_grad():
            for k, v in got.items():
                if tuple(v.shape) != tuple(own[k].shape):
                    raise ValueError(f"{path}: {k} has shape {tuple(v.shape)}, expected {tuple(own[k].shape)}")
                own[k].copy_(v)

    def loss_from_logits(self, logits: torch.Tensor, labels: torch.Tensor) -> torch.Tensor:
        """CaduceusForSequenceClassification.loss_from_logits: the loss without gradient (lora_predict.eval_loss calls it per batch)"""
        with torch.no_grad():
            return sequence_classification_loss(logits, labels, self.problem_type, self.num_labels)

    LORA_MODULES = ("in_proj", "x_proj", "out_proj")            # a module's index in the dropout stream formula

    def dropout_stream(self, step: int, layer: int, reverse: bool, module: str) -> int:
        """the mask stream of one adapted projection at one step: step 2^16 + (layer 2 + dir) 3 + module"""
        return int(step) * 65536 + (int(layer) * 2 + int(bool(reverse))) * 3 + self.LORA_MODULES.index(module)

    def _linear(self, x, holder, stream: Optional[int] = None):
        if hasattr(holder, "lora_A"):
            if stream is not None and self.lora_dropout > 0 and self.training and torch.is_grad_enabled():
                return ops.lora_dropout_linear_fn(x, holder.weight, holder.lora_A.weight, holder.lora_B.weight, self.lora_alpha / self.r,
                                                  self.lora_dropout, self.dropout_seed, stream)
            return ops.lora_linear_fn(x, holder.weight, holder.lora_A.weight, holder.lora_B.weight, self.lora_alpha / self.r)
        return F.linear(x, holder.weight.to(x.dtype))

    def _direction(self, hn, m, reverse: bool, layer: int = 0, step: Optional[int] = None):
        E, R, dt = self.config.d_inner, self.config.dt_rank, hn.dtype
        stream = (lambda mod: None) if step is None else (lambda mod: self.dropout_stream(step, layer, reverse, mod))
        xz = self._linear(hn, m.in_proj, stream("in_proj"))                                      # (2B, L, 2E)
        xc = ops.causal_conv1d_dir(xz[..., :E], m.conv1d.weight.reshape(E, -1), m.conv1d.bias, reverse)
        x_dbl = self._linear(xc, m.x_proj, stream("x_proj"))                                     # (2B, L, R + 32)
        delta = F.linear(x_dbl[..., :R], m.dt_proj.weight.to(dt)).transpose(1, 2)                # (2B, E, L)
        y = ops.selective_scan_fn(xc.transpose(1, 2), delta, -torch.exp(m.A_log.float()), x_dbl[..., R:R + 16].transpose(1, 2),
                                  x_dbl[..., R + 16:].transpose(1, 2), m.D.float(), z=xz[..., E:].transpose(1, 2),
                                  delta_bias=m.dt_proj.bias.float(), delta_softplus=True, reverse=reverse, segments=self.scan_bwd_segments,
                                  fwd_segments=self.scan_fwd_segments)
        return self._linear(y.transpose(1, 2), m.out_proj, stream("out_proj"))

    def _block(self, blk, h, res, layer: int = 0, step: Optional[int] = None):
        """one block, (h, res) -> (h, res): the unit gradient checkpointing keeps the inputs of.  layer / step: the block's index and
        the forward's dropout step (None: no dropout) - plain arguments, so that a checkpointed block that runs again sees the same"""
        cfg = self.config
        hn, res = ops.rms_norm_fn(h, blk.norm.weight, None, res, cfg.norm_epsilon, prenorm=True, residual_in_fp32=cfg.residual_in_fp32)
        bi = blk.mixer.submodule
        return self._direction(hn, bi.mamba_fwd, False, layer, step) + self._direction(hn, bi.mamba_rev, True, layer, step), res

    def _run_block(self, blk, h, res, layer: int = 0, step: Optional[int] = None):
        if step is None:
            return super()._run_block(blk, h, res)
        if self.is_gradient_checkpointing and torch.is_grad_enabled():
            return checkpoint(self._block, blk, h, res, layer, step, use_reentrant=False, preserve_rng_state=False)
        return self._block(blk, h, res, layer, step)

    def feature_engine(self, engine_options=None):
        """The inference engine bound to the frozen trunk's base weights in the tied form, as CaduceusForSequenceClassification binds
        them (every trunk tensor in the model dtype; the factors are not bound) - built at the first call and kept; `engine_options`
        (a mapping, e.g. {"f32_gemm_split": 1}) is read then and only then.  Allowed only with train_lora=False: with
        trained factors the two directions untie and the trunk's output moves with every step, so nothing about it can be kept."""
        if self.train_lora:
            raise ValueError("feature_engine needs train_lora=False: with trained LoRA factors the trunk's features change every step "
                             "(and the directions untie); the frozen-trunk mode alone can run the trunk on the inference engine")
        if self._feature_engine is None:
            import copy
            from .engine import Engine
            emb = self.caduceus.backbone.embeddings.word_embeddings.embedding.weight
            _require_gpu(emb, "the model")
            cfg = copy.copy(self.config)
            cfg.engine_options = dict(engine_options or {})
            sd = {"caduceus." + k: (v.to(self.dtype) if v.is_floating_point() else v) for k, v in self.caduceus.state_dict().items()
                  if ".lora_" not in k}
            self._feature_engine = Engine(cfg, sd, self.dtype, emb.device)
        return self._feature_engine

    def pooled_features(self, input_ids) -> torch.Tensor:
        """the frozen trunk's pooled vectors fp32 [B, 2, D] of the windows input_ids [B, L], from `feature_engine()` under no_grad with
        this model's pooling; `feature_windows` counts the windows sent through the engine"""
        eng = self.feature_engine()
        with torch.no_grad():
            _, pooled = eng.forward_pooled(input_ids, self.pooling_strategy, self.score.weight, want_pooled=True)
        self.feature_windows += int(input_ids.shape[0])
        return pooled

    def logits_from_features(self, pooled) -> torch.Tensor:
        """logits fp32 [B, NL] of cached `pooled_features` rows: the engine's own head arithmetic, differentiable in `score`"""
        return ops.pooled_logits_fn(pooled, self.score.weight, self.dtype)

    def forward(self, input_ids=None, labels=None, *, pooled=None) -> SequenceClassificationTrainingOutput:
        if (input_ids is None) == (pooled is None):
            raise ValueError("exactly one of input_ids [B, L] and pooled [B, 2, D] (cached pooled_features rows)")
        if pooled is not None:
            logits = self.logits_from_features(pooled)
            loss = sequence_classification_loss(logits, labels, self.problem_type, self.num_labels) if labels is not None else None
            return SequenceClassificationTrainingOutput(loss=loss, logits=logits)
        cfg = self.config
        emb = self.caduceus.backbone.embeddings.word_embeddings.embedding.weight
        _require_gpu(emb, "the model")
        _require_gpu(input_ids, "input_ids")
        if input_ids.dim() != 2:
            raise ValueError(f"input_ids must be [B, L], got {tuple(input_ids.shape)}")
        comp = torch.tensor(cfg.complement_list()[:8], dtype=torch.long, device=emb.device)
        ids = input_ids.long()
        strands = torch.cat([ids, comp[ids.flip(1)]], dim=0)                                     # [2B, L]
        h, res = F.embedding(strands, emb), None
        eps = cfg.norm_epsilon
        dropping = self.lora_dropout > 0 and self.training and torch.is_grad_enabled()
        step = int(self.dropout_step) if dropping else None      # read once: every block of this forward, run again or not, sees this value
        for i, blk in enumerate(self.caduceus.backbone.layers):
            h, res = self._run_block(blk, h, res, i, step)
        if dropping:
            self.dropout_step = step + 1
        logits = ops.pooled_head_fn(h, res, self.caduceus.backbone.norm_f.weight, self.score.weight, self.pooling_strategy, eps)
        loss = sequence_classification_loss(logits, labels, self.problem_type, self.num_labels) if labels is not None else None
        return SequenceClassificationTrainingOutput(loss=loss, logits=logits)
