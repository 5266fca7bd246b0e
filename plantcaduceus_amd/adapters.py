"""PEFT LoRA adapters of the fine-tuned PlantCAD2 models (reference src/lora_fine_tune.py `create_peft_model` :608-617,
`PeftModel.from_pretrained` in `predict` / `evaluate`) without `peft`.

The adapter layout is PEFT's, which `/reference` does not contain; it is restated here from the public PEFT code (recalled, as
oracle/caduceus_oracle.py restates the RCPS wiring):
  adapter_config.json        base_model_name_or_path, r, lora_alpha, target_modules, task_type ("SEQ_CLS"), modules_to_save
  adapter_model.safetensors  (or adapter_model.bin)
      base_model.model.caduceus.backbone.layers.{i}.mixer.submodule.mamba_{fwd,rev}.{x_proj,in_proj,out_proj}.lora_{A,B}.weight
      base_model.model.score.weight                                   [num_labels, d_model]  (the trained head)
  accepted variants: a `.default` adapter-name infix (`lora_A.default.weight`, `score.modules_to_save.default.weight`) and keys
  without the `base_model.model.` prefix.  Any other key fails, in the style of checkpoint.audit_snapshot.

LoRA deltas (DESIGN.md §4f "LoRA policy").  Under the reference's pinned mamba-ssm 2.2.2 + causal-conv1d 1.4.0, `Mamba.forward`'s
fast path hands `in_proj.weight`, `x_proj.weight` and `out_proj.weight` as tensors to `mamba_inner_fn`; it never calls the modules
PEFT wraps, and the wrapper's `.weight` is the base weight.  PEFT initialises `lora_B` to zero, those parameters then receive no
gradient, so an adapter trained there carries lora_B == 0 and is "frozen trunk + trained score".  `lora_deltas`:
  "auto"   (default) all lora_B exactly zero: bind the base weights (logged); otherwise ValueError naming the tensors
  "ignore" bind the base weights whatever the deltas are (what the pinned fast path computes)
  "apply"  merge the deltas into the weights (`merge_lora`: W + lora_alpha / r * B A per direction, in fp32, cast once) - what an
           environment computes in which `Mamba.forward` calls the wrapped modules (no causal-conv1d, use_fast_path=False, a newer
           stack).  Per-direction in_proj / out_proj deltas untie the two directions: the engine is then bound with
           "untied_directions" 1; x_proj is per direction anyway and merges into the tied form.
"""
from __future__ import annotations

import json
import logging
import os
import re
from typing import Dict, Optional

import torch

from .checkpoint import resolve_snapshot

logger = logging.getLogger(__name__)

ADAPTER_CONFIG = "adapter_config.json"
ADAPTER_WEIGHTS = ("adapter_model.safetensors", "adapter_model.bin")
TARGETS = ("x_proj", "in_proj", "out_proj")
TASKS = {"classification": (2, "single_label_classification"), "regression": (1, "regression"),
         "multi_label": (None, "multi_label_classification")}

_LORA_RE = re.compile(r"^(?:base_model\.model\.)?caduceus\.backbone\.layers\.(\d+)\.mixer\.submodule\.mamba_(fwd|rev)\."
                      r"(x_proj|in_proj|out_proj)\.lora_(A|B)(?:\.default)?\.weight$")
_SCORE_RE = re.compile(r"^(?:base_model\.model\.)?score(?:\.modules_to_save\.default)?\.weight$")


def read_adapter_config(path: str) -> dict:
    with open(os.path.join(path, ADAPTER_CONFIG)) as f:
        cfg = json.load(f)
    for k in ("r", "lora_alpha", "target_modules"):
        if k not in cfg:
            raise ValueError(f"{path}/{ADAPTER_CONFIG} lacks {k!r}")
    tm = cfg["target_modules"]
    cfg["target_modules"] = sorted([tm] if isinstance(tm, str) else list(tm))
    bad = [t for t in cfg["target_modules"] if t not in TARGETS]
    if bad:
        raise ValueError(f"{path}: LoRA target modules {bad} are not among {list(TARGETS)} (the reference's create_peft_model)")
    if cfg.get("task_type") not in (None, "SEQ_CLS"):
        raise ValueError(f"{path}: task_type {cfg.get('task_type')!r}, expected 'SEQ_CLS'")
    return cfg


def read_adapter_weights(path: str) -> Dict[str, torch.Tensor]:
    for fn in ADAPTER_WEIGHTS:
        full = os.path.join(path, fn)
        if os.path.exists(full):
            if fn.endswith(".safetensors"):
                from safetensors.torch import load_file
                return dict(load_file(full))
            return dict(torch.load(full, map_location="cpu", weights_only=True))
    raise FileNotFoundError(f"{path}: no {' / '.join(ADAPTER_WEIGHTS)}")


def audit_adapter(sd: Dict[str, torch.Tensor], cfg: dict, n_layer: Optional[int] = None, d_model: Optional[int] = None) -> dict:
    """Sort the adapter's tensors into LoRA factors and the score head; any other key, a factor of a module that is not a target,
    a layer outside the base or an inconsistent rank fails (ValueError listing the problems)."""
    lora: Dict[tuple, Dict[str, torch.Tensor]] = {}
    score = None
    problems = []
    for k, v in sd.items():
        m = _LORA_RE.match(k)
        if m:
            layer, direction, mod, ab = int(m.group(1)), m.group(2), m.group(3), m.group(4)
            if mod not in cfg["target_modules"]:
                problems.append(f"{k}: {mod} is not a target module {cfg['target_modules']}")
            if n_layer is not None and layer >= n_layer:
                problems.append(f"{k}: layer {layer} outside the base's {n_layer} layers")
            if v.dim() != 2 or (ab == "A" and v.shape[0] != cfg["r"]) or (ab == "B" and v.shape[1] != cfg["r"]):
                problems.append(f"{k}: shape {tuple(v.shape)} does not have rank r={cfg['r']}")
            lora.setdefault((layer, direction, mod), {})[ab] = v
            continue
        if _SCORE_RE.match(k):
            if score is not None:
                problems.append(f"{k}: a second score weight")
            score = v
            continue
        problems.append(f"unexpected tensor {k}")
    for key, ab in lora.items():
        if set(ab) != {"A", "B"}:
            problems.append("layers.%d.mamba_%s.%s: lora_A / lora_B incomplete" % key)
    if score is None:
        problems.append("no score weight (base_model.model.score.weight): the adapter does not carry the trained head")
    elif score.dim() != 2 or (d_model is not None and score.shape[1] != d_model):
        problems.append(f"score weight shape {tuple(score.shape)} does not match d_model={d_model}")
    if problems:
        raise ValueError("adapter does not pass the audit:\n  - " + "\n  - ".join(problems))
    return {"lora": lora, "score": score}


def lora_delta_report(lora: Dict[tuple, Dict[str, torch.Tensor]], r: int, alpha: float) -> dict:
    """-> {"nonzero": [names of lora_B tensors with a non-zero entry], "max_abs_delta": max |alpha / r * B A|}."""
    scale = float(alpha) / float(r)
    nonzero, worst = [], 0.0
    for (layer, direction, mod), ab in sorted(lora.items()):
        B = ab["B"].float()
        if torch.count_nonzero(B).item():
            nonzero.append(f"caduceus.backbone.layers.{layer}.mixer.submodule.mamba_{direction}.{mod}.lora_B.weight")
            worst = max(worst, (scale * (B @ ab["A"].float())).abs().max().item())
    return {"nonzero": nonzero, "max_abs_delta": worst}


def merge_lora(base_sd: Dict[str, torch.Tensor], lora: Dict[tuple, Dict[str, torch.Tensor]], r: int, alpha: float,
               dtype: Optional[torch.dtype] = None) -> Dict[str, torch.Tensor]:
    """The base state dict (reference key names, `caduceus.backbone. ...`) with the LoRA deltas merged in: for each
    (layer, direction, module) with factors, `W_dir = W + (alpha / r) * B @ A`, formed in fp32 on the host.  x_proj merges into
    that direction's own x_proj; in_proj / out_proj - one tied tensor in the base - come back as distinct `mamba_fwd.*` /
    `mamba_rev.*` tensors, a direction without factors keeping W (a tied duplicate missing from base_sd is taken from mamba_fwd's).
    dtype: cast the merged tensors to the model dtype - once, after the merge; the other tensors are returned as they are."""
    scale = float(alpha) / float(r)
    out = dict(base_sd)
    for (layer, direction, mod), ab in sorted(lora.items()):
        key = f"caduceus.backbone.layers.{layer}.mixer.submodule.mamba_{direction}.{mod}.weight"
        src = key if key in base_sd else key.replace(".mamba_rev.", ".mamba_fwd.")
        W = base_sd[src].detach().to("cpu", torch.float32)
        delta = scale * (ab["B"].detach().to("cpu", torch.float32) @ ab["A"].detach().to("cpu", torch.float32))
        if tuple(delta.shape) != tuple(W.shape):
            raise ValueError(f"{key}: LoRA delta {tuple(delta.shape)} does not match the weight {tuple(W.shape)}")
        merged = W + delta
        out[key] = merged.to(dtype) if dtype is not None else merged
        if mod != "x_proj":      # the other direction's name must exist too, and must not alias the merged tensor
            other = key.replace(f".mamba_{direction}.", ".mamba_rev." if direction == "fwd" else ".mamba_fwd.")
            if (int(layer), "rev" if direction == "fwd" else "fwd", mod) not in lora:
                Wo = base_sd[other] if other in base_sd else base_sd[src]
                out[other] = Wo.detach().to("cpu", torch.float32).to(dtype) if dtype is not None else Wo.detach().clone()
    return out


def untie_directions(model) -> None:
    """Give every layer's mamba_rev its own in_proj / out_proj parameters (copies of mamba_fwd's) and make the engine bind with
    "untied_directions" 1.  Must run before the model's engine exists (the option is read when the weights are bound)."""
    owner = model._backbone_owner()
    if getattr(owner, "_pcad_engine", None) is not None:
        raise RuntimeError("untie_directions: the engine is already bound; untie before the first forward")
    for blk in owner.backbone.layers:
        bm = blk.mixer.submodule
        for mod in ("in_proj", "out_proj"):
            src = getattr(bm.mamba_fwd, mod).weight
            getattr(bm.mamba_rev, mod).weight = torch.nn.Parameter(src.detach().clone(), requires_grad=False)
    opts = dict(getattr(model.config, "engine_options", None) or {})
    opts["untied_directions"] = 1
    model.config.engine_options = opts


def load_adapter(dir_or_hub_id: str, task_type: str = "classification", num_labels: Optional[int] = None,
                 lora_deltas: str = "auto", base: Optional[str] = None, dtype=torch.float32, device=None,
                 pooling_strategy: str = "mean", **hub_kwargs):
    """The reference's `load_base_model` + `PeftModel.from_pretrained` (src/lora_fine_tune.py :566-605, :503-515) ->
    CaduceusForSequenceClassification with the adapter's trained `score`.  dir_or_hub_id: adapter directory or hub id (local
    files / HF cache only); base: the base snapshot (default: the adapter's base_model_name_or_path; the reference's
    --model_name).  task_type: classification (2 labels) / regression (1) / multi_label (num_labels > 1)."""
    from .modeling_caduceus import CaduceusForSequenceClassification
    if task_type not in TASKS:
        raise ValueError(f"task_type must be one of {list(TASKS)}, got {task_type!r}")
    if lora_deltas not in ("auto", "ignore", "apply"):
        raise ValueError(f"lora_deltas must be 'auto', 'ignore' or 'apply', got {lora_deltas!r}")
    nl, problem_type = TASKS[task_type]
    if task_type == "multi_label":
        if num_labels is None or int(num_labels) <= 1:
            raise ValueError("For multi_label, please provide num_labels > 1")
        nl = int(num_labels)
    path = resolve_snapshot(dir_or_hub_id, **hub_kwargs)
    cfg = read_adapter_config(path)
    base = base or cfg.get("base_model_name_or_path")
    if not base:
        raise ValueError(f"{path}/{ADAPTER_CONFIG} names no base_model_name_or_path; pass the base snapshot")
    base_path = resolve_snapshot(base, **hub_kwargs)
    kw = dict(num_labels=nl, pooling_strategy=pooling_strategy, torch_dtype=dtype)
    if task_type == "classification":
        kw.update(id2label={0: "NEGATIVE", 1: "POSITIVE"}, label2id={"NEGATIVE": 0, "POSITIVE": 1})
    else:
        kw["problem_type"] = problem_type
    model = CaduceusForSequenceClassification.from_pretrained(base_path, **kw)
    sd = read_adapter_weights(path)
    aud = audit_adapter(sd, cfg, n_layer=model.config.n_layer, d_model=model.config.d_model)
    if tuple(aud["score"].shape) != tuple(model.score.weight.shape):
        raise ValueError(f"adapter score weight {tuple(aud['score'].shape)} does not match num_labels={nl}, "
                         f"d_model={model.config.d_model} {tuple(model.score.weight.shape)}")
    rep = lora_delta_report(aud["lora"], cfg["r"], cfg["lora_alpha"])
    applied = None
    if lora_deltas == "apply":
        from .checkpoint import load_state_dict
        # only the pairs that change anything are merged: a null delta neither moves a weight nor unties a direction
        live = {k: ab for k, ab in aud["lora"].items() if torch.count_nonzero(ab["B"]).item()}
        untied = any(mod != "x_proj" for (_, _, mod) in live)
        if live:
            # from the snapshot's own precision, so that a bf16 model's merged weights are rounded once
            base_sd = {k: v for k, v in load_state_dict(base_path).items() if k.startswith("caduceus.")}
            merged = merge_lora(base_sd, live, cfg["r"], cfg["lora_alpha"], dtype=dtype)
            if untied:
                untie_directions(model)
            own = model.state_dict()
            with torch.no_grad():
                for (layer, direction, mod) in live:
                    names = [f"caduceus.backbone.layers.{layer}.mixer.submodule.mamba_{direction}.{mod}.weight"]
                    if mod != "x_proj":
                        names.append(names[0].replace(f".mamba_{direction}.", ".mamba_rev." if direction == "fwd" else ".mamba_fwd."))
                    for k in names:
                        own[k].copy_(merged[k].to(own[k].dtype))
        applied = {"merged_pairs": len(live), "untied_directions": bool(untied)}
        logger.info("%d LoRA factor pair(s) of %s merged into the weights (lora_deltas='apply'; largest |lora_alpha / r * B A| = %.3e); "
                    "bound %s", len(live), path, rep["max_abs_delta"],
                    "with untied_directions 1 (per-direction in_proj / out_proj)" if untied else "in the tied form")
    elif rep["nonzero"]:
        msg = (f"{len(rep['nonzero'])} LoRA B factor(s) of {path} are non-zero, e.g. {rep['nonzero'][:3]}; largest "
               f"|lora_alpha / r * B A| = {rep['max_abs_delta']:.3e}")
        if lora_deltas == "auto":
            raise ValueError(msg + ". Pass lora_deltas='ignore' (--lora-deltas ignore) to bind the base weights, which is what the "
                             "reference's pinned mamba-ssm fast path computes (it never reads the LoRA modules), or lora_deltas='apply' "
                             "(--lora-deltas apply) to merge the deltas, which is what a run that calls the wrapped modules computes")
        logger.warning("%s; binding the base weights (lora_deltas='ignore')", msg)
    elif aud["lora"]:
        logger.info("%d LoRA factor pairs of %s have lora_B == 0: the deltas are null, the base weights are bound",
                    len(aud["lora"]), path)
    with torch.no_grad():
        model.score.weight.copy_(aud["score"].to(model.score.weight.dtype))
    model.adapter_info = {"path": path, "base": base_path, "r": cfg["r"], "lora_alpha": cfg["lora_alpha"],
                          "target_modules": cfg["target_modules"], "lora_pairs": len(aud["lora"]),
                          "nonzero_lora_B": rep["nonzero"], "max_abs_delta": rep["max_abs_delta"]}
    if applied is not None:
        model.adapter_info.update(lora_deltas="apply", **applied)
    if device is not None:
        model.to(device)
    return model


def make_synthetic_adapter(path: str, base_cfg, num_labels: int, lora_b_scale: float = 0.0, base_path: Optional[str] = None,
                           seed: int = 0, r: int = 8, lora_alpha: int = 32, targets=TARGETS, prefix: bool = True,
                           default_infix: bool = False, score_scale: float = 0.05, bin_format: bool = False) -> Dict[str, torch.Tensor]:
    """Write an adapter in PEFT's layout (create_peft_model's LoRA r 8, alpha 32, targets x_proj / in_proj / out_proj, SEQ_CLS)
    for tests: lora_A ~ U(-1/sqrt(in), 1/sqrt(in)), lora_B = lora_b_scale * N(0, 1) (0: PEFT's initial value), score ~
    score_scale * N(0, 1).  prefix=False drops `base_model.model.`; default_infix=True writes the `.default` adapter-name infixes.
    -> the tensors written."""
    os.makedirs(path, exist_ok=True)
    g = torch.Generator().manual_seed(seed)
    D, E, R, N = base_cfg.d_model, base_cfg.d_inner, base_cfg.dt_rank, base_cfg.d_state
    shapes = {"in_proj": (2 * E, D), "x_proj": (R + 2 * N, E), "out_proj": (D, E)}     # (out, in)
    pre = "base_model.model." if prefix else ""
    inf = ".default" if default_infix else ""
    sd: Dict[str, torch.Tensor] = {}
    for i in range(base_cfg.n_layer):
        for d in ("fwd", "rev"):
            for mod in targets:
                out_f, in_f = shapes[mod]
                k = f"{pre}caduceus.backbone.layers.{i}.mixer.submodule.mamba_{d}.{mod}"
                sd[f"{k}.lora_A{inf}.weight"] = (torch.rand((r, in_f), generator=g) * 2 - 1) / in_f ** 0.5
                sd[f"{k}.lora_B{inf}.weight"] = torch.randn((out_f, r), generator=g) * lora_b_scale
    sd[f"{pre}score{'.modules_to_save.default' if default_infix else ''}.weight"] = \
        torch.randn((num_labels, D), generator=g) * score_scale
    cfg = {"base_model_name_or_path": base_path, "r": r, "lora_alpha": lora_alpha, "lora_dropout": 0.1,
           "target_modules": list(targets), "task_type": "SEQ_CLS", "modules_to_save": ["classifier", "score"],
           "peft_type": "LORA", "inference_mode": True, "bias": "none"}
    with open(os.path.join(path, ADAPTER_CONFIG), "w") as f:
        json.dump(cfg, f, indent=2)
    sd = {k: v.contiguous() for k, v in sd.items()}
    if bin_format:
        torch.save(sd, os.path.join(path, "adapter_model.bin"))
    else:
        from safetensors.torch import save_file
        save_file(sd, os.path.join(path, "adapter_model.safetensors"), metadata={"format": "pt"})
    return sd
