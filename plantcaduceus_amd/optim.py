"""AdamW with global-norm gradient clipping on this project's fused optimizer kernels (include/pcad_bwd.h pcad_adamw_step):
one step over every parameter in three launches, `zero_grad()` in one, nothing read back by the host.

    opt = AdamW(model.named_parameters(), lr=5e-5, weight_decay=0.01, max_grad_norm=1.0)
    loss.backward(); opt.step(lr=schedule(t)); opt.zero_grad()
    opt.state()          # {"norm", "coef", "finite", "skipped"} of the last step - synchronises: for logging only

The arithmetic is torch.optim.AdamW's after torch.nn.utils.clip_grad_norm_(max_grad_norm) of grad_scale * grad, in fp32.  bf16
parameters get an fp32 master copy here and are its round-to-nearest-even image after every step.  A step whose gradient norm is not
finite changes nothing and is counted (`skipped`); the step number - and with it the bias corrections and the caller's schedule - still
advances.  There is no CPU path."""
from __future__ import annotations

from typing import Dict, Iterable, List, Optional, Tuple, Union

import torch

from . import ops


def applies_weight_decay(name: str, param: Optional[torch.Tensor] = None) -> bool:
    """The decay flag of a parameter by its name in the module tree: off for biases (`*.bias`), for every RMSNorm weight (the blocks'
    `norm.weight` and `norm_f.weight`), and for `A_log` and `D`, which Mamba marks `_no_weight_decay` (the attribute is honoured too)."""
    if param is not None and getattr(param, "_no_weight_decay", False):
        return False
    leaf = name.rsplit(".", 1)[-1]
    if leaf == "bias" or leaf in ("A_log", "D"):
        return False
    if leaf == "weight" and name.rsplit(".", 2)[-2:-1] in (["norm"], ["norm_f"]):
        return False
    return True


class AdamW:
    """params: an iterable of Parameters, or of (name, Parameter) pairs such as `module.named_parameters()` - then the decay flags follow
    `applies_weight_decay`; without names weight decay applies to every tensor not marked `_no_weight_decay`.  A Parameter is taken
    once, so tied weights (one Parameter under several names) are one tensor.  Parameters that do not require grad are left out.
    grad_scale multiplies every gradient before the norm is taken (1 / accumulation steps for summed micro-batch gradients);
    max_grad_norm <= 0: no clipping.
    reducer: a `ddp.GradReducer` for data-parallel training, or None.  With one, `step()` gathers every gradient into the
    reducer's fp32 buffer in one launch, sums that buffer over the ranks, and takes the step on a second table of the same parameters,
    masters and moments whose gradients are the buffer's slices - so the norm, the clipping and the skip rule see the reduced gradients
    and are the same on every rank.  Without one the class makes exactly the calls it always made.
    fp32_grad_accumulation: the gradients live in one fp32 buffer in `ops.grads_flat_plan`'s layout (the reducer's own
    when there is one), every parameter gets its slice as `p.main_grad`, `ops.linear_fn` adds the projections' weight gradients to the
    slices unrounded, and a post-accumulate-grad hook adds every other parameter's `.grad` and drops it.  `step()` is the collective (with
    a reducer) and `adamw_step` on the table of the slices - no gather launch; `zero_grad()` zeroes the slices.  False: nothing changes."""

    def __init__(self, params: Iterable[Union[torch.nn.Parameter, Tuple[str, torch.nn.Parameter]]], lr: float = 5e-5,
                 betas: Tuple[float, float] = (0.9, 0.999), eps: float = 1e-8, weight_decay: float = 0.0, max_grad_norm: float = 1.0,
                 grad_scale: float = 1.0, reducer=None, fp32_grad_accumulation: bool = False):
        self.lr, self.betas, self.eps, self.weight_decay = float(lr), (float(betas[0]), float(betas[1])), float(eps), float(weight_decay)
        self.max_grad_norm, self.grad_scale = float(max_grad_norm), float(grad_scale)
        self.names: List[str] = []
        self.params: List[torch.nn.Parameter] = []
        self.decay: List[bool] = []
        seen = set()
        for i, item in enumerate(params):
            name, p = item if isinstance(item, tuple) else (None, item)
            if id(p) in seen or not p.requires_grad:
                continue
            seen.add(id(p))
            if not p.is_cuda:
                raise RuntimeError(f"parameter {name or i} must live on a ROCm device (got {p.device}); the optimizer has no CPU path")
            if p.dtype not in (torch.float32, torch.bfloat16) or not p.is_contiguous():
                raise ValueError(f"parameter {name or i}: a contiguous bf16 or fp32 tensor is required (got {p.dtype})")
            self.names.append(name if name is not None else str(i))
            self.params.append(p)
            self.decay.append(applies_weight_decay(name, p) if name is not None else not getattr(p, "_no_weight_decay", False))
        if not self.params:
            raise ValueError("no parameter requires grad")
        with torch.no_grad():
            self.master = [p.detach().float().clone() if p.dtype == torch.bfloat16 else None for p in self.params]
            self.exp_avg = [torch.zeros(p.shape, dtype=torch.float32, device=p.device) for p in self.params]
            self.exp_avg_sq = [torch.zeros(p.shape, dtype=torch.float32, device=p.device) for p in self.params]
        self._state = torch.zeros(4, dtype=torch.int32, device=self.params[0].device)      # pcad_optim_state: outlives every table
        self._table: Optional[ops.OptimTable] = None
        self._pointers = None
        self.reducer = reducer
        self._flat_table: Optional[ops.OptimTable] = None
        self.step_count = 0
        self.fp32_grad_accumulation = bool(fp32_grad_accumulation)
        self.main_grads: Optional[List[torch.Tensor]] = None
        if self.fp32_grad_accumulation:
            self._init_main_grads()
        elif reducer is not None:
            self.table()                                         # the buffer exists from here on: a trainer writes its loss slot before step()

    def _init_main_grads(self):
        """fp32 main gradients: one flat fp32 buffer in `ops.grads_flat_plan`'s layout - the reducer's own when there is
        one - whose slices become `p.main_grad`.  `ops.linear_fn` adds the projections' weight gradients to them in the backward; every
        other parameter's `.grad` is added by a post-accumulate-grad hook and dropped.  The only table is the one on the slices."""
        dev = self.params[0].device
        # the plan compares pointers and never reads them: the parameter stands in for a gradient that does not exist
        records = [(p.data_ptr() or None, p.data_ptr() or None, m.data_ptr() if m is not None and m.numel() else None, a.data_ptr() or None,
                    v.data_ptr() or None, p.numel(), ops._dt(p), ops._dt(a), ops.OPTIM_DECAY if d else 0)
                   for p, m, a, v, d in zip(self.params, self.master, self.exp_avg, self.exp_avg_sq, self.decay)]
        offsets, total = ops.grads_flat_plan(records)
        if self.reducer is not None:
            self.reducer.allocate(total)
            self.flat = self.reducer.grads
        else:
            self.flat = torch.zeros(total, dtype=torch.float32, device=dev)
        self.main_grads = [self.flat[o:o + p.numel()].view(p.shape) for o, p in zip(offsets, self.params)]

        def fold(p):
            if p.grad is None:                                   # a projection routed through ops.linear_fn: autograd was handed None
                return
            p.main_grad.add_(p.grad)                             # type promotion: the bf16 gradient is widened, the sum is fp32
            p.grad = None

        self._hooks = []
        for p, g in zip(self.params, self.main_grads):
            p.main_grad = g
            self._hooks.append(p.register_post_accumulate_grad_hook(fold))
        self._main_table()

    def _main_table(self) -> ops.OptimTable:
        now = tuple(p.data_ptr() for p in self.params)
        if self._table is None or now != self._pointers:
            self._table = ops.OptimTable([p.data for p in self.params], self.main_grads, self.master, self.exp_avg, self.exp_avg_sq,
                                         self.decay, state=self._state)
            self._pointers = now
        return self._table

    def table(self) -> ops.OptimTable:
        """The device table, rebuilt and uploaded again (on the stream, without synchronising) only when a pointer in it has changed.  A
        parameter that has no gradient yet gets a zero one: every tensor of the set takes part in every step.  The per-step check is two
        data_ptr() calls per tensor and nothing else, so that the host stays ahead of the device.  With fp32_grad_accumulation the
        gradients are the main gradients' slices and no `.grad` is created."""
        if self.fp32_grad_accumulation:
            return self._main_table()
        grads = [p.grad for p in self.params]
        now = None
        if not any(g is None for g in grads):
            now = (tuple(p.data_ptr() for p in self.params), tuple(g.data_ptr() for g in grads))
        if self._table is None or now is None or now != self._pointers:
            for p in self.params:
                if p.grad is None:
                    p.grad = torch.zeros_like(p, memory_format=torch.contiguous_format)
                elif not p.grad.is_contiguous():
                    p.grad = p.grad.contiguous()
            grads = [p.grad for p in self.params]
            self._table = ops.OptimTable([p.data for p in self.params], grads, self.master, self.exp_avg, self.exp_avg_sq, self.decay,
                                         state=self._state)
            self._pointers = (tuple(p.data_ptr() for p in self.params), tuple(g.data_ptr() for g in grads))
            if self.reducer is not None:
                self.reducer.allocate(self._table.flat_plan()[1])
                self._flat_table = self._table.on_flat(self.reducer.grads)
        return self._table

    def step(self, lr: Optional[float] = None):
        """One step at learning rate `lr` (default: the constructor's).  No host synchronisation (a gloo reducer: one, in its collective)."""
        self.step_count += 1
        table = self.table()
        if self.fp32_grad_accumulation:
            # the main gradients already are the collective's operand: no gather launch, and the table is the one on the slices
            if self.reducer is not None:
                self.reducer.all_reduce()
        elif self.reducer is not None:
            ops.grads_gather(table, self.reducer.grads, table.flat_offsets())
            self.reducer.all_reduce()
            table = self._flat_table
        ops.adamw_step(table, self.lr if lr is None else float(lr), self.betas[0], self.betas[1], self.eps, self.weight_decay,
                       self.step_count, self.max_grad_norm, self.grad_scale)

    def zero_grad(self):
        """Every gradient set to zero in one launch; the storage stays, so the table stays.  With fp32_grad_accumulation the gradients
        are the main gradients' slices: all their elements and nothing beyond them - the padding was zeroed once, the reducer's tail is
        the trainer's."""
        ops.zero_grads(self.table())

    def state(self) -> Dict[str, float]:
        """norm (of grad_scale * grad), coef (the factor applied to the gradients), finite and skipped of the last step.  Synchronises."""
        return (self._table or self.table()).read_state()

    def state_dict(self) -> dict:
        """master weights (fp32 parameters: the parameter itself), both moments, the step count and the skipped count, on the CPU."""
        cpu = lambda t: t.detach().cpu().clone()
        return {"step": self.step_count, "skipped": self.state()["skipped"], "names": list(self.names),
                "master": [cpu(m if m is not None else p) for m, p in zip(self.master, self.params)],
                "exp_avg": [cpu(t) for t in self.exp_avg], "exp_avg_sq": [cpu(t) for t in self.exp_avg_sq]}

    def load_state_dict(self, sd: dict):
        if list(sd["names"]) != self.names:
            raise ValueError("the optimizer state was saved for another parameter set")
        with torch.no_grad():
            for i, p in enumerate(self.params):
                if tuple(sd["master"][i].shape) != tuple(p.shape):
                    raise ValueError(f"{self.names[i]}: saved shape {tuple(sd['master'][i].shape)}, parameter {tuple(p.shape)}")
                if self.master[i] is not None:
                    self.master[i].copy_(sd["master"][i])
                    p.copy_(self.master[i])                  # the bf16 parameter is the rounded master
                else:
                    p.copy_(sd["master"][i])
                self.exp_avg[i].copy_(sd["exp_avg"][i])
                self.exp_avg_sq[i].copy_(sd["exp_avg_sq"][i])
            self._state.copy_(torch.tensor([0, 0, 1, int(sd.get("skipped", 0))], dtype=torch.int32))
        self.step_count = int(sd["step"])
