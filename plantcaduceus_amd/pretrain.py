"""Masked-LM pretraining: the `--do_train` half of the reference's `src/HF_pre_train.py` (:446-501: `Trainer.train()`, `save_model`,
`save_metrics("train")`, `save_state`) on this project's kernels - forward and backward of `training.TrainableCaduceusForMaskedLM`,
the fused AdamW step of `optim.AdamW`.  One process and one GPU under plain `python`; data-parallel over the GPUs
of a node under `torchrun` (below).

    python -m plantcaduceus_amd.pretrain --model_name_or_path <snapshot> | --config_name <config.json> \\
        --dataset_name <dir or table> --do_train [--do_eval] --output_dir out \\
        --per_device_train_batch_size 8 --gradient_accumulation_steps 1 --learning_rate 5e-5 --weight_decay 0.0 \\
        --adam_beta1 0.9 --adam_beta2 0.999 --adam_epsilon 1e-8 --max_grad_norm 1.0 \\
        --num_train_epochs 3 | --max_steps N  --lr_scheduler_type linear|cosine|constant|constant_with_warmup \\
        --warmup_steps K | --warmup_ratio R  --mlm_probability 0.15 --soft_masked_loss_weights_train 1.0 \\
        --logging_steps 500 --save_steps 500 --seed 42 --resume_from_checkpoint <dir> --dtype float32|bfloat16 \\
        [--gradient_checkpointing] [--fp32_grad_accumulation] [--scan_bwd_segments N|auto] [--scan_fwd_segments N|auto] \\
        [--ddp_backend nccl|gloo] \\
        [--eval_strategy no|steps|epoch --eval_steps N --per_device_eval_batch_size 8 --max_eval_samples M] \\
        [--save_strategy steps|epoch|no --save_total_limit K --load_best_model_at_end --metric_for_best_model loss]
    torchrun --nproc-per-node W -m plantcaduceus_amd.pretrain ... (the same flags)

Flag names and defaults are `transformers.TrainingArguments`' and `HF_pre_train.py`'s.  `--config_name` alone starts from scratch:
`checkpoint.synthetic_state_dict(config, seed=--seed, stress=False)`, the Mamba-style initialisation.

Data is `mlm_eval`'s: `load_sequences(..., "train")`, `tokenize_windows` (equal-length windows only), and HF's own
`DataCollatorForLanguageModeling.torch_mask_tokens` on a CPU generator of its own, seeded with `--seed`: masks are drawn afresh for
every micro-batch.  The window order of epoch e is `torch.randperm(N)` from a generator seeded by (`--seed`, e).  An optimizer step is
`--gradient_accumulation_steps` micro-batches of `--per_device_train_batch_size` windows, each `forward(...).loss.backward()`, then
`optimizer.step(lr=schedule(t))` with `grad_scale = 1 / micro-batches` and `zero_grad()`.  An epoch has
max(1, ceil(N / batch) // accumulation) steps, as `Trainer` counts them; micro-batches beyond the last whole step of an epoch are not
used.  The learning rate of the t-th step (t = 0, 1, ...) is `learning_rate * lambda(t)` with `transformers.get_scheduler`'s lambdas
(so the first step of a warm-up runs at 0, as under `Trainer`).  The loop reads nothing back from the device except at
`--logging_steps`, `--save_steps` and the end.

Written: `output_dir/` becomes a snapshot (config.json, model.safetensors under the reference's key names, the tokenizer) that
`CaduceusForMaskedLM.from_pretrained`, `mlm_eval` and `zero_shot` load, with `train_results.json`, `all_results.json` and
`trainer_state.json`; `output_dir/checkpoint-<step>/` is such a snapshot plus `optimizer.pt` (master weights, moments, step),
`rng_state.pt` (the mask generator's state; the window order is re-derived from (`--seed`, epoch)) and `trainer_state.json` (step, epoch, log history of loss,
learning_rate, grad_norm and skipped_steps).  `--resume_from_checkpoint` continues from one, bit for bit.  `--do_eval` runs
`mlm_eval.evaluate_split` on the saved snapshot.

Departures from the reference, all stated in DESIGN.md §4o: a step whose gradient norm is not finite is skipped and counted instead
of letting NaNs into the weights; weight decay leaves out `A_log` and `D` beside biases and norm weights; `--dtype bfloat16` means
bf16 parameters and kernels with fp32 master weights in the optimizer, where the reference's `bf16=True` is autocast around fp32
parameters.  `--gradient_checkpointing` (`TrainingArguments`' name and default) keeps only each block's inputs and runs the block again in
the backward: the same bits for about an eighth of the stored activations.  `--fp32_grad_accumulation` (bf16 only) brings
the gradients back to the reference's fp32: one fp32 buffer holds them, the projections' weight gradients are added to it unrounded by
`pcad_linear_wgrad`, and micro-batches - and ranks - are summed in fp32.  Checkpoints, resume and logs are unchanged.
`--scan_bwd_segments N|auto` (or the environment variable PCAD_TRAIN_SCAN_SEGMENTS, which `lora_predict train` reads too) cuts every
strand of the selective scan's backward into segments walked in parallel - for long windows at a small batch, where one wave per
(strand, 64 channels) leaves most of the device idle.  Off by default; the forward's bits do not depend on it.
`--scan_fwd_segments N|auto` (or PCAD_TRAIN_SCAN_FWD_SEGMENTS, likewise read by `lora_predict train`) does the same for the scan's training
FORWARD: its own setting, which neither the backward's flag nor its variable turns on.  Off by default: no bit changes; on,
the scans' outputs differ by fp32 rounding and a run is reproducible for a given value.

Under `torchrun` with world size W an optimizer step consumes the `--gradient_accumulation_steps` x W micro-batches that
one process with that accumulation would consume, in the same window order and with the same masks: every rank draws all of them (the
mask generator advances identically everywhere), rank r runs those with index j = r (mod W), one collective sums the gradients of all
ranks in fp32, and `grad_scale` = 1 / (micro-batches of the step over all ranks) is applied after the sum.  `steps_per_epoch`, the
schedule and `trainer_state.json` are those of that single process, so a checkpoint written at one world size resumes at another with
accumulation x world kept equal; at W = 2 and accumulation 1 in fp32 the run equals the single-process run with accumulation 2 bit for
bit.  `--ddp_backend` (`TrainingArguments`' name; the environment's PCAD_DDP_BACKEND when absent; default nccl): nccl is RCCL, one rank
per device, no host wait; gloo stages the buffer through pinned host memory with one stream synchronisation per step and lets ranks
share a device.  Rank 0 alone logs and writes; every checkpoint and the end compare a checksum of the master weights over the ranks.
`--do_eval` runs on rank 0 after the group is shut down.

Evaluation during the run.  `--eval_strategy steps|epoch` (`--evaluation_strategy` is the same option) evaluates at
step % `--eval_steps` == 0 (`--logging_steps` when absent) or at whole epochs, after the step's log entry and before its checkpoint -
`Trainer._maybe_log_save_evaluate`'s order, so a checkpoint written at an evaluated step holds that evaluation.  The validation split is
loaded once before the first step, cut to `--max_eval_samples`, tokenized with `--soft_masked_loss_weights_evaluation`, and its masks
are drawn ONCE, per loss batch of `--per_device_eval_batch_size`, on a private generator seeded with `--seed`: the masks
`mlm_eval.evaluate_split(seed=--seed)` draws; every evaluation of a run sees the same ones (HF's collator redraws them each time) and
neither the training masks nor torch's global generator are touched.  One evaluation is `evaluate_model`: the training model itself under
torch.no_grad(), one forward per loss batch, the [N, 4] per-window sums through `mlm_eval.metrics_from_sums` - `eval_loss` (the mean of
batch losses, as `Trainer.evaluation_loop` forms it), `perplexity`, `eval_token_accuracy`, `eval_loss_token_mean`, `eval_samples`,
`eval_labelled_tokens`, plus `eval_runtime`, `eval_samples_per_second`, `eval_steps_per_second`, `step`, `epoch` in the log history.
Under `torchrun` the loss batches are dealt to the ranks in contiguous blocks (`sharding.batch_block`) and one gather hands every rank
all rows: every forward sees the rows it sees in one process, so the entries are the same bits at any world size.
`trainer_state.json` carries `best_metric`, `best_global_step`, `best_model_checkpoint`: the lowest `eval_loss` among evaluations at
steps where a checkpoint was written (nan never).  `--save_total_limit N` keeps the newest N checkpoints (`rotate_checkpoints`,
`Trainer._rotate_checkpoints`' rule); `--load_best_model_at_end` (the same eval and save strategy; `--save_steps` a multiple of
`--eval_steps`) protects the best checkpoint from rotation and ends with its weights in `output_dir`.  `--metric_for_best_model` takes
loss / eval_loss only; `--prediction_loss_only` is accepted; `--dataloader_num_workers`, `--preprocessing_num_workers`,
`--remove_unused_columns`, `--overwrite_output_dir`, `--run_name`, `--optim adamw_torch` and `--report_to none` are accepted and ignored."""
from __future__ import annotations

import json
import logging
import math
import os
import time
from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

logger = logging.getLogger(__name__)

SCHEDULES = ("linear", "cosine", "constant", "constant_with_warmup")
SCAN_SEGMENTS_ENV = "PCAD_TRAIN_SCAN_SEGMENTS"
SCAN_FWD_SEGMENTS_ENV = "PCAD_TRAIN_SCAN_FWD_SEGMENTS"


def lr_lambda(kind: str, step: int, warmup: int, total: int) -> float:
    """`transformers.get_scheduler(kind, ..., num_warmup_steps=warmup, num_training_steps=total)`'s multiplier after `step` scheduler steps"""
    if kind == "constant":
        return 1.0
    if step < warmup:
        return float(step) / float(max(1, warmup))
    if kind == "constant_with_warmup":
        return 1.0
    if kind == "linear":
        return max(0.0, float(total - step) / float(max(1, total - warmup)))
    if kind == "cosine":
        progress = float(step - warmup) / float(max(1, total - warmup))
        return max(0.0, 0.5 * (1.0 + math.cos(math.pi * 0.5 * 2.0 * progress)))
    raise ValueError(f"unknown --lr_scheduler_type {kind!r} (one of {', '.join(SCHEDULES)})")


def warmup_steps_of(warmup_steps: int, warmup_ratio: float, total: int) -> int:
    """`TrainingArguments.get_warmup_steps`"""
    return int(warmup_steps) if warmup_steps > 0 else math.ceil(total * warmup_ratio)


def steps_per_epoch(n_windows: int, batch: int, accumulation: int) -> int:
    return max(1, math.ceil(n_windows / batch) // accumulation)


class WindowOrder:
    """Which windows make up each micro-batch of every optimizer step, a function of (seed, n, batch, accumulation): the order of
    epoch e is `torch.randperm(n)` from a generator seeded by (seed, e).  Shared with `lora_predict train`."""

    def __init__(self, n: int, batch: int, accumulation: int, seed: int):
        self.n, self.batch, self.accumulation, self.seed = int(n), int(batch), int(accumulation), int(seed)
        if self.n == 0:
            raise ValueError("no training windows")
        self.steps_per_epoch = steps_per_epoch(self.n, self.batch, self.accumulation)
        self.order_generator = torch.Generator()
        self._epoch, self._order = None, None

    def order(self, epoch: int) -> torch.Tensor:
        if self._epoch != epoch:
            self.order_generator.manual_seed(self.seed * 1000003 + epoch)
            self._epoch, self._order = epoch, torch.randperm(self.n, generator=self.order_generator)
        return self._order

    def windows(self, step: int) -> List[np.ndarray]:
        """the window indices of each micro-batch of optimizer step `step` (0-based)"""
        epoch, s = divmod(step, self.steps_per_epoch)
        order = self.order(epoch).numpy()
        out = []
        for j in range(self.accumulation):
            lo = (s * self.accumulation + j) * self.batch
            if lo < self.n:
                out.append(order[lo:lo + self.batch])
        return out


class BatchSource(WindowOrder):
    """The micro-batches of every optimizer step, a function of (seed, data, batch, accumulation) and of how many micro-batches were
    drawn before: window order from a generator seeded by (seed, epoch), masks from the collator on a CPU generator of its own."""

    def __init__(self, ids: np.ndarray, special: np.ndarray, weights: np.ndarray, collator, batch: int, accumulation: int, seed: int):
        super().__init__(ids.shape[0], batch, accumulation, seed)
        self.ids, self.special, self.weights, self.collator = ids, special, weights, collator
        self.mask_generator = torch.Generator().manual_seed(self.seed)
        self.collator.generator = self.mask_generator

    def step_batches(self, step: int):
        """-> [(masked input_ids int32 [b, L], labels int32 [b, L], loss_weights fp32 [b, L])] CPU tensors; advances the mask generator"""
        out = []
        for idx in self.windows(step):
            x, y = self.collator.torch_mask_tokens(torch.from_numpy(self.ids[idx].copy()), special_tokens_mask=torch.from_numpy(self.special[idx].copy()))
            out.append((x.to(torch.int32), y.to(torch.int32), torch.from_numpy(self.weights[idx].copy())))
        return out

    def state(self) -> dict:
        """what a resume cannot re-derive: the mask generator's state (the order is a function of (seed, epoch))"""
        return {"mask_generator": self.mask_generator.get_state()}

    def load_state(self, st: dict):
        self.mask_generator.set_state(st["mask_generator"])


# ---------------------------------------------------------------------------------------------------------------------
# when to evaluate and to save; which checkpoints stay; which one is the best
STRATEGIES = ("no", "steps", "epoch")


def interval(strategy: str, steps: int, per_epoch: int, flag: str) -> int:
    """every how many optimizer steps a `--<flag>` of no / steps / epoch is due; 0: never"""
    if strategy == "no":
        return 0
    if strategy == "steps":
        return max(0, int(steps))
    if strategy == "epoch":
        return int(per_epoch)
    raise SystemExit(f"--{flag} must be one of {', '.join(STRATEGIES)} (got {strategy!r})")


def eval_interval(a, per_epoch: int) -> int:
    """`--eval_strategy` with `--eval_steps`, which follows `--logging_steps` when it is not given (`TrainingArguments.__post_init__`)"""
    steps = getattr(a, "eval_steps", None)
    return interval(getattr(a, "eval_strategy", "no"), a.logging_steps if steps is None else steps, per_epoch, "eval_strategy")


def save_interval(a, per_epoch: int) -> int:
    """`--save_strategy` with `--save_steps`; `--save_steps 0` writes no checkpoint"""
    return interval(getattr(a, "save_strategy", "steps"), a.save_steps, per_epoch, "save_strategy")


def due_steps(every: int, last: int) -> List[int]:
    """the steps in 1 .. last at which something due every `every` steps happens"""
    return [s for s in range(1, last + 1) if every and s % every == 0]


def checkpoint_dirs(output_dir: str) -> List[str]:
    """output_dir's `checkpoint-<n>` directories, oldest step first"""
    if not os.path.isdir(output_dir):
        return []
    found = sorted((int(d.split("-", 1)[1]), d) for d in os.listdir(output_dir)
                   if d.startswith("checkpoint-") and d.split("-", 1)[1].isdigit() and os.path.isdir(os.path.join(output_dir, d)))
    return [os.path.join(output_dir, d) for _, d in found]


def rotate_checkpoints(output_dir: str, limit: Optional[int], best: Optional[str] = None) -> List[str]:
    """`Trainer._rotate_checkpoints`: keep the newest `limit` checkpoints of output_dir and delete the older ones -> the deleted paths.
    `best` (a checkpoint path, or None) is never deleted and counts towards the limit: it takes the place next to the newest one.  With a
    limit of 1 and a best checkpoint that is not the newest both stay, so that the run can still be resumed.  limit None or < 1: keep all."""
    import shutil
    if limit is None or int(limit) < 1:
        return []
    kept = checkpoint_dirs(output_dir)
    limit = int(limit)
    same = [os.path.abspath(k) for k in kept]
    if best is not None and os.path.abspath(best) in same:
        at = same.index(os.path.abspath(best))
        kept.insert(max(at, len(kept) - 2), kept.pop(at))
        if limit == 1 and os.path.abspath(kept[-1]) != os.path.abspath(best):
            limit = 2
    gone = kept[:max(0, len(kept) - limit)]
    for d in gone:
        shutil.rmtree(d)
    return gone


class BestCheckpoint:
    """HF's `best_metric`, `best_global_step` and `best_model_checkpoint`.  The metric is `eval_loss`, lower is better, and only an
    evaluation at a step where a checkpoint is written is offered: the three fields always name one checkpoint.  nan is never the best."""

    def __init__(self):
        self.metric, self.step, self.path = None, 0, None

    def offer(self, loss: float, step: int, path: str) -> bool:
        loss = float(loss)
        if math.isnan(loss) or (self.metric is not None and not loss < self.metric):
            return False
        self.metric, self.step, self.path = loss, int(step), path
        return True

    def state(self) -> dict:
        return {"best_metric": self.metric, "best_global_step": self.step, "best_model_checkpoint": self.path}

    def load_state(self, ts: dict):
        self.metric, self.step, self.path = ts.get("best_metric"), int(ts.get("best_global_step") or 0), ts.get("best_model_checkpoint")


# ---------------------------------------------------------------------------------------------------------------------
# the validation set and one evaluation of the training model on it
class ValidationSet:
    """The validation windows as every evaluation of a run sees them: masked input_ids int32 [N, L], labels int32 [N, L] (-100 off the
    masked set), loss_weights fp32 [N, L] and the loss batch size.  `build` draws the masks ONCE, per loss batch in dataset order as
    `mlm_eval.mask_windows` does, on a generator of its own seeded with `seed`: the masks `mlm_eval.evaluate_split(seed=seed)` draws, and
    torch's global generator is left alone."""

    def __init__(self, ids: np.ndarray, labels: np.ndarray, weights: np.ndarray, batch_size: int):
        self.ids, self.labels, self.weights, self.batch_size = ids, labels, weights, max(1, int(batch_size))
        self.n = int(ids.shape[0])

    @classmethod
    def build(cls, tokenizer, seqs: Sequence[str], soft_masked_weight: float = 1.0, mlm_probability: float = 0.15, batch_size: int = 8,
              seed: int = 42, max_samples: Optional[int] = None) -> "ValidationSet":
        from . import mlm_eval
        if max_samples is not None:
            seqs = list(seqs)[:max(0, int(max_samples))]
        ids, special, weights = mlm_eval.tokenize_windows(tokenizer, seqs, soft_masked_weight)
        collator = mlm_eval.make_collator(tokenizer, mlm_probability)
        collator.generator = torch.Generator().manual_seed(int(seed))
        masked, labels = mlm_eval.mask_windows(collator, ids, special, max(1, int(batch_size)))
        return cls(masked, labels, weights, batch_size)


def evaluate_model(model, valid: ValidationSet, device) -> np.ndarray:
    """The training model's per-window sums fp32 [N, 4] (sum w nll, sum w, labelled positions, arg-max hits) on `valid`, in window
    order: one forward per loss batch under torch.no_grad() - the fused inference kernels and the fused loss head; no file, no copy of
    the weights.  In a process group the loss batches are dealt to the ranks in contiguous blocks (`sharding.batch_block`) and one
    gather hands every rank all rows; `mlm_eval.metrics_from_sums(sums, valid.batch_size, "eval")` is the host arithmetic on them."""
    from . import sharding
    t_ids, t_lab, t_w = (torch.from_numpy(np.ascontiguousarray(x)) for x in (valid.ids, valid.labels, valid.weights))

    def run_batch(lo, hi):
        return model(t_ids[lo:hi].to(device), t_lab[lo:hi].to(device), t_w[lo:hi].to(device)).sums

    with torch.no_grad():
        sums = sharding.gather_batch_rows(valid.n, valid.batch_size, run_batch, 4, device)
    return sums.cpu().numpy()


# ---------------------------------------------------------------------------------------------------------------------
def _bool(v) -> bool:
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("1", "true", "yes", "y"):
        return True
    if str(v).lower() in ("0", "false", "no", "n"):
        return False
    raise ValueError(f"not a boolean: {v!r}")


# TrainingArguments / HF_pre_train.py flags that have nothing to do here: accepted, named in one INFO line, ignored
IGNORED_FLAGS = ("dataloader_num_workers", "preprocessing_num_workers", "remove_unused_columns", "overwrite_output_dir", "run_name", "optim",
                 "report_to")


def check_args(a):
    """what argparse's types and choices do not say; every refusal names its flag.  -> a, with --eval_steps an int or None"""
    if a.eval_steps is not None and not isinstance(a.eval_steps, int):
        try:
            val = float(a.eval_steps)
        except ValueError:
            val = 0.0
        if val < 1 or val != int(val):
            raise SystemExit(f"--eval_steps must be an integer >= 1 (got {a.eval_steps!r}; a ratio of the run's steps is not supported)")
        a.eval_steps = int(val)
    if a.metric_for_best_model not in (None, "loss", "eval_loss"):
        raise SystemExit(f"--metric_for_best_model {a.metric_for_best_model}: only loss and eval_loss are accepted, the evaluation here is the loss")
    if a.optim not in (None, "adamw_torch"):
        raise SystemExit(f"--optim {a.optim}: only adamw_torch is accepted (the step is optim.AdamW's fused kernel, DESIGN.md §4o)")
    if a.report_to not in (None, "none"):
        raise SystemExit(f"--report_to {a.report_to} is not supported: the log history is written to trainer_state.json; only none is accepted")
    if a.save_total_limit is not None and a.save_total_limit < 1:
        raise SystemExit(f"--save_total_limit must be >= 1 (got {a.save_total_limit})")
    if a.load_best_model_at_end:
        every = a.logging_steps if a.eval_steps is None else a.eval_steps
        if a.eval_strategy != "epoch" and a.save_strategy == "steps" and (a.save_steps < 1 or every < 1 or a.save_steps % every != 0):
            raise SystemExit(f"--load_best_model_at_end needs --save_steps ({a.save_steps}) to be a round multiple of --eval_steps ({every}): "
                             "the best checkpoint is chosen among evaluated steps at which a checkpoint was written")
        if a.eval_strategy == "no":
            raise SystemExit("--load_best_model_at_end needs an evaluation: pass --eval_strategy steps or epoch")
        if a.save_strategy != a.eval_strategy:
            raise SystemExit(f"--load_best_model_at_end needs --save_strategy ({a.save_strategy}) to be the same as --eval_strategy ({a.eval_strategy})")
    return a


def build_parser():
    import argparse

    class Parser(argparse.ArgumentParser):
        def parse_args(self, args=None, namespace=None):
            return check_args(super().parse_args(args, namespace))

    p = Parser(prog="pretrain", description="Masked-LM pretraining on the MI355X kernels (src/HF_pre_train.py --do_train)")
    p.add_argument("--model_name_or_path", default=None)
    p.add_argument("--config_name", default=None)
    p.add_argument("--tokenizer_name", default=None)
    p.add_argument("--dataset_name", required=True)
    p.add_argument("--dataset_config_name", default=None)
    p.add_argument("--do_train", action="store_true")
    p.add_argument("--do_eval", action="store_true")
    p.add_argument("--output_dir", required=True)
    p.add_argument("--per_device_train_batch_size", type=int, default=8)
    p.add_argument("--per_device_eval_batch_size", type=int, default=8)
    p.add_argument("--gradient_accumulation_steps", type=int, default=1)
    p.add_argument("--learning_rate", type=float, default=5e-5)
    p.add_argument("--weight_decay", type=float, default=0.0)
    p.add_argument("--adam_beta1", type=float, default=0.9)
    p.add_argument("--adam_beta2", type=float, default=0.999)
    p.add_argument("--adam_epsilon", type=float, default=1e-8)
    p.add_argument("--max_grad_norm", type=float, default=1.0)
    p.add_argument("--num_train_epochs", type=float, default=3.0)
    p.add_argument("--max_steps", type=int, default=-1)
    p.add_argument("--lr_scheduler_type", default="linear", choices=SCHEDULES)
    p.add_argument("--warmup_steps", type=int, default=0)
    p.add_argument("--warmup_ratio", type=float, default=0.0)
    p.add_argument("--mlm_probability", type=float, default=0.15)
    p.add_argument("--soft_masked_loss_weights_train", type=float, default=1.0)
    p.add_argument("--soft_masked_loss_weights_evaluation", type=float, default=1.0)
    p.add_argument("--max_train_samples", type=int, default=None)
    p.add_argument("--max_eval_samples", type=int, default=None)
    p.add_argument("--logging_steps", type=int, default=500)
    p.add_argument("--save_steps", type=int, default=500)
    p.add_argument("--eval_strategy", "--evaluation_strategy", dest="eval_strategy", default="no", choices=STRATEGIES,
                   help="evaluate the training model on the validation split during the run (DESIGN.md §4t); --evaluation_strategy is "
                        "transformers 4.40's spelling of the same option")
    p.add_argument("--eval_steps", default=None, help="with --eval_strategy steps; an integer >= 1; --logging_steps when absent")
    p.add_argument("--save_strategy", default="steps", choices=STRATEGIES, help="--save_steps 0 still means no checkpoints")
    p.add_argument("--save_total_limit", type=int, default=None, help="keep the newest N checkpoints; all of them when absent")
    p.add_argument("--load_best_model_at_end", type=_bool, nargs="?", const=True, default=False,
                   help="end with the checkpoint of the lowest eval_loss in output_dir; needs the same eval and save strategy")
    p.add_argument("--metric_for_best_model", default=None, help="loss or eval_loss (the default)")
    p.add_argument("--prediction_loss_only", type=_bool, nargs="?", const=True, default=False, help="accepted: the evaluation is the loss")
    for name in IGNORED_FLAGS:
        kind = {"dataloader_num_workers": int, "preprocessing_num_workers": int, "remove_unused_columns": _bool, "overwrite_output_dir": _bool}.get(name, str)
        p.add_argument("--" + name, type=kind, default=None, **({"nargs": "?", "const": True} if kind is _bool else {}),
                       help="accepted and ignored")
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--resume_from_checkpoint", default=None)
    p.add_argument("--gradient_checkpointing", action="store_true",
                   help="keep only each block's inputs and run its forward again in the backward (DESIGN.md §4q): same bits, less memory")
    p.add_argument("--fp32_grad_accumulation", action="store_true",
                   help="with --dtype bfloat16: keep the gradients in one fp32 buffer; the projections' weight gradients are added to it "
                        "unrounded by the weight-gradient MFMA kernel, so micro-batches are summed in fp32 (DESIGN.md §4s)")
    p.add_argument("--scan_bwd_segments", default=None,
                   help="segments per strand of the selective scan's backward: 1 (off), 2..64 or auto (DESIGN.md §4v); the "
                        f"environment's {SCAN_SEGMENTS_ENV} when absent")
    p.add_argument("--scan_fwd_segments", default=None,
                   help="segments per strand of the selective scan's training forward: 1 (off), 2..64 or auto (DESIGN.md §4w); the "
                        f"environment's {SCAN_FWD_SEGMENTS_ENV} when absent")
    p.add_argument("--ddp_backend", default=None, choices=("nccl", "gloo"),
                   help="under torchrun: nccl (RCCL, one rank per device; the default) or gloo (ranks may share a device; one host "
                        "synchronisation per step); the environment's PCAD_DDP_BACKEND when absent (DESIGN.md §4r)")
    p.add_argument("--dtype", default="float32", choices=("float32", "bfloat16"))
    p.add_argument("--device", default="cuda:0")
    return p


def scan_segments_from_env(env=None, name=SCAN_SEGMENTS_ENV):
    """The segments of the selective scan's backward from the environment variable PCAD_TRAIN_SCAN_SEGMENTS (`env`: a
    mapping, os.environ when None; a bare value is taken too): unset, empty or `1` -> 1 (off); `2`..`64` -> that many; `auto` -> "auto"
    (ops.scan_bwd_auto_segments per call).  Anything else exits naming the variable.  name: the variable to read instead -
    SCAN_FWD_SEGMENTS_ENV for the forward's segments, which are a setting of their own."""
    val = env if isinstance(env, str) else (os.environ if env is None else env).get(name, "")
    val = str(val).strip().lower()
    if not val:
        return 1
    if val == "auto":
        return "auto"
    if val.isdigit() and 1 <= int(val) <= 64:
        return int(val)
    raise SystemExit(f"{name} must be 1 (off), 2..64 or auto, got {val!r}")


def load_tokenizer(a):
    from .checkpoint import resolve_snapshot
    src = a.tokenizer_name or a.model_name_or_path
    if src:
        from transformers import AutoTokenizer
        from . import register
        register()
        return AutoTokenizer.from_pretrained(resolve_snapshot(src))
    from .tokenization_caduceus import CaduceusTokenizer
    return CaduceusTokenizer()


def build_model(a, dtype: torch.dtype, source: Optional[str] = None):
    """the trainable model from `source` (a checkpoint to resume), else --model_name_or_path, else --config_name from scratch"""
    from .checkpoint import synthetic_state_dict
    from .configuration_caduceus import config_from_dict
    from .training import TrainableCaduceusForMaskedLM
    path = source or a.model_name_or_path
    recompute = bool(getattr(a, "gradient_checkpointing", False))
    flag = getattr(a, "scan_bwd_segments", None)
    segments = scan_segments_from_env(os.environ if flag is None else str(flag))
    logger.info("Segments of the scan's backward (--scan_bwd_segments / %s): %s", SCAN_SEGMENTS_ENV, "off" if segments == 1 else segments)
    fwd_flag = getattr(a, "scan_fwd_segments", None)
    fwd_segments = scan_segments_from_env(os.environ if fwd_flag is None else str(fwd_flag), SCAN_FWD_SEGMENTS_ENV)
    logger.info("Segments of the scan's forward (--scan_fwd_segments / %s): %s", SCAN_FWD_SEGMENTS_ENV,
                "off" if fwd_segments == 1 else fwd_segments)
    if path:
        return TrainableCaduceusForMaskedLM.from_pretrained(path, dtype=dtype, device=a.device, gradient_checkpointing=recompute,
                                                            scan_bwd_segments=segments, scan_fwd_segments=fwd_segments)
    if not a.config_name:
        raise SystemExit("pass --model_name_or_path or --config_name")
    cfg_path = os.path.join(a.config_name, "config.json") if os.path.isdir(a.config_name) else a.config_name
    with open(cfg_path) as f:
        cfg = config_from_dict(json.load(f))
    model = TrainableCaduceusForMaskedLM(cfg, dtype=dtype, device=a.device, gradient_checkpointing=recompute, scan_bwd_segments=segments,
                                         scan_fwd_segments=fwd_segments)
    model.load_state_dict(synthetic_state_dict(cfg, seed=a.seed, stress=False))
    return model


def save_snapshot(model, tokenizer, path: str):
    """config.json + model.safetensors (the reference's key names, tied duplicates dropped as in a real snapshot) + the tokenizer"""
    from .checkpoint import save_checkpoint
    sd = {k: v.detach().cpu() for k, v in model.state_dict().items()}
    save_checkpoint(path, model.config, sd, with_tokenizer=False)
    tokenizer.save_pretrained(path)


def _write_json(path: str, obj):
    with open(path, "w") as f:
        json.dump(obj, f, indent=2, sort_keys=True)


class Trainer:
    """The loop around model, optimizer and batch source; `micro_step` is the only place the model runs.  rank / world: this process's
    place in a data-parallel run: `source` hands out the micro-batches of all ranks, this one runs those with index
    j = rank (mod world), and an optimizer with a `reducer` sums the gradients and the loss over the ranks; rank 0 alone logs and writes."""

    def __init__(self, model, optimizer, source: BatchSource, tokenizer, a, max_steps: int, warmup: int, rank: int = 0, world: int = 1,
                 valid: Optional[ValidationSet] = None):
        self.model, self.opt, self.source, self.tok, self.a = model, optimizer, source, tokenizer, a
        self.max_steps, self.warmup = max_steps, warmup
        self.valid, self.best = valid, BestCheckpoint()
        self.rank, self.world = int(rank), int(world)
        if self.world > 1 and getattr(optimizer, "reducer", None) is None:
            raise ValueError("a world of more than one rank needs an optimizer with a reducer (optim.AdamW(..., reducer=ddp.GradReducer(...)))")
        self.step = 0
        self.log_history: List[dict] = []
        dev = a.device
        self.window_loss = torch.zeros((), dtype=torch.float32, device=dev)     # sum of the step losses since the last log
        self.total_loss = torch.zeros((), dtype=torch.float32, device=dev)      # ... since the start
        self.window_steps = 0

    def lr(self, step: int) -> float:
        return self.a.learning_rate * lr_lambda(self.a.lr_scheduler_type, step, self.warmup, self.max_steps)

    def micro_step(self, ids, labels, weights):
        dev = self.a.device
        up = lambda t: t.pin_memory().to(dev, non_blocking=True)
        out = self.model(up(ids), up(labels), up(weights))
        out.loss.backward()
        return out.loss.detach()

    def before_micro_step(self, j: int, n: int):
        """called before micro-batch j of the step's n (the index it has in the one-process run); nothing to do here - a trainer whose
        model draws per-step randomness from a counter sets the counter (lora_predict.FinetuneTrainer)"""

    def train_step(self):
        """optimizer step number self.step (0-based): this rank's share of its micro-batches, the fused step, zero_grad; nothing is read
        back.  With a reducer the rank's sum of loss x scale travels in the reducer's loss slot and comes back as the global loss; a rank
        whose share is empty contributes zero gradients and a zero loss and still takes part in the collective."""
        from . import ddp
        batches = self.source.step_batches(self.step)           # every rank draws all of them
        scale = 1.0 / len(batches)
        self.opt.grad_scale = scale
        reducer = getattr(self.opt, "reducer", None)
        loss = None
        for j, (ids, labels, weights) in ddp.share(list(enumerate(batches)), self.rank, self.world):
            self.before_micro_step(j, len(batches))
            l = self.micro_step(ids, labels, weights).float() * scale
            loss = l if loss is None else loss + l
        if reducer is not None:
            reducer.loss.zero_() if loss is None else reducer.loss.copy_(loss.reshape(1))
        lr = self.lr(self.step)
        self.opt.step(lr=lr)
        if reducer is not None:
            loss = reducer.loss[0].clone()
        self.opt.zero_grad()
        self.window_loss += loss
        self.total_loss += loss
        self.window_steps += 1
        self.step += 1
        return lr

    def epoch(self) -> float:
        return self.step / self.source.steps_per_epoch

    def log(self, lr: float):
        st = self.opt.state()                                   # synchronises
        entry = {"step": self.step, "epoch": round(self.epoch(), 4), "loss": float(self.window_loss) / max(1, self.window_steps),
                 "learning_rate": lr, "grad_norm": st["norm"], "skipped_steps": st["skipped"]}
        self.window_loss.zero_()
        self.window_steps = 0
        self.log_history.append(entry)
        if self.rank == 0:
            logger.info(json.dumps(entry))
        return entry

    def evaluate(self) -> Dict[str, float]:
        """One evaluation of the training model on the validation set (every rank calls it: `evaluate_model` gathers) -> the metrics,
        appended to the log history with the timing keys, `step` and `epoch`.  Nothing is written and no generator is touched."""
        from . import mlm_eval
        t0 = time.time()
        sums = evaluate_model(self.model, self.valid, self.a.device)
        res = mlm_eval.metrics_from_sums(sums, self.valid.batch_size, "eval")
        rt = time.time() - t0
        batches = -(-self.valid.n // self.valid.batch_size)
        res["eval_runtime"] = round(rt, 4)
        res["eval_samples_per_second"] = round(self.valid.n / rt, 3) if rt > 0 else 0.0
        res["eval_steps_per_second"] = round(batches / rt, 3) if rt > 0 else 0.0
        entry = dict(res, step=self.step, epoch=round(self.epoch(), 4))
        self.log_history.append(entry)
        if self.rank == 0:
            logger.info(json.dumps(entry))
        return res

    def trainer_state(self) -> dict:
        return {"global_step": self.step, "epoch": self.epoch(), "max_steps": self.max_steps, "log_history": self.log_history,
                "window_loss": float(self.window_loss), "window_steps": self.window_steps, "total_loss": float(self.total_loss),
                **self.best.state()}

    def checkpoint_path(self) -> str:
        return os.path.join(self.a.output_dir, f"checkpoint-{self.step}")

    def rotate(self):
        """after a checkpoint: `--save_total_limit`; under `--load_best_model_at_end` the best checkpoint stays"""
        a = self.a
        rotate_checkpoints(a.output_dir, getattr(a, "save_total_limit", None), self.best.path if getattr(a, "load_best_model_at_end", False) else None)

    def save_checkpoint(self):
        path = self.checkpoint_path()
        save_snapshot(self.model, self.tok, path)
        torch.save(self.opt.state_dict(), os.path.join(path, "optimizer.pt"))
        torch.save(self.source.state(), os.path.join(path, "rng_state.pt"))
        _write_json(os.path.join(path, "trainer_state.json"), self.trainer_state())
        self.rotate()
        return path

    def masters(self):
        """the fp32 weights the optimizer steps on (an fp32 parameter is its own master)"""
        return [m if m is not None else p.data for m, p in zip(self.opt.master, self.opt.params)]

    def checkpoint(self):
        """A checkpoint in a data-parallel run: the ranks compare a checksum of their master weights (a mismatch raises on every rank and
        names the step), rank 0 writes, and a barrier follows so that no rank reads a checkpoint that is still being written."""
        from . import ddp
        if ddp.active():
            ddp.check_in_step(self.masters(), self.step)
        path = self.save_checkpoint() if self.rank == 0 else self.checkpoint_path()
        ddp.barrier()
        return path

    def restore_inputs(self, path: str):
        """what a checkpoint holds beside the optimizer's and the trainer's state: here the mask generator's state"""
        self.source.load_state(torch.load(os.path.join(path, "rng_state.pt"), weights_only=False))

    def resume(self, path: str):
        self.opt.load_state_dict(torch.load(os.path.join(path, "optimizer.pt"), weights_only=False))
        self.restore_inputs(path)
        with open(os.path.join(path, "trainer_state.json")) as f:
            ts = json.load(f)
        self.step, self.log_history, self.window_steps = int(ts["global_step"]), list(ts["log_history"]), int(ts["window_steps"])
        self.window_loss.fill_(ts["window_loss"])               # fp32 values, exact in the JSON's doubles
        self.total_loss.fill_(ts["total_loss"])
        self.best.load_state(ts)                                # absent in a checkpoint written before evaluations existed: none yet
        if self.opt.step_count != self.step:
            raise ValueError(f"{path}: optimizer at step {self.opt.step_count}, trainer_state at {self.step}")

    def run(self):
        """after every step, in `Trainer._maybe_log_save_evaluate`'s order: log, evaluate, save - so a checkpoint written at an evaluated
        step holds that evaluation, and is offered as the best, in its own trainer_state.json"""
        a = self.a
        every_eval = eval_interval(a, self.source.steps_per_epoch) if self.valid is not None else 0
        every_save = save_interval(a, self.source.steps_per_epoch)
        while self.step < self.max_steps:
            lr = self.train_step()
            if a.logging_steps > 0 and (self.step % a.logging_steps == 0 or self.step == self.max_steps):
                self.log(lr)
            res = self.evaluate() if every_eval and self.step % every_eval == 0 else None
            if every_save and self.step % every_save == 0:
                if res is not None:
                    self.best.offer(res["eval_loss"], self.step, self.checkpoint_path())
                self.checkpoint()


def load_best_model(model, best: BestCheckpoint) -> bool:
    """`--load_best_model_at_end`: the best checkpoint's model.safetensors into the model's parameters -> whether there was one"""
    from .checkpoint import load_state_dict
    if best.path is None:
        return False
    logger.info("Loading the best model from %s (eval_loss %s at step %d)", best.path, best.metric, best.step)
    model.load_state_dict(load_state_dict(best.path))
    return True


def load_validation(a, tok) -> ValidationSet:
    """the validation split as `--do_eval` reads it, cut to --max_eval_samples, masked once on a generator seeded with --seed"""
    from . import mlm_eval
    try:
        seqs = mlm_eval.load_sequences(a.dataset_name, "validation", a.dataset_config_name)
    except (FileNotFoundError, KeyError, ValueError) as ex:
        raise SystemExit(f"--eval_strategy {a.eval_strategy} needs the validation split of {a.dataset_name}: {ex}")
    valid = ValidationSet.build(tok, seqs, a.soft_masked_loss_weights_evaluation, a.mlm_probability, a.per_device_eval_batch_size, a.seed,
                                a.max_eval_samples)
    if valid.n == 0:
        raise SystemExit(f"--eval_strategy {a.eval_strategy}: the validation split of {a.dataset_name} holds no window")
    return valid


def train(a, rank: int = 0, world: int = 1) -> Dict[str, float]:
    """rank / world: `ddp.init_from_env`'s, with a.device this rank's device; world > 1 (or a one-rank group): the data-parallel run"""
    import torch.distributed as dist
    from . import ddp, mlm_eval
    from .optim import AdamW
    dtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}[a.dtype]
    if a.per_device_train_batch_size < 1 or a.gradient_accumulation_steps < 1:
        raise SystemExit("--per_device_train_batch_size and --gradient_accumulation_steps must be >= 1")
    main_grads = bool(getattr(a, "fp32_grad_accumulation", False))
    if main_grads and dtype != torch.bfloat16:
        raise SystemExit("--fp32_grad_accumulation requires --dtype bfloat16: with float32 parameters the gradients are fp32 already")
    tok = load_tokenizer(a)
    seqs = mlm_eval.load_sequences(a.dataset_name, "train", a.dataset_config_name)
    if a.max_train_samples is not None:
        seqs = seqs[:max(0, a.max_train_samples)]
    ids, special, weights = mlm_eval.tokenize_windows(tok, seqs, a.soft_masked_loss_weights_train)
    source = BatchSource(ids, special, weights, mlm_eval.make_collator(tok, a.mlm_probability), a.per_device_train_batch_size,
                         a.gradient_accumulation_steps * world, a.seed)     # the single process this run equals
    valid = load_validation(a, tok) if getattr(a, "eval_strategy", "no") != "no" else None      # once, before the first step, on every rank
    max_steps = a.max_steps if a.max_steps > 0 else math.ceil(a.num_train_epochs * source.steps_per_epoch)
    warmup = warmup_steps_of(a.warmup_steps, a.warmup_ratio, max_steps)
    model = build_model(a, dtype, a.resume_from_checkpoint)
    reducer = ddp.GradReducer(dist.group.WORLD, a.device) if ddp.active() else None
    opt = AdamW(model.named_parameters(), lr=a.learning_rate, betas=(a.adam_beta1, a.adam_beta2), eps=a.adam_epsilon,
                weight_decay=a.weight_decay, max_grad_norm=a.max_grad_norm, reducer=reducer, fp32_grad_accumulation=main_grads)
    tr = Trainer(model, opt, source, tok, a, max_steps, warmup, rank, world, valid)
    if a.resume_from_checkpoint:
        tr.resume(a.resume_from_checkpoint)
    if rank == 0:
        os.makedirs(a.output_dir, exist_ok=True)
    ddp.barrier()
    first = tr.step
    t0 = time.time()
    tr.run()
    torch.cuda.synchronize(a.device)
    runtime = time.time() - t0
    if reducer is not None:
        ddp.check_in_step(tr.masters(), tr.step)
    if rank == 0:
        if getattr(a, "load_best_model_at_end", False):
            load_best_model(model, tr.best)                     # output_dir becomes the best model, not the last
        save_snapshot(model, tok, a.output_dir)
    done = tr.step - first
    windows = done * a.per_device_train_batch_size * a.gradient_accumulation_steps * world      # the windows of all ranks
    metrics = {"epoch": tr.epoch(), "train_loss": float(tr.total_loss) / max(1, tr.step), "train_runtime": round(runtime, 4),
               "train_samples": int(source.n), "train_samples_per_second": round(windows / runtime, 3) if runtime > 0 else 0.0,
               "train_steps_per_second": round(done / runtime, 3) if runtime > 0 else 0.0, "skipped_steps": opt.state()["skipped"]}
    if rank == 0:
        _write_json(os.path.join(a.output_dir, "train_results.json"), metrics)
        _write_json(os.path.join(a.output_dir, "trainer_state.json"), tr.trainer_state())
    ddp.barrier()
    return metrics


def evaluate(a) -> Dict[str, float]:
    from . import mlm_eval
    model, tok = mlm_eval.load_model_and_tokenizer(a.output_dir if a.do_train else (a.model_name_or_path or a.output_dir), a.tokenizer_name,
                                                   a.device, a.dtype)
    seqs = mlm_eval.load_sequences(a.dataset_name, "validation", a.dataset_config_name)
    res = mlm_eval.evaluate_split(model, tok, seqs, "eval", a.soft_masked_loss_weights_evaluation, a.mlm_probability,
                                  a.per_device_eval_batch_size, a.seed, a.max_eval_samples, a.device)
    _write_json(os.path.join(a.output_dir, "eval_results.json"), res)
    return res


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, Dict[str, float]]:
    a = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    if not (a.do_train or a.do_eval):
        raise SystemExit("nothing to do: pass --do_train and / or --do_eval")
    if a.per_device_eval_batch_size < 1:
        raise SystemExit("--per_device_eval_batch_size must be >= 1")
    ignored = [f"--{k}" for k in IGNORED_FLAGS if getattr(a, k) is not None]
    if ignored:
        logger.info("Accepted and ignored: %s", " ".join(ignored))
    from . import ddp
    a.device, rank, world = ddp.init_from_env(a.device, ddp.backend_from(a.ddp_backend))
    results = {}
    if a.do_train:
        results["train"] = train(a, rank, world)
    ddp.shutdown()                                              # after the final barrier: no rank sits in a collective during the evaluation
    if rank != 0:
        return results
    if a.do_train:
        print(json.dumps(results["train"], sort_keys=True), flush=True)
    if a.do_eval:
        os.makedirs(a.output_dir, exist_ok=True)
        results["eval"] = evaluate(a)
        print(json.dumps(results["eval"], sort_keys=True), flush=True)
    merged = {k: v for r in results.values() for k, v in r.items()}
    _write_json(os.path.join(a.output_dir, "all_results.json"), merged)
    return results


if __name__ == "__main__":
    main()
