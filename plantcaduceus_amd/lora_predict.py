"""The commands of the reference's `src/lora_fine_tune.py` - `tokenize` (:43-170), `train` (:243-353), `evaluate` (:356-413) and
`predict` (:415-499) - for the fine-tuned PlantCAD2 models (LoRA adapters over the PlantCAD2 trunks), on the MI355X
engine:

    python -m plantcaduceus_amd.lora_predict tokenize --data_dir x.tsv --model_name <base> --sequence_length 8192 --output_path x.parquet
    python -m plantcaduceus_amd.lora_predict train    --train_dir t.parquet --valid_dir v.parquet --model_name <base> --output_dir out
    python -m plantcaduceus_amd.lora_predict predict  --checkpoint_dir <adapter> --data_dir x.parquet --task_type classification
    python -m plantcaduceus_amd.lora_predict evaluate --checkpoint_dir <adapter> --data_dir x.parquet --task_type multi_label --num_labels 92

Flags keep the reference's names (both `_` and `-` spellings; `fire` is not used).  Additions: `--dtype` (float32, the
reference's dtype - it passes none to from_pretrained - runs with "f32_gemm_split" 1, the project's parity configuration;
bfloat16), `--pooling` (the head's pooling_strategy, default mean) and `--lora-deltas` (adapters.load_adapter).  `--model_name`
overrides the adapter's base_model_name_or_path.  Hub ids resolve from local files / the HF cache only.

`train` fine-tunes `training.TrainableCaduceusForSequenceClassification` - frozen trunk, LoRA factors, `score` - with
`optim.AdamW` and `pretrain`'s schedules, window order and checkpoint form; one process and one GPU under plain `python`, data-parallel under `torchrun` as `pretrain` is (world x
`--gradient_accumulation_steps` micro-batches per step, one fused gradient all-reduce; the environment variable PCAD_DDP_BACKEND = nccl,
the default, or gloo - no flag, as below; the validation's batches of `--eval_batch_size` are dealt to the ranks in contiguous blocks and
one gather per evaluation hands every rank all logits; rank 0 logs and writes).  It takes the reference
`train()`'s flag names and defaults, except that `--bf16` defaults to false (float32, as `predict` / `evaluate` default) and means
bf16 trunk and kernels with fp32 factors and score; `save_total_limit` is 5.  Additions: `--device`, `--pooling`, `--train_lora {1,0}`
(0: the frozen-trunk mode), `--max_grad_norm` (1.0) and `--lora_dropout` (0.0; any other value is refused, as is `--use_wandb`).  The
dropout on the LoRA branches (the reference's lora_dropout=0.1) is set by the environment variable PCAD_LORA_DROPOUT.
`output_dir/checkpoint-<step>/` is an adapter directory plus `optimizer.pt` and `trainer_state.json`; `output_dir/` ends as the final
adapter, which `predict --checkpoint_dir <output_dir> --lora-deltas apply` loads (after `--train_lora 0`: the default `auto`).
Whether the blocks' activations are kept or recomputed in the backward (the same bits either way) is `recompute_policy`'s
choice, logged at the start: the environment variable PCAD_TRAIN_RECOMPUTE=1 / 0 forces it, unset or `auto` recomputes when the formula's
stored bytes for a micro-batch exceed half of the device's free memory.  The command has no flag for it: the flag set is the reference's.
Likewise PCAD_TRAIN_SCAN_SEGMENTS (`pretrain.scan_segments_from_env`: unset or 1 off, 2..64, or auto) cuts every strand of the selective
scan's backward into segments walked in parallel - long windows at a small --train_batch_size; logged at the start.
PCAD_TRAIN_SCAN_FWD_SEGMENTS (the same helper and values) does so for the scan's forward: a setting of its own, logged too.
PCAD_TRAIN_FEATURES=cache (unset or `off`: nothing changes) is the frozen-trunk mode on cached features: it needs
`--train_lora 0`, runs the trunk ONCE per training and validation window on the inference engine before the first step - in fixed blocks of
max(1, 2^18 // L) consecutive windows, or PCAD_TRAIN_FEATURE_BATCH -, keeps the pooled vectors [N, 2, D] on the device and trains and
evaluates the score head on them (`ops.pooled_logits_fn`); a run that schedules fewer samples than half the training set is refused.

Under torchrun the windows are sharded over the ranks (plantcad2_eval._sharded_rows); rank 0 writes / prints.  Metrics are
computed on the host without sklearn (the reference's compute_metrics_* :517-563 restated; pinned against sklearn / scipy in
tests/test_seqcls.py).
"""
from __future__ import annotations

import json
import logging
import os
import time
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import pretrain, sharding
from .plantcad2_eval import _midranks, _sharded_rows, auroc, average_precision

logger = logging.getLogger(__name__)

TASK_TYPES = ("classification", "regression", "multi_label")


# ---------------------------------------------------------------------------------------------------------------------
# data
def sample_indices(n: int, sampling_rate: Optional[float], seed: int = 42) -> Optional[np.ndarray]:
    """`Dataset.shuffle(seed).select(range(max(1, int(rate * n))))` (:390-395): datasets' shuffle is the permutation
    `np.random.default_rng(seed).permutation(n)` (pinned against `datasets` in tests/test_seqcls.py).  None: keep all rows."""
    if not sampling_rate:
        return None
    if sampling_rate > 1 or sampling_rate <= 0:
        raise ValueError("sampling_rate must be in (0, 1]")
    k = max(min(int(sampling_rate * n), n), 1)
    return np.random.default_rng(seed).permutation(n)[:k]


def read_tokenized(path: str) -> Tuple[np.ndarray, Optional[np.ndarray], Optional[str]]:
    """The `tokenize` command's parquet -> (ids int32 [N, L], labels or None, label column name or None).  The `input_ids` list
    column is flattened and reshaped (pyarrow), not converted row by row."""
    import pyarrow.parquet as pq
    t = pq.read_table(path)
    if "input_ids" not in t.column_names:
        raise ValueError("Dataset must contain 'input_ids'. Tokenize your data first via `tokenize` and pass the resulting parquet.")
    col = t.column("input_ids").combine_chunks()
    n = len(col)
    flat = np.asarray(col.flatten().to_numpy(zero_copy_only=False))
    offs = np.asarray(col.offsets.to_numpy())
    lens = np.diff(offs)
    if n and (lens != lens[0]).any():
        raise ValueError(f"input_ids rows of unequal length {sorted(set(lens.tolist()))[:4]}: tokenize with padding='max_length'")
    L = int(lens[0]) if n else 0
    ids = flat[offs[0]:offs[0] + n * L].astype(np.int32).reshape(n, L)
    labels, name = None, None
    for c in ("labels", "label"):
        if c in t.column_names:
            name = c
            v = t.column(c).combine_chunks()
            if c == "labels" and hasattr(v, "flatten") and hasattr(v, "offsets"):
                fl = np.asarray(v.flatten().to_numpy(zero_copy_only=False))
                labels = fl.reshape(n, -1) if n else fl.reshape(0, 0)
            else:
                labels = np.asarray(v.to_numpy(zero_copy_only=False))
            break
    return ids, labels, name


def _to_label_list(val):
    """multi_label Label: a 0/1 string or a list (:110-120)."""
    if isinstance(val, str):
        return [int(c) for c in val]
    if isinstance(val, (list, tuple, np.ndarray)):
        return [int(x) for x in val]
    return [int(c) for c in str(val)]


def tokenize(data_dir: Optional[str] = None, output_path: Optional[str] = None, model_name: Optional[str] = None,
             sequence_length: int = 8192, batch_size: int = 1000, max_batches: Optional[int] = None, num_proc: Optional[int] = None,
             task_type: str = "classification", hf_dataset: Optional[str] = None, hf_config: Optional[str] = None,
             hf_split: str = "train", seq_column: str = "sequence", label_column: str = "label") -> str:
    """Local TSV (case-insensitive columns) or a `datasets` dataset from the local cache -> parquet with `input_ids` (list of int,
    padded / truncated to sequence_length) and `label` (or `labels` for multi_label).  -> the parquet path."""
    import pandas as pd
    import pyarrow as pa
    import pyarrow.parquet as pq
    from transformers import AutoTokenizer
    from . import register
    if model_name is None:
        raise ValueError("model_name must be provided to load the tokenizer")
    if data_dir is None and hf_dataset is None:
        raise ValueError("Provide either data_dir (local TSV) or hf_dataset (Hugging Face)")
    register()
    from .checkpoint import resolve_snapshot
    tok = AutoTokenizer.from_pretrained(resolve_snapshot(model_name))
    if hf_dataset is not None:
        os.environ.setdefault("HF_DATASETS_OFFLINE", "1")        # the local datasets cache only
        os.environ.setdefault("HF_HUB_OFFLINE", "1")
        from datasets import load_dataset
        df = load_dataset(hf_dataset, hf_config, split=hf_split).to_pandas()
    else:
        if output_path is None:
            from pathlib import Path
            output_path = str(Path(data_dir).with_suffix(".parquet"))
        # as text: a multi_label Label such as "0101" keeps its leading zeros (a numeric parse would read 101)
        df = pd.read_csv(data_dir, sep="\t", dtype=str, keep_default_na=False)
    df.columns = [str(c).lower() for c in df.columns]
    seq_column, label_column = seq_column.lower(), label_column.lower()
    if hf_dataset is None and task_type != "multi_label" and label_column in df.columns:
        df[label_column] = pd.to_numeric(df[label_column])
    if max_batches is not None:
        df = df.iloc[:min(max_batches * batch_size, len(df))]
    if seq_column not in df.columns:
        raise KeyError(f"Missing sequence column '{seq_column}' in dataset; set --seq_column if different")
    ids = tok.encode_batch_padded([str(s) for s in df[seq_column]], max_length=sequence_length, padding="max_length",
                                  truncation=True)
    cols = {"input_ids": pa.array(list(ids), type=pa.list_(pa.int32()))} if len(ids) else \
        {"input_ids": pa.array([], type=pa.list_(pa.int32()))}
    if task_type == "multi_label":
        if label_column not in df.columns:
            raise KeyError(f"Missing label column '{label_column}' for multi_label tasks")
        cols["labels"] = pa.array([_to_label_list(v) for v in df[label_column]], type=pa.list_(pa.int64()))
    elif label_column in df.columns:
        cols["label"] = pa.array(df[label_column].to_numpy())
    if output_path is None:
        src = hf_dataset.replace("/", "_")
        output_path = f"{src}{'_' + hf_config if hf_config else ''}_{hf_split}_tokenized.parquet"
    pq.write_table(pa.table(cols), output_path, compression="zstd")
    logger.info("Saved %d tokenized rows to %s", len(ids), output_path)
    return output_path


# ---------------------------------------------------------------------------------------------------------------------
# metrics (compute_metrics_* :517-563, without sklearn / scipy)
def _softmax(x: np.ndarray) -> np.ndarray:
    return torch.softmax(torch.as_tensor(x, dtype=torch.float32), dim=1).numpy()


def _sigmoid(x: np.ndarray) -> np.ndarray:
    return torch.sigmoid(torch.as_tensor(x, dtype=torch.float32)).numpy()


def _f1(y: np.ndarray, p: np.ndarray) -> float:
    tp = float(np.sum((y == 1) & (p == 1)))
    fp = float(np.sum((y != 1) & (p == 1)))
    fn = float(np.sum((y == 1) & (p != 1)))
    return 0.0 if tp == 0 else 2 * tp / (2 * tp + fp + fn)


def _pearson(a: np.ndarray, b: np.ndarray) -> float:
    a = np.asarray(a, dtype=np.float64)
    b = np.asarray(b, dtype=np.float64)
    a, b = a - a.mean(), b - b.mean()
    den = np.sqrt((a * a).sum() * (b * b).sum())
    return float((a * b).sum() / den) if den > 0 else float("nan")


def metrics_classification(logits: np.ndarray, labels: np.ndarray) -> Dict[str, float]:
    labels = np.asarray(labels).astype(np.int64).reshape(-1)
    preds = np.argmax(logits, axis=1)
    scores = _softmax(logits)[:, 1]
    return {"accuracy": float(np.mean(preds == labels)), "f1": _f1(labels, preds), "roc_auc": auroc(labels, scores),
            "average_precision": average_precision(labels, scores), "balance": float(np.sum(labels) / len(labels))}


def metrics_regression(logits: np.ndarray, labels: np.ndarray) -> Dict[str, float]:
    pred = np.asarray(logits).squeeze()
    labels = np.asarray(labels).reshape(pred.shape)
    mse = ((pred - labels) ** 2).mean()
    ss_tot = ((labels - labels.mean()) ** 2).sum()
    ss_res = ((labels - pred) ** 2).sum()
    return {"mse": float(mse), "rmse": float(np.sqrt(mse)), "mae": float(np.abs(pred - labels).mean()),
            "r2": float(1 - ss_res / (ss_tot + 1e-8)), "pearson_r": _pearson(pred, labels),
            "spearman_r": _pearson(_midranks(np.asarray(pred, dtype=np.float64)), _midranks(np.asarray(labels, dtype=np.float64)))}


def metrics_multilabel(logits: np.ndarray, labels: np.ndarray) -> Dict[str, float]:
    """sklearn's accuracy_score on 2-D indicators is the exact-match ratio; f1 / roc_auc / average_precision `average="micro"`
    are the binary metrics of the flattened arrays."""
    labels = np.asarray(labels).astype(np.int64)
    probs = _sigmoid(logits)
    preds = (probs > 0.5).astype(np.int64)
    return {"accuracy": float(np.mean(np.all(preds == labels, axis=1))), "f1": _f1(labels.ravel(), preds.ravel()),
            "roc_auc": auroc(labels.ravel(), probs.ravel()), "average_precision": average_precision(labels.ravel(), probs.ravel())}


METRICS = {"classification": metrics_classification, "regression": metrics_regression, "multi_label": metrics_multilabel}


# ---------------------------------------------------------------------------------------------------------------------
# model + inference
def load_model(checkpoint_dir: str, task_type: str, num_labels: Optional[int], model_name: Optional[str], device: str,
               dtype: str = "float32", pooling: str = "mean", lora_deltas: str = "auto"):
    from .adapters import load_adapter
    from .configuration_caduceus import CaduceusConfig  # noqa: F401
    if task_type not in TASK_TYPES:
        raise ValueError(f"task_type must be one of {TASK_TYPES}")
    if task_type == "multi_label" and (num_labels is None or num_labels <= 1):
        raise ValueError("For multi_label, please provide num_labels > 1")
    td = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    model = load_adapter(checkpoint_dir, task_type=task_type, num_labels=num_labels, lora_deltas=lora_deltas, base=model_name,
                         dtype=td, pooling_strategy=pooling)
    if td == torch.float32:
        # the project's parity configuration for the reference's fp32 numbers (packed at bind time: set before the engine exists)
        opts = dict(getattr(model.config, "engine_options", None) or {})
        opts.setdefault("f32_gemm_split", 1)
        model.config.engine_options = opts
    return model.to(device).eval()


def predict_logits(model, ids: np.ndarray, device: str, batch_size: int = 32) -> np.ndarray:
    """fp32 logits [N, num_labels] in row order; sharded over the ranks of a process group (plantcad2_eval._sharded_rows)."""
    from .zero_shot import check_model_inputs
    n = ids.shape[0]
    nl = int(model.num_labels)
    t = torch.from_numpy(np.ascontiguousarray(ids))

    def run_rows(lo, hi):
        if hi <= lo:
            return torch.zeros((0, nl), dtype=torch.float32, device=device)
        parts = [model(input_ids=t[b0:min(b0 + batch_size, hi)].to(device)).logits for b0 in range(lo, hi, batch_size)]
        return torch.cat(parts, dim=0)

    out = np.zeros((n, nl), dtype=np.float32)
    with torch.inference_mode():
        _sharded_rows(n, run_rows, out)
    check_model_inputs(model)
    return out


def eval_loss(model, logits: np.ndarray, labels: np.ndarray, task_type: str, batch_size: int) -> float:
    """Trainer.evaluate's `eval_loss`: the model's loss per batch of `batch_size`, repeated per sample, averaged."""
    lab = torch.as_tensor(labels)
    lab = lab.float() if task_type in ("multi_label", "regression") else lab.long()
    lg = torch.as_tensor(logits, dtype=torch.float32)
    tot, n = 0.0, lg.shape[0]
    for b0 in range(0, n, batch_size):
        b1 = min(b0 + batch_size, n)
        tot += float(model.loss_from_logits(lg[b0:b1], lab[b0:b1])) * (b1 - b0)
    return tot / max(n, 1)


def predict(checkpoint_dir: str, data_dir: str, output_file: str = "/tmp/predictions.csv", model_name: Optional[str] = None,
            task_type: str = "classification", num_labels: Optional[int] = None, batch_size: int = 32,
            sampling_rate: Optional[float] = None, seed: int = 42, device: str = "cuda:0", dtype: str = "float32",
            pooling: str = "mean", lora_deltas: str = "auto"):
    """-> the DataFrame written to output_file (rank 0): probability_positive / predicted_value / class_0 .. class_{N-1}."""
    import pandas as pd
    model = load_model(checkpoint_dir, task_type, num_labels, model_name, device, dtype, pooling, lora_deltas)
    ids, _, _ = read_tokenized(data_dir)
    sel = sample_indices(len(ids), sampling_rate, seed)
    if sel is not None:
        ids = ids[sel]
    logits = predict_logits(model, ids, device, batch_size)
    if task_type == "classification":
        df = pd.DataFrame({"probability_positive": _softmax(logits)[:, 1]})
    elif task_type == "regression":
        df = pd.DataFrame({"predicted_value": logits.squeeze()})
    else:
        probs = _sigmoid(logits)
        df = pd.DataFrame(probs, columns=[f"class_{i}" for i in range(probs.shape[1])])
    if sharding.world()[0] == 0:
        logger.info("Saving predictions to %s", output_file)
        df.to_csv(output_file, index=False)
    return df


def evaluate(checkpoint_dir: str, data_dir: str, output_dir: str = "/tmp/pcv2-ft-eval", model_name: Optional[str] = None,
             task_type: str = "classification", num_labels: Optional[int] = None, batch_size: int = 32,
             sampling_rate: Optional[float] = None, seed: int = 42, device: str = "cuda:0", dtype: str = "float32",
             pooling: str = "mean", lora_deltas: str = "auto") -> Dict[str, float]:
    """-> Trainer.evaluate's dict: eval_loss, eval_<compute_metrics_* keys>, eval_runtime, eval_samples_per_second,
    eval_steps_per_second (printed by rank 0)."""
    model = load_model(checkpoint_dir, task_type, num_labels, model_name, device, dtype, pooling, lora_deltas)
    ids, labels, _ = read_tokenized(data_dir)
    if labels is None:
        raise ValueError(f"{data_dir} has no label / labels column to evaluate against")
    sel = sample_indices(len(ids), sampling_rate, seed)
    if sel is not None:
        ids, labels = ids[sel], labels[sel]
    t0 = time.time()
    logits = predict_logits(model, ids, device, batch_size)
    res = {"eval_loss": eval_loss(model, logits, labels, task_type, batch_size)}
    res.update({"eval_" + k: v for k, v in METRICS[task_type](logits, labels).items()})
    rt = time.time() - t0
    n = len(ids)
    res["eval_runtime"] = round(rt, 4)
    res["eval_samples_per_second"] = round(n / rt, 3) if rt > 0 else float("inf")
    res["eval_steps_per_second"] = round(-(-n // batch_size) / rt, 3) if rt > 0 else float("inf")
    if sharding.world()[0] == 0:
        print(res, flush=True)
    return res


# ---------------------------------------------------------------------------------------------------------------------
# train (reference :243-353)
class LabelledBatches(pretrain.WindowOrder):
    """`pretrain.WindowOrder` over labelled windows: the micro-batches of every optimizer step, a function of (seed, data, batch,
    accumulation); nothing is drawn per batch."""

    def __init__(self, ids: np.ndarray, labels: np.ndarray, batch: int, accumulation: int, seed: int):
        super().__init__(ids.shape[0], batch, accumulation, seed)
        self.ids, self.labels = ids, labels

    def step_batches(self, step: int):
        """-> [(input_ids int32 [b, L], labels [b] or [b, NL], None)] CPU tensors"""
        return [(torch.from_numpy(self.ids[idx].copy()), torch.from_numpy(self.labels[idx].copy()), None) for idx in self.windows(step)]


class LabelledIndexBatches(LabelledBatches):
    """`LabelledBatches` for a run on cached features: the same windows for the same (seed, step) - `windows(step)` is
    the parent's - handed out as dataset indices instead of ids, so that the micro-step gathers their rows from the cache."""

    def step_batches(self, step: int):
        """-> [(window indices int64 [b], labels [b] or [b, NL], None)] CPU tensors"""
        return [(torch.from_numpy(np.asarray(idx, dtype=np.int64).copy()), torch.from_numpy(self.labels[idx].copy()), None)
                for idx in self.windows(step)]


def _labels_for(labels: np.ndarray, task_type: str) -> np.ndarray:
    if task_type == "classification":
        return np.asarray(labels).astype(np.int64).reshape(-1)
    if task_type == "regression":
        return np.asarray(labels).astype(np.float32).reshape(-1)
    return np.asarray(labels).astype(np.float32)


_interval = pretrain.interval

SAVE_TOTAL_LIMIT = 5          # the reference's TrainingArguments(save_total_limit=5)


class FinetuneTrainer(pretrain.Trainer):
    """`pretrain.Trainer` around the sequence-classification model: its step, schedule, logging, trainer_state and resume; the micro-step,
    the checkpoint (an adapter directory) and the evaluation are this command's.  a: the command's settings (output_dir, model_name,
    task_type, device, learning_rate, lr_scheduler_type, warmup_steps, eval_batch_size, eval / save strategy and steps, logging_steps);
    valid: (ids, labels) of the validation windows, or None."""

    def __init__(self, model, optimizer, source, a, max_steps: int, valid=None, rank: int = 0, world: int = 1):
        super().__init__(model, optimizer, source, None, a, max_steps, int(a.warmup_steps), rank, world)
        self.valid = valid

    def before_micro_step(self, j: int, n: int):
        """the dropout masks of micro-batch j of this step are those it has in the one-process run: a function of (seed, step n + j), so
        that W ranks x accumulation A draw what one process with accumulation A W draws, and a resumed run needs no generator state"""
        self.model.dropout_step = self.step * n + j

    def micro_step(self, ids, labels, _weights):
        dev = self.a.device
        out = self.model(ids.to(dev), labels.to(dev))
        out.loss.backward()
        return out.loss.detach()

    def evaluate(self):
        ids, labels = self.valid
        t0 = time.time()
        logits = predict_logits_trainable(self.model, ids, self.a.device, self.a.eval_batch_size)
        res = {"eval_loss": eval_loss(self.model, logits, labels, self.a.task_type, self.a.eval_batch_size)}
        res.update({"eval_" + k: v for k, v in METRICS[self.a.task_type](logits, labels).items()})
        res["eval_runtime"] = round(time.time() - t0, 4)
        entry = dict(res, step=self.step, epoch=round(self.epoch(), 4))
        self.log_history.append(entry)
        if self.rank == 0:                                      # the logits are gathered: every rank holds the same values
            logger.info(json.dumps(entry))
        return res

    def save_checkpoint(self):
        path = self.checkpoint_path()
        self.model.save_adapter(path, self.a.model_name)
        torch.save(self.opt.state_dict(), os.path.join(path, "optimizer.pt"))
        pretrain._write_json(os.path.join(path, "trainer_state.json"), self.trainer_state())
        pretrain.rotate_checkpoints(self.a.output_dir, SAVE_TOTAL_LIMIT)
        return path

    def restore_inputs(self, path: str):
        """a checkpoint is an adapter directory: the factors and the head (nothing is drawn per batch, so there is no generator state)"""
        self.model.load_adapter_weights(path)

    def run(self):
        a = self.a
        every_eval = _interval(a.eval_strategy, a.eval_steps, self.source.steps_per_epoch, "eval_strategy") if self.valid is not None else 0
        every_save = _interval(a.save_strategy, a.save_steps, self.source.steps_per_epoch, "save_strategy")
        while self.step < self.max_steps:
            lr = self.train_step()
            if a.logging_steps > 0 and (self.step % a.logging_steps == 0 or self.step == self.max_steps):
                self.log(lr)
            if every_eval and self.step % every_eval == 0:
                self.evaluate()
            if every_save and self.step % every_save == 0:
                self.checkpoint()


class FeatureTrainer(FinetuneTrainer):
    """`FinetuneTrainer` on cached pooled features: `source` is a `LabelledIndexBatches`, `features` the training
    windows' cache fp32 [N, 2, D] on the device and `valid` (features [Nv, 2, D], labels).  The micro-step gathers its rows and runs
    the score head alone; the evaluation takes its logits from the cached validation features.  No trunk forward runs here."""

    def __init__(self, model, optimizer, source, a, max_steps: int, features: torch.Tensor, valid=None, rank: int = 0, world: int = 1):
        super().__init__(model, optimizer, source, a, max_steps, valid, rank, world)
        self.features = features

    def before_micro_step(self, j: int, n: int):
        """nothing is drawn: the mode has no LoRA branch"""

    def micro_step(self, idx, labels, _weights):
        dev = self.a.device
        out = self.model(pooled=self.features.index_select(0, idx.to(dev)), labels=labels.to(dev))
        out.loss.backward()
        return out.loss.detach()

    def eval_logits(self) -> np.ndarray:
        feats, bs = self.valid[0], max(1, int(self.a.eval_batch_size))
        with torch.no_grad():
            parts = [self.model.logits_from_features(feats[b0:b0 + bs]) for b0 in range(0, feats.shape[0], bs)]
        nl = int(self.model.num_labels)
        return (torch.cat(parts, dim=0) if parts else torch.zeros((0, nl), dtype=torch.float32)).cpu().numpy()

    def evaluate(self):
        labels = self.valid[1]
        t0 = time.time()
        logits = self.eval_logits()                              # every rank holds the whole cache: the same values everywhere, no gather
        res = {"eval_loss": eval_loss(self.model, logits, labels, self.a.task_type, self.a.eval_batch_size)}
        res.update({"eval_" + k: v for k, v in METRICS[self.a.task_type](logits, labels).items()})
        res["eval_runtime"] = round(time.time() - t0, 4)
        entry = dict(res, step=self.step, epoch=round(self.epoch(), 4))
        self.log_history.append(entry)
        if self.rank == 0:
            logger.info(json.dumps(entry))
        return res


FEATURES_ENV = "PCAD_TRAIN_FEATURES"
FEATURE_BATCH_ENV = "PCAD_TRAIN_FEATURE_BATCH"
FEATURE_BLOCK_POSITIONS = 2 ** 18        # windows x positions of one block of the feature pass: 32 windows at L = 8 192


def train_features_from_env(env=None, train_lora: bool = True) -> bool:
    """Whether `train` runs on cached pooled features, from the environment variable PCAD_TRAIN_FEATURES (`env`: a
    mapping, os.environ when None): unset, empty or `off` - no; `cache` - yes, which needs --train_lora 0 (with trained factors the
    features move every step).  Anything else, and `cache` with --train_lora 1, exits naming the variable (and the flag)."""
    val = str((os.environ if env is None else env).get(FEATURES_ENV, "")).strip().lower()
    if val in ("", "off"):
        return False
    if val != "cache":
        raise SystemExit(f"{FEATURES_ENV} must be off or cache, got {val!r}")
    if train_lora:
        raise SystemExit(f"{FEATURES_ENV}=cache needs --train_lora 0: with trained LoRA factors the trunk's features change every step and "
                         "cannot be cached; unset one")
    return True


def feature_block_windows(L: int, env=None) -> int:
    """Windows per block of the feature pass: max(1, 2^18 // L) - a function of L alone, so that a window always meets the same
    companions - unless PCAD_TRAIN_FEATURE_BATCH (a positive integer) overrides it."""
    val = str((os.environ if env is None else env).get(FEATURE_BATCH_ENV, "")).strip()
    if not val:
        return max(1, FEATURE_BLOCK_POSITIONS // max(1, int(L)))
    try:
        fb = int(val)
    except ValueError:
        fb = 0
    if fb < 1:
        raise SystemExit(f"{FEATURE_BATCH_ENV} must be a positive integer, got {val!r}")
    return fb


def check_feature_budget(scheduled: int, n_train: int):
    """The feature pass costs one trunk forward per training window; a run that schedules fewer samples than half of them would pay
    more forwards for the pass than the plain path pays in all: exit naming the two numbers and the variable."""
    if 2 * int(scheduled) < int(n_train):
        raise SystemExit(f"{FEATURES_ENV}=cache: the run schedules {int(scheduled)} samples (steps x batch x accumulation x world), fewer than "
                         f"half of the {int(n_train)} training windows the feature pass would send through the trunk; unset {FEATURES_ENV}")


def feature_pass(n: int, fb: int, run_block, width: int, device) -> torch.Tensor:
    """[n, width] fp32 on every rank: `run_block(lo, hi)` -> [hi - lo, width] over FIXED blocks of `fb` consecutive dataset indices (the
    last one short), dealt to the ranks in contiguous runs of whole blocks and reassembled by one gather
    (`sharding.gather_batch_rows`).  A window's block - its companions in the forward - depends on (index, fb) alone, never on the
    training order, the world size or a resume, so its row's bits do not either."""
    return sharding.gather_batch_rows(int(n), int(fb), run_block, int(width), device)


def cache_features(model, ids: np.ndarray, device, fb: int) -> torch.Tensor:
    """the frozen trunk's pooled vectors of every window of `ids` [N, L] -> fp32 [N, 2, D] on `device`: `feature_pass` over
    `model.pooled_features`"""
    D = int(model.config.d_model)
    t = torch.from_numpy(np.ascontiguousarray(ids))
    rows = feature_pass(len(ids), fb, lambda lo, hi: model.pooled_features(t[lo:hi].to(device)).reshape(hi - lo, 2 * D), 2 * D, device)
    from .zero_shot import check_model_inputs
    check_model_inputs(model.feature_engine())                   # an id outside the vocabulary raises here, on every rank
    return rows.reshape(len(ids), 2, D).contiguous()


def predict_logits_trainable(model, ids: np.ndarray, device: str, batch_size: int) -> np.ndarray:
    """fp32 logits [N, num_labels] of the trainable model under torch.no_grad(), one forward per batch of `batch_size` windows.  In a
    process group the batches are dealt to the ranks in contiguous blocks (`sharding.batch_block`) - every forward sees
    the rows it sees in a one-process run - and one gather hands every rank all rows."""
    t = torch.from_numpy(np.ascontiguousarray(ids))
    with torch.no_grad():
        logits = sharding.gather_batch_rows(len(ids), batch_size, lambda lo, hi: model(t[lo:hi].to(device)).logits, int(model.num_labels), device)
    return logits.cpu().numpy()


RECOMPUTE_ENV = "PCAD_TRAIN_RECOMPUTE"
DROPOUT_ENV = "PCAD_LORA_DROPOUT"


def lora_dropout_from_env(env=None, train_lora: bool = True) -> float:
    """The dropout rate of the LoRA branches from the environment variable PCAD_LORA_DROPOUT (`env`: a mapping, os.environ
    when None): unset or empty 0.0; a number in [0, 1) whose threshold floor(p 65536 + 0.5) is at most 65535.  Anything else, and a
    rate above 0 with --train_lora 0 (frozen factors have no branch to regularise), exits naming the variable."""
    from .ops import lora_dropout_threshold
    val = str((os.environ if env is None else env).get(DROPOUT_ENV, "")).strip()
    if not val:
        return 0.0
    try:
        p = float(val)
        lora_dropout_threshold(p)
    except ValueError:
        raise SystemExit(f"{DROPOUT_ENV} must be a number in [0, 1), got {val!r}")
    if p > 0 and not train_lora:
        raise SystemExit(f"{DROPOUT_ENV}={val} with --train_lora 0: the factors are frozen at zero, there is no LoRA branch to drop out; unset one")
    return p


def recompute_policy(bytes_per_window: int, batch: int, free_bytes: int, env=None, train_lora: bool = True) -> bool:
    """Whether `train` recomputes each block in the backward (training's gradient_checkpointing).  `env` is the process
    environment (a mapping; os.environ when None): PCAD_TRAIN_RECOMPUTE=1 forces it on, =0 off; unset or `auto` turns it on exactly when
    the factors train and a micro-batch's stored activations, batch * bytes_per_window by the formula
    (bytes_per_window = 2 L * training.stored_bytes_per_strand_position), exceed half of the device's free bytes.  The half is room for
    what the formula leaves out (the merged weights, the operators' own copies, the allocator's slack): a stated policy, not a measured
    threshold.  Gradients are bit-equal either way, so the choice changes no result."""
    val = env if isinstance(env, str) else (os.environ if env is None else env).get(RECOMPUTE_ENV, "auto")     # a bare value is taken too
    val = str(val).strip().lower() or "auto"
    if val not in ("0", "1", "auto"):
        raise ValueError(f"{RECOMPUTE_ENV} must be 0, 1 or auto, got {val!r}")
    if val != "auto":
        return val == "1"
    return bool(train_lora) and int(batch) * int(bytes_per_window) > int(free_bytes) / 2


def train(train_dir: str, valid_dir: str, output_dir: str = "/tmp/pcv2-ft", model_name: Optional[str] = None,
          task_type: str = "classification", num_labels: Optional[int] = None, train_batch_size: int = 43, eval_batch_size: int = 3,
          eval_num_samples: Optional[int] = 0, max_steps: int = 500, seed: int = 42, use_wandb: bool = False, learning_rate: float = 1e-3,
          warmup_steps: int = 50, lr_scheduler_type: str = "linear", gradient_accumulation_steps: int = 64, bf16: bool = False,
          num_train_epochs: float = 3, weight_decay: float = 0.01, eval_strategy: str = "steps", eval_steps: int = 25,
          save_strategy: str = "steps", save_steps: int = 100, logging_steps: int = 100, resume_from_checkpoint: Optional[str] = None,
          device: str = "cuda:0", pooling: str = "mean", train_lora: int = 1, max_grad_norm: float = 1.0, lora_dropout: float = 0.0) -> Dict[str, float]:
    """Fine-tune a PlantCAD2 trunk with LoRA on tokenized parquet files (the `tokenize` command's).  -> the train metrics.
    Under `torchrun` the run is data-parallel as `pretrain`'s is: world x gradient_accumulation_steps micro-batches per
    step, rank r running those with index j = r (mod world); `device` is then the rank's own (PCAD_DDP_BACKEND: nccl, the default, or gloo)."""
    import math
    from types import SimpleNamespace
    import torch.distributed as dist
    from . import ddp
    from .adapters import TASKS
    from .optim import AdamW
    from .training import TrainableCaduceusForSequenceClassification, stored_bytes_per_strand_position
    if model_name is None:
        raise SystemExit("--model_name is required")
    if task_type not in TASK_TYPES:
        raise SystemExit(f"--task_type must be one of {TASK_TYPES}")
    if task_type == "multi_label" and (num_labels is None or num_labels <= 1):
        raise SystemExit("For multi_label, please provide --num_labels > 1")
    if use_wandb:
        raise SystemExit("--use_wandb is not supported: the log history is written to trainer_state.json")
    if float(lora_dropout) != 0.0:
        raise SystemExit(f"--lora_dropout {lora_dropout} is not accepted on the command line yet: set the environment variable "
                         f"{DROPOUT_ENV}={lora_dropout} instead (DESIGN.md §4u); the flag itself takes only 0.0")
    dropout = lora_dropout_from_env(os.environ, bool(int(train_lora)))
    cached = train_features_from_env(os.environ, bool(int(train_lora)))
    segments = pretrain.scan_segments_from_env(os.environ)
    fwd_segments = pretrain.scan_segments_from_env(os.environ, pretrain.SCAN_FWD_SEGMENTS_ENV)
    if pooling not in ("mean", "first", "last"):
        raise SystemExit(f"--pooling {pooling} has no backward (max pooling's gradient needs a tie rule nothing pins): one of mean, first, last")
    if lr_scheduler_type not in pretrain.SCHEDULES:
        raise SystemExit(f"--lr_scheduler_type must be one of {', '.join(pretrain.SCHEDULES)}")
    if train_batch_size < 1 or gradient_accumulation_steps < 1 or eval_batch_size < 1:
        raise SystemExit("--train_batch_size, --eval_batch_size and --gradient_accumulation_steps must be >= 1")
    nl, problem_type = TASKS[task_type]
    nl = int(num_labels) if task_type == "multi_label" else nl
    device, rank, world = ddp.init_from_env(device, ddp.backend_from())
    ids, labels, _ = read_tokenized(train_dir)
    if labels is None:
        raise SystemExit(f"{train_dir} has no label / labels column to train on")
    source = (LabelledIndexBatches if cached else LabelledBatches)(ids, _labels_for(labels, task_type), train_batch_size,
                                                                   gradient_accumulation_steps * world, seed)
    valid = None
    if valid_dir:
        vids, vlabels, _ = read_tokenized(valid_dir)
        if vlabels is None:
            raise SystemExit(f"{valid_dir} has no label / labels column to evaluate against")
        if eval_num_samples:
            vids, vlabels = vids[:eval_num_samples], vlabels[:eval_num_samples]
        valid = (vids, vlabels)
    total = max_steps if max_steps > 0 else math.ceil(num_train_epochs * source.steps_per_epoch)
    if cached:
        check_feature_budget(total * train_batch_size * gradient_accumulation_steps * world, len(ids))
    model = TrainableCaduceusForSequenceClassification.from_pretrained(
        model_name, nl, problem_type, pooling_strategy=pooling, dtype=torch.bfloat16 if bf16 else torch.float32, device=device,
        train_lora=bool(int(train_lora)), seed=seed, lora_dropout=dropout, scan_bwd_segments=segments,
        scan_fwd_segments=fwd_segments)
    model.dropout_seed = int(seed) % (1 << 64)
    if dropout > 0:
        logger.info("LoRA dropout (%s): %g, masks from seed %d and the micro-batch's index in the one-process run", DROPOUT_ENV, dropout, seed)
    logger.info("Segments of the scan's backward (%s): %s", pretrain.SCAN_SEGMENTS_ENV, "off" if segments == 1 else segments)
    logger.info("Segments of the scan's forward (%s): %s", pretrain.SCAN_FWD_SEGMENTS_ENV, "off" if fwd_segments == 1 else fwd_segments)
    per_window = 2 * ids.shape[1] * stored_bytes_per_strand_position(model.config, model.dtype, lora=True)
    free_bytes = torch.cuda.mem_get_info(device)[0]
    if recompute_policy(per_window, train_batch_size, free_bytes, os.environ, model.train_lora):
        model.gradient_checkpointing_enable()
    logger.info("Recompute blocks in the backward (%s=%s): %s; stored activations by the formula %d bytes per micro-batch (%d windows), "
                "%d bytes free on %s", RECOMPUTE_ENV, os.environ.get(RECOMPUTE_ENV, "auto"), "on" if model.is_gradient_checkpointing else "off",
                train_batch_size * per_window, train_batch_size, free_bytes, device)
    n_train = sum(p.numel() for p in model.parameters() if p.requires_grad)
    n_all = sum(p.numel() for p in model.parameters())
    logger.info("Trainable parameters: %d of %d (%.2f%%)", n_train, n_all, 100.0 * n_train / n_all)
    reducer = ddp.GradReducer(dist.group.WORLD, device) if ddp.active() else None
    opt = AdamW(model.named_parameters(), lr=learning_rate, weight_decay=weight_decay, max_grad_norm=max_grad_norm, reducer=reducer)
    a = SimpleNamespace(output_dir=output_dir, model_name=model_name, task_type=task_type, device=device, learning_rate=learning_rate,
                        lr_scheduler_type=lr_scheduler_type, warmup_steps=warmup_steps, eval_batch_size=eval_batch_size, eval_strategy=eval_strategy,
                        eval_steps=eval_steps, save_strategy=save_strategy, save_steps=save_steps, logging_steps=logging_steps)
    feature_runtime = None
    if cached:
        # the trunk runs once per window, on the inference engine, before the first step; a resumed run runs the pass again
        fb = feature_block_windows(ids.shape[1], os.environ)
        model.feature_engine({} if bf16 else {"f32_gemm_split": 1})     # the options `predict` runs the trunk with (load_model)
        torch.cuda.synchronize(device)
        t_pass = time.time()
        features = cache_features(model, ids, device, fb)
        if valid is not None:
            valid = (cache_features(model, valid[0], device, fb), valid[1])
        torch.cuda.synchronize(device)
        feature_runtime = time.time() - t_pass
        n_valid = 0 if valid is None else int(valid[0].shape[0])
        cache_bytes = (len(ids) + n_valid) * 2 * int(model.config.d_model) * 4
        logger.info("Training on cached trunk features (%s=cache): %d training + %d validation windows through the inference engine in blocks "
                    "of %d (%s), %.3f s; the cache holds %d bytes on %s; no trunk forward runs after this", FEATURES_ENV, len(ids), n_valid, fb,
                    FEATURE_BATCH_ENV, feature_runtime, cache_bytes, device)
        model.feature_engine().release_workspace()
        tr = FeatureTrainer(model, opt, source, a, total, features, valid, rank, world)
    else:
        tr = FinetuneTrainer(model, opt, source, a, total, valid, rank, world)
    if resume_from_checkpoint:
        logger.info("Resuming training from checkpoint: %s", resume_from_checkpoint)
        tr.resume(resume_from_checkpoint)
    if rank == 0:
        os.makedirs(output_dir, exist_ok=True)
    ddp.barrier()
    first, t0 = tr.step, time.time()
    tr.run()
    torch.cuda.synchronize(device)
    runtime = time.time() - t0
    if reducer is not None:
        ddp.check_in_step(tr.masters(), tr.step)
    if rank == 0:
        model.save_adapter(output_dir, model_name)
    done = tr.step - first
    windows = done * train_batch_size * gradient_accumulation_steps * world      # the windows of all ranks
    metrics = {"epoch": tr.epoch(), "train_loss": float(tr.total_loss) / max(1, tr.step), "train_runtime": round(runtime, 4),
               "train_samples": int(source.n), "train_samples_per_second": round(windows / runtime, 3) if runtime > 0 else 0.0,
               "train_steps_per_second": round(done / runtime, 3) if runtime > 0 else 0.0, "skipped_steps": opt.state()["skipped"]}
    if cached:
        metrics["feature_pass_runtime"] = round(feature_runtime, 4)
        metrics["feature_windows"] = int(len(ids) + (0 if valid is None else valid[0].shape[0]))      # over all ranks
    if rank == 0:
        pretrain._write_json(os.path.join(output_dir, "train_results.json"), metrics)
        pretrain._write_json(os.path.join(output_dir, "trainer_state.json"), tr.trainer_state())
        print(metrics, flush=True)
    ddp.shutdown()
    return metrics


# ---------------------------------------------------------------------------------------------------------------------
def _bool(v) -> bool:
    if isinstance(v, bool):
        return v
    if str(v).lower() in ("1", "true", "yes", "y"):
        return True
    if str(v).lower() in ("0", "false", "no", "n"):
        return False
    raise ValueError(f"not a boolean: {v!r}")


# the reference train()'s flags (name, type, default) as this command takes them; bf16 defaults to False here (module docstring)
TRAIN_FLAGS = (("train_dir", str, None), ("valid_dir", str, None), ("output_dir", str, "/tmp/pcv2-ft"), ("model_name", str, None),
               ("task_type", str, "classification"), ("num_labels", int, None), ("train_batch_size", int, 43), ("eval_batch_size", int, 3),
               ("eval_num_samples", int, 0), ("max_steps", int, 500), ("seed", int, 42), ("use_wandb", _bool, False),
               ("learning_rate", float, 1e-3), ("warmup_steps", int, 50), ("lr_scheduler_type", str, "linear"),
               ("gradient_accumulation_steps", int, 64), ("bf16", _bool, False), ("num_train_epochs", float, 3), ("weight_decay", float, 0.01),
               ("eval_strategy", str, "steps"), ("eval_steps", int, 25), ("save_strategy", str, "steps"), ("save_steps", int, 100),
               ("logging_steps", int, 100), ("resume_from_checkpoint", str, None),
               # this project's additions
               ("device", str, "cuda:0"), ("pooling", str, "mean"), ("train_lora", int, 1), ("max_grad_norm", float, 1.0),
               ("lora_dropout", float, 0.0))


def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="lora_predict", description="Fine-tuned PlantCAD2 (LoRA adapter) inference on the MI355X engine")
    sub = p.add_subparsers(dest="cmd", required=True)

    def flag(q, name, **kw):
        q.add_argument("--" + name, *(["--" + name.replace("_", "-")] if "_" in name else []), dest=name, **kw)

    q = sub.add_parser("tokenize")
    for f in ("data_dir", "output_path", "model_name", "hf_dataset", "hf_config"):
        flag(q, f, default=None)
    flag(q, "sequence_length", type=int, default=8192)
    flag(q, "batch_size", type=int, default=1000)
    flag(q, "max_batches", type=int, default=None)
    flag(q, "num_proc", type=int, default=None)
    flag(q, "task_type", default="classification", choices=TASK_TYPES)
    flag(q, "hf_split", default="train")
    flag(q, "seq_column", default="sequence")
    flag(q, "label_column", default="label")
    q = sub.add_parser("train")
    for name, ty, default in TRAIN_FLAGS:
        flag(q, name, type=ty, default=default, required=name in ("train_dir", "valid_dir"),
             **({"choices": TASK_TYPES} if name == "task_type" else {}))
    for name in ("predict", "evaluate"):
        q = sub.add_parser(name)
        flag(q, "checkpoint_dir", required=True)
        flag(q, "data_dir", required=True)
        if name == "predict":
            flag(q, "output_file", default="/tmp/predictions.csv")
        else:
            flag(q, "output_dir", default="/tmp/pcv2-ft-eval")
        flag(q, "model_name", default=None)
        flag(q, "task_type", default="classification", choices=TASK_TYPES)
        flag(q, "num_labels", type=int, default=None)
        flag(q, "batch_size", type=int, default=32)
        flag(q, "sampling_rate", type=float, default=None)
        flag(q, "seed", type=int, default=42)
        flag(q, "device", default="cuda:0")
        flag(q, "dtype", default="float32", choices=("float32", "bfloat16"))
        flag(q, "pooling", default="mean", choices=("mean", "max", "first", "last"))
        flag(q, "lora_deltas", default="auto", choices=("auto", "ignore", "apply"))
    return p


def main(argv: Optional[Sequence[str]] = None):
    a = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    kw = {k: v for k, v in vars(a).items() if k != "cmd"}
    if a.cmd == "tokenize":
        return tokenize(**kw)
    if a.cmd == "train":
        return train(**kw)
    kw["device"] = sharding.init_from_env(a.device)
    try:
        return predict(**kw) if a.cmd == "predict" else evaluate(**kw)
    finally:
        sharding.shutdown()


if __name__ == "__main__":
    main()
