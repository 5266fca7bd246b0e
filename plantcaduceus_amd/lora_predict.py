"""The inference commands of the reference's `src/lora_fine_tune.py` - `tokenize` (:43-170), `evaluate` (:356-413) and
`predict` (:415-499) - for the released fine-tuned PlantCAD2 models (LoRA adapters over the PlantCAD2 trunks), on the MI355X
engine:

    python -m plantcaduceus_amd.lora_predict tokenize --data_dir x.tsv --model_name <base> --sequence_length 8192 --output_path x.parquet
    python -m plantcaduceus_amd.lora_predict predict  --checkpoint_dir <adapter> --data_dir x.parquet --task_type classification
    python -m plantcaduceus_amd.lora_predict evaluate --checkpoint_dir <adapter> --data_dir x.parquet --task_type multi_label --num_labels 92

Flags keep the reference's names (both `_` and `-` spellings; `fire` is not used).  Additions: `--dtype` (float32, the
reference's dtype - it passes none to from_pretrained - runs with "f32_gemm_split" 1, the project's parity configuration;
bfloat16), `--pooling` (the head's pooling_strategy, default mean) and `--lora-deltas` (adapters.load_adapter).  `--model_name`
overrides the adapter's base_model_name_or_path.  Hub ids resolve from local files / the HF cache only.

Under torchrun the windows are sharded over the ranks (plantcad2_eval._sharded_rows); rank 0 writes / prints.  Metrics are
computed on the host without sklearn (the reference's compute_metrics_* :517-563 restated; pinned against sklearn / scipy in
tests/test_seqcls.py).
"""
from __future__ import annotations

import logging
import os
import time
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import sharding
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
    kw["device"] = sharding.init_from_env(a.device)
    try:
        return predict(**kw) if a.cmd == "predict" else evaluate(**kw)
    finally:
        sharding.shutdown()


if __name__ == "__main__":
    main()
