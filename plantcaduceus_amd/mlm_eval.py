"""Masked-LM loss and perplexity of a checkpoint: the `--do_eval` / `--do_test` half of the reference's `src/HF_pre_train.py`
(:455-471, :503-532: `trainer.evaluate()` / `trainer.predict()`, `perplexity = exp(eval_loss)`), on the MI355X engine:

    python -m plantcaduceus_amd.mlm_eval --model_name_or_path <snapshot> --dataset_name <dir> --do_eval --output_dir out
    torchrun --nproc-per-node 8 -m plantcaduceus_amd.mlm_eval ... --do_eval --do_test --soft_masked_loss_weights_evaluation 0.0

Flags keep the reference's names.  `--dataset_name` is a hub id in the local `datasets` cache, a local directory holding
`validation.*` / `test.*` tables (parquet / tsv / csv), or one such table (used for whichever split is asked for); the table needs a
`seq` column.  Additions: `--dtype` (float32 runs with "f32_gemm_split" 1, the project's parity configuration, as
`lora_predict`), `--device`, `--token-nll-out FILE.npy` (the per-base surprisal track, fp32 [N, L], 0 where no label).

What is computed:
  * masking: `transformers.DataCollatorForLanguageModeling.torch_mask_tokens` itself (15 % of the positions; 80 % [MASK], 10 % a random
    token, 10 % kept; labels -100 elsewhere), on the CPU generator after `set_seed(--seed)`, once per LOSS BATCH of
    `--per_device_eval_batch_size` windows in dataset order.  The masks are a function of (seed, batch size, data) only - not of
    the number of ranks or the engine's batch.  They are NOT bit-equal to a reference run's: there the generator has been advanced by
    the model set-up before the first batch is drawn.
  * loss_weights: 1, and `--soft_masked_loss_weights_evaluation` / `_test` at lower-case (soft-masked, repeat) bases (:424-437).
  * per loss batch: loss = sum(w nll) / sum(w) over its labelled positions (the public Caduceus model code's weighted cross entropy,
    recalled); `eval_loss` = the mean over windows of their loss batch's loss, which is what `Trainer.evaluation_loop` forms (each
    batch's loss repeated batch-size times, concatenated, mean).  The engine returns per-window sums (`pcad_forward_loss`), so its
    own batch is free: windows run in `preferred_batch_size` calls and are regrouped into loss batches on the host.
  * also reported: `eval_loss_token_mean` = the global sum(w nll) / sum(w), `eval_token_accuracy` = arg-max hits / labelled
    positions, `eval_samples`, `perplexity = exp(eval_loss)`.
Under torchrun the windows are block-sharded over the ranks (sharding.py), one all-gather of the [n, 4] sums per chunk, rank 0
writes.  `--do_train` is not provided: this is an inference engine.
"""
from __future__ import annotations

import json
import logging
import math
import os
from typing import Dict, Optional, Sequence, Tuple

import numpy as np
import torch

from . import sharding
from .plantcad2_eval import _sharded_rows

logger = logging.getLogger(__name__)

SPLITS = {"eval": "validation", "test": "test"}


# ---------------------------------------------------------------------------------------------------------------------
# data
def _read_table(path: str):
    import pandas as pd
    if path.endswith(".parquet"):
        return pd.read_parquet(path)
    return pd.read_csv(path, sep="\t" if path.endswith((".tsv", ".txt")) else ",")


def load_sequences(dataset_name: str, split: str, dataset_config_name: Optional[str] = None) -> list:
    """The `seq` column of one split (`validation` / `test`): a local table, a local directory with `<split>.parquet|tsv|csv`
    (or `<split>/` holding such files), or a `datasets` hub id resolved from the local cache only."""
    if os.path.isfile(dataset_name):
        df = _read_table(dataset_name)
    elif os.path.isdir(dataset_name):
        import pandas as pd
        found = [os.path.join(dataset_name, split + ext) for ext in (".parquet", ".tsv", ".csv", ".txt")]
        found = [f for f in found if os.path.isfile(f)]
        sub = os.path.join(dataset_name, split)
        if not found and os.path.isdir(sub):
            found = sorted(os.path.join(sub, f) for f in os.listdir(sub) if f.endswith((".parquet", ".tsv", ".csv", ".txt")))
        if not found:
            raise FileNotFoundError(f"{dataset_name} holds no {split}.parquet / .tsv / .csv table (nor a {split}/ directory of them)")
        df = pd.concat([_read_table(f) for f in found], ignore_index=True)
    else:
        os.environ.setdefault("HF_DATASETS_OFFLINE", "1")        # the local datasets cache only
        os.environ.setdefault("HF_HUB_OFFLINE", "1")
        from datasets import load_dataset
        df = load_dataset(dataset_name, dataset_config_name, split=split).to_pandas()
    if "seq" not in df.columns:
        raise KeyError(f"the {split} split of {dataset_name} has no 'seq' column (columns: {list(df.columns)})")
    return [str(s) for s in df["seq"]]


def tokenize_windows(tokenizer, seqs: Sequence[str], soft_masked_weight: float) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
    """-> (input_ids int64 [N, L], special_tokens_mask bool [N, L], loss_weights fp32 [N, L]): the reference's tokenize_function
    (:424-437: weight 1, `soft_masked_weight` at lower-case characters).  Windows of unequal length are refused (the reference's
    collator stacks them without padding)."""
    lens = sorted({len(s) for s in seqs})
    if len(lens) > 1:
        raise ValueError(f"windows of unequal length {lens[:4]}{'...' if len(lens) > 4 else ''}: masked-LM evaluation needs "
                         "equal-length windows (the reference's collator assumes it)")
    n, L = len(seqs), (lens[0] if lens else 0)
    ids = np.asarray(tokenizer.encode_batch(list(seqs)), dtype=np.int64).reshape(n, L) if n else np.zeros((0, 0), np.int64)
    chars = np.frombuffer("".join(seqs).encode("ascii", "replace"), dtype=np.uint8).reshape(n, L)
    lower = (chars >= ord("a")) & (chars <= ord("z"))
    w = np.ones((n, L), dtype=np.float32)
    w[lower] = np.float32(soft_masked_weight)
    special = np.isin(ids, np.asarray(sorted(set(tokenizer.all_special_ids)), dtype=np.int64))
    return ids, special, w


def make_collator(tokenizer, mlm_probability: float = 0.15):
    from transformers import DataCollatorForLanguageModeling
    return DataCollatorForLanguageModeling(tokenizer=tokenizer, mlm=True, mlm_probability=mlm_probability)


def mask_windows(collator, ids: np.ndarray, special: np.ndarray, batch_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """`collator.torch_mask_tokens` once per loss batch of `batch_size` windows, in dataset order, on torch's global CPU generator
    (seed it with `transformers.set_seed` first) -> (masked input_ids int32 [N, L], labels int32 [N, L], -100 off the masked set)."""
    n = ids.shape[0]
    out_ids = np.empty(ids.shape, dtype=np.int32)
    labels = np.empty(ids.shape, dtype=np.int32)
    for b0 in range(0, n, max(1, batch_size)):
        b1 = min(b0 + batch_size, n)
        x, y = collator.torch_mask_tokens(torch.from_numpy(ids[b0:b1].copy()),
                                          special_tokens_mask=torch.from_numpy(special[b0:b1].copy()))
        out_ids[b0:b1] = x.numpy()
        labels[b0:b1] = y.numpy()
    return out_ids, labels


# ---------------------------------------------------------------------------------------------------------------------
# host arithmetic on the per-window sums
def regroup_losses(sums: np.ndarray, batch_size: int) -> Tuple[np.ndarray, np.ndarray]:
    """Per-window sums [N, >= 2] (sum w nll, sum w) -> (loss of every loss batch of `batch_size` consecutive windows (the last
    one may be short) = sum of its windows' sum w nll / sum of their sum w, in float64, nan for a batch without weight; windows
    per batch)."""
    s = np.asarray(sums, dtype=np.float64)
    n = s.shape[0]
    starts = np.arange(0, n, max(1, batch_size))
    counts = np.minimum(starts + batch_size, n) - starts
    num = np.add.reduceat(s[:, 0], starts) if n else np.zeros(0)
    den = np.add.reduceat(s[:, 1], starts) if n else np.zeros(0)
    with np.errstate(divide="ignore", invalid="ignore"):
        return num / den, counts


def trainer_eval_loss(sums: np.ndarray, batch_size: int) -> float:
    """`Trainer.evaluation_loop`'s `eval_loss`: every loss batch's loss repeated once per window of the batch, concatenated, mean."""
    losses, counts = regroup_losses(sums, batch_size)
    if len(losses) == 0:
        return float("nan")
    return float(np.repeat(losses, counts).mean())


def metrics_from_sums(sums: np.ndarray, batch_size: int, prefix: str) -> Dict[str, float]:
    s = np.asarray(sums, dtype=np.float64).reshape(-1, 4)
    loss = trainer_eval_loss(s, batch_size)
    try:
        ppl = math.exp(loss)
    except OverflowError:
        ppl = float("inf")
    with np.errstate(divide="ignore", invalid="ignore"):
        tok_mean = float(s[:, 0].sum() / s[:, 1].sum()) if len(s) else float("nan")
        acc = float(s[:, 3].sum() / s[:, 2].sum()) if len(s) else float("nan")
    return {f"{prefix}_loss": loss, "perplexity": ppl, f"{prefix}_samples": int(len(s)), f"{prefix}_token_accuracy": acc,
            f"{prefix}_loss_token_mean": tok_mean, f"{prefix}_labelled_tokens": int(s[:, 2].sum())}


# ---------------------------------------------------------------------------------------------------------------------
# model
def load_model_and_tokenizer(model_name_or_path: str, tokenizer_name: Optional[str], device: str, dtype: str = "float32"):
    from transformers import AutoModelForMaskedLM, AutoTokenizer
    from . import register
    from .checkpoint import resolve_snapshot
    register()
    td = {"float32": torch.float32, "bfloat16": torch.bfloat16}[dtype]
    path = resolve_snapshot(model_name_or_path)
    tok = AutoTokenizer.from_pretrained(resolve_snapshot(tokenizer_name) if tokenizer_name else path)
    model = AutoModelForMaskedLM.from_pretrained(path)
    if td == torch.float32:      # the project's parity configuration for fp32 numbers (packed at bind time: set before the engine exists)
        opts = dict(getattr(model.config, "engine_options", None) or {})
        opts.setdefault("f32_gemm_split", 1)
        model.config.engine_options = opts
    return model.to(td).to(device).eval(), tok


def window_sums(model, ids: np.ndarray, labels: np.ndarray, weights: np.ndarray, device: str, engine_batch: Optional[int] = None,
                want_nll: bool = False) -> Tuple[np.ndarray, Optional[np.ndarray]]:
    """The model's per-window sums fp32 [N, 4] (and token nll fp32 [N, L]) in window order, sharded over the ranks of a process group.
    The model is called as `model(input_ids=, labels=, loss_weights=, output_logits=False, return_window_sums=True[,
    return_token_nll=True])` (CaduceusForMaskedLM: the engine's fused loss head)."""
    from .zero_shot import check_model_inputs
    n, L = ids.shape
    if engine_batch is None:
        engine_batch = int(model.preferred_batch_size(L)) if hasattr(model, "preferred_batch_size") else 32
    engine_batch = max(1, engine_batch)
    width = 4 + (L if want_nll else 0)
    t_ids, t_lab, t_w = (torch.from_numpy(np.ascontiguousarray(a)) for a in (ids, labels, weights))

    def run_rows(lo, hi):
        if hi <= lo:
            return torch.zeros((0, width), dtype=torch.float32, device=device)
        parts = []
        for b0 in range(lo, hi, engine_batch):
            b1 = min(b0 + engine_batch, hi)
            out = model(input_ids=t_ids[b0:b1].to(device), labels=t_lab[b0:b1].to(device), loss_weights=t_w[b0:b1].to(device),
                        output_logits=False, return_window_sums=True, return_token_nll=want_nll)
            s = out["window_sums"].float()
            parts.append(torch.cat([s, out["token_nll"].float()], dim=1) if want_nll else s)
        return torch.cat(parts, dim=0)

    out = np.zeros((n, width), dtype=np.float32)
    with torch.inference_mode():
        _sharded_rows(n, run_rows, out)
    check_model_inputs(model)
    return out[:, :4], (out[:, 4:] if want_nll else None)


def evaluate_split(model, tokenizer, seqs: Sequence[str], prefix: str, soft_masked_weight: float = 1.0, mlm_probability: float = 0.15,
                   batch_size: int = 8, seed: int = 42, max_samples: Optional[int] = None, device: str = "cuda:0",
                   engine_batch: Optional[int] = None, token_nll_out: Optional[str] = None) -> Dict[str, float]:
    from transformers import set_seed
    if max_samples is not None:
        seqs = list(seqs)[:max(0, int(max_samples))]
    ids, special, w = tokenize_windows(tokenizer, seqs, soft_masked_weight)
    set_seed(seed)
    masked, labels = mask_windows(make_collator(tokenizer, mlm_probability), ids, special, batch_size)
    sums, nll = window_sums(model, masked, labels, w, device, engine_batch, want_nll=token_nll_out is not None)
    if nll is not None and sharding.world()[0] == 0:
        np.save(token_nll_out, nll)
    return metrics_from_sums(sums, batch_size, prefix)


# ---------------------------------------------------------------------------------------------------------------------
def build_parser():
    import argparse
    p = argparse.ArgumentParser(prog="mlm_eval", description="Masked-LM loss / perplexity of a checkpoint on the MI355X engine "
                                                             "(src/HF_pre_train.py --do_eval / --do_test)")
    p.add_argument("--model_name_or_path", required=True)
    p.add_argument("--tokenizer_name", default=None)
    p.add_argument("--dataset_name", required=True)
    p.add_argument("--dataset_config_name", default=None)
    p.add_argument("--do_eval", action="store_true")
    p.add_argument("--do_test", action="store_true")
    p.add_argument("--do_train", action="store_true", help="not provided: this is an inference engine")
    p.add_argument("--mlm_probability", type=float, default=0.15)
    p.add_argument("--soft_masked_loss_weights_evaluation", type=float, default=1.0)
    p.add_argument("--soft_masked_loss_weights_test", type=float, default=1.0)
    p.add_argument("--max_eval_samples", type=int, default=None)
    p.add_argument("--per_device_eval_batch_size", type=int, default=8)
    p.add_argument("--seed", type=int, default=42)
    p.add_argument("--output_dir", required=True)
    p.add_argument("--dtype", default="float32", choices=("float32", "bfloat16"))
    p.add_argument("--device", default="cuda:0")
    p.add_argument("--engine_batch_size", type=int, default=None, help="windows per engine call (default: the model's preferred batch)")
    p.add_argument("--token-nll-out", "--token_nll_out", dest="token_nll_out", default=None)
    return p


def main(argv: Optional[Sequence[str]] = None) -> Dict[str, Dict[str, float]]:
    a = build_parser().parse_args(argv)
    logging.basicConfig(level=logging.INFO, format="%(asctime)s %(levelname)s %(message)s")
    if a.do_train:
        raise SystemExit("--do_train is not provided: this is an inference engine (no backward pass)")
    if not (a.do_eval or a.do_test):
        raise SystemExit("nothing to do: pass --do_eval and / or --do_test")
    if a.per_device_eval_batch_size < 1:
        raise SystemExit("--per_device_eval_batch_size must be >= 1")
    device = sharding.init_from_env(a.device)
    results = {}
    try:
        model, tok = load_model_and_tokenizer(a.model_name_or_path, a.tokenizer_name, device, a.dtype)
        for prefix, on, soft in (("eval", a.do_eval, a.soft_masked_loss_weights_evaluation),
                                 ("test", a.do_test, a.soft_masked_loss_weights_test)):
            if not on:
                continue
            seqs = load_sequences(a.dataset_name, SPLITS[prefix], a.dataset_config_name)
            nll_out = a.token_nll_out
            if nll_out and a.do_eval and a.do_test:
                root, ext = os.path.splitext(nll_out)
                nll_out = f"{root}.{prefix}{ext}"
            res = evaluate_split(model, tok, seqs, prefix, soft, a.mlm_probability, a.per_device_eval_batch_size, a.seed,
                                 a.max_eval_samples if prefix == "eval" else None, device, a.engine_batch_size, nll_out)
            results[prefix] = res
            if sharding.world()[0] == 0:
                os.makedirs(a.output_dir, exist_ok=True)
                with open(os.path.join(a.output_dir, f"{prefix}_results.json"), "w") as f:
                    json.dump(res, f, indent=4, sort_keys=True)
                print(json.dumps(res, sort_keys=True), flush=True)
    finally:
        sharding.shutdown()
    return results


if __name__ == "__main__":
    main()
