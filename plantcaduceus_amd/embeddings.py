"""Embedding extraction — host side of the hot path, mirroring reference `src/train_XGBoost.py`
(`extract_embeddings` :96-114, `SequenceDataset` :29-49, `load_data` :51-54; `predict_XGBoost.py`
reaches the same function through `from train_XGBoost import *`).

  extract_embeddings(model, sequences, device, tokenIdx, tokenizer, batch_size)
      forward with output_hidden_states=True, hidden_states[-1][:, tokenIdx, :] -> fp32,
      forward half + channel-reversed rc half, / 2                                   -> fp32 [N, d_model]

Host-side differences only: whole-list vectorised tokenisation (no masking on this path), the model is
asked for position tokenIdx only (hidden [B,1,2D] instead of 33 x [B,512,2D]), the averaging runs on the
device, and under torch.distributed the window list is block-sharded and the [N, D] result reassembled with
one all-gather per call (= one `-chunk_size` chunk of the reference's -save_memory mode, :175-190).
The XGBoost fit/predict and the ROC/PR plots of the reference script are CPU tree-model code and are out of
scope; `save_embedding_cache` keeps the reference's .npz keys so they run unchanged.
"""
from __future__ import annotations

import logging
import os

import numpy as np
import torch

from . import sharding
from .zero_shot import _window_len, check_model_inputs, effective_batch, iter_device_batches, local_ids


def load_data(filepath):
    import pandas as pd
    logging.info(f"Loading data from {filepath}")
    data = pd.read_csv(filepath, delimiter="\t")
    return data["sequences"].tolist(), data["label"].tolist()


def resolve_layers(layer, n_layer: int):
    """`layer` (an int or a list of ints; negative counts from the end, as indexing the n_layer + 1 entries of `hidden_states`
    would) -> the levels as non-negative ints, in the caller's order."""
    out = []
    for k in ([layer] if isinstance(layer, (int, np.integer)) else list(layer)):
        k = int(k)
        if not -(n_layer + 1) <= k <= n_layer:
            raise IndexError(f"layer {k} is outside the {n_layer + 1} levels of hidden_states")
        out.append(k + n_layer + 1 if k < 0 else k)
    if not out:
        raise ValueError("layer: an empty list")
    return out


def with_layer(name: str, layer) -> str:
    """File name of a cache / result of `-layer K` runs: `_layer<K>` before the extension (layer None: the name as it is), so that
    caches of different layers never collide with each other or with the default run's."""
    if layer is None:
        return name
    stem, ext = os.path.splitext(name)
    return f"{stem}_layer{int(layer)}{ext}"


def layer_arg(value: str) -> int:
    """argparse type of `-layer K`: a level of `hidden_states`, 0 (the embedding output) .. n_layer (the last hidden state)."""
    k = int(value)
    if k < 0:
        raise ValueError("-layer counts from 0 (the embedding output); the last level is n_layer")
    return k


def extract_embeddings(model, sequences, device, tokenIdx: int, tokenizer=None, batch_size: int = 128,
                       batch_explicit: bool = False, layer=None) -> np.ndarray:
    """layer=None: the reference's embedding, from hidden_states[-1].  layer=K / [K, ...] (negative: from the end): the same
    strand-averaged fp32 embedding of level K of `hidden_states` -> [N, d_model] / [N, NL, d_model], formed on the device by
    `model.hidden_states_at(..., average=True)` (models with `supports_layer_hidden`)."""
    if layer is not None:
        return _extract_layer_embeddings(model, sequences, device, tokenIdx, tokenizer, batch_size, batch_explicit, layer)
    logging.info("Extracting embeddings")
    n_total = len(sequences)
    rank, ws = sharding.world()
    start, stop, per = sharding.shard_bounds(n_total, rank, ws)            # only this rank's block is tokenised
    fast = bool(getattr(model, "supports_positions", False))
    if fast and n_total:
        batch_size = effective_batch(model, batch_size, _window_len(sequences), batch_explicit)
    model.eval()
    outs = []
    with torch.inference_mode():
        for cur in iter_device_batches(sequences, start, stop, per if ws > 1 else 0, batch_size, tokenizer, None, device):
            if fast:
                e = model(input_ids=cur, output_hidden_states=True, positions=[tokenIdx]).hidden_states[-1][:, 0, :]
            else:
                e = model(input_ids=cur, output_hidden_states=True).hidden_states[-1][:, tokenIdx, :]
            e = e.to(torch.float32)
            hsz = e.shape[-1] // 2
            outs.append((e[:, :hsz] + torch.flip(e[:, hsz:], dims=[-1])) / 2)
        if outs:
            emb = torch.cat(outs, dim=0)
        else:
            d = getattr(getattr(model, "config", None), "d_model", 0)
            emb = torch.empty((0, d), dtype=torch.float32, device=device)
        emb = sharding.all_gather_rows(emb, n_total)
    out = emb.cpu().numpy()
    check_model_inputs(model)
    return out


def _extract_layer_embeddings(model, sequences, device, tokenIdx, tokenizer, batch_size, batch_explicit, layer) -> np.ndarray:
    if not getattr(model, "supports_layer_hidden", False):
        raise NotImplementedError("layer=: the model has no hidden_states_at (supports_layer_hidden); intermediate levels of another "
                                  "model are read from model(..., output_hidden_states=True).hidden_states")
    n_layer = int(model.config.n_layer)
    levels = resolve_layers(layer, n_layer)
    single = isinstance(layer, (int, np.integer))
    order = sorted(set(levels))                     # the engine takes strictly increasing levels; the caller's order is restored below
    pick = [order.index(k) for k in levels]
    logging.info(f"Extracting embeddings of hidden_states level(s) {levels}")
    n_total = len(sequences)
    rank, ws = sharding.world()
    start, stop, per = sharding.shard_bounds(n_total, rank, ws)
    if n_total:
        batch_size = effective_batch(model, batch_size, _window_len(sequences), batch_explicit)
    model.eval()
    d = int(model.config.d_model)
    outs = []
    with torch.inference_mode():
        for cur in iter_device_batches(sequences, start, stop, per if ws > 1 else 0, batch_size, tokenizer, None, device):
            e = model.hidden_states_at(cur, layers=order, positions=[tokenIdx], average=True)          # fp32 [NLu, b, 1, D]
            outs.append(e[:, :, 0, :].permute(1, 0, 2)[:, pick, :].reshape(e.shape[1], len(pick) * d))
        emb = torch.cat(outs, dim=0) if outs else torch.empty((0, len(pick) * d), dtype=torch.float32, device=device)
        emb = sharding.all_gather_rows(emb, n_total)     # one gather of the rows flattened to [N, NL * D]
    out = emb.cpu().numpy()
    check_model_inputs(model)
    return out if single else out.reshape(n_total, len(pick), d)


def save_embedding_cache(path: str, compresslevel: int = 1, **arrays):
    """The reference's cache file (`np.savez_compressed` with keys `train`, `valid`, `test`: src/train_XGBoost.py:186,199,221),
    readable by `np.load` exactly as the reference reads it, written with a chosen deflate level (0 = stored).  fp32 embeddings
    hardly compress (7 %) and deflate runs at ~20 MB/s on one core at any level (2.3 s at level 1, 2.8 s at numpy's default, for
    the 51 MB of one rank's share of a chunk; 6 s on the GPU box's slower cores, profiles/r03_e2e_embed.json), so callers that
    extract chunk after chunk write the file on a worker thread while the next chunk runs (xgb_predict.py)."""
    import zipfile
    bad = set(arrays) - {"train", "valid", "test"}
    if bad:
        raise ValueError(f"unexpected cache keys {sorted(bad)}")
    if not path.endswith(".npz"):
        path = path + ".npz"                       # np.savez_compressed appends the suffix the same way
    comp = zipfile.ZIP_DEFLATED if compresslevel > 0 else zipfile.ZIP_STORED
    # written beside the final name and renamed once the archive is closed: a run that dies mid-write (the writer may be a
    # background thread that lives for a whole chunk's compute time) leaves a .tmp file, never a truncated cache that the next
    # run would find with os.path.exists() and fail to read
    tmp = path + ".tmp"
    try:
        with zipfile.ZipFile(tmp, "w", compression=comp, compresslevel=compresslevel if compresslevel > 0 else None, allowZip64=True) as zf:
            for key, arr in arrays.items():
                with zf.open(key + ".npy", "w", force_zip64=True) as f:
                    np.lib.format.write_array(f, np.asanyarray(arr), allow_pickle=False)
        os.replace(tmp, path)
    except BaseException:
        try:
            os.unlink(tmp)
        except OSError:
            pass
        raise
