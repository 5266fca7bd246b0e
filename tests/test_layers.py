"""Per-layer hidden states at the evaluated positions (csrc/layers.hip), the parts that need no GPU: the C ABI's
declarations, exports and argument checks, and the host side - extract_embeddings(layer=...) and the `-layer` file names of the
XGBoost commands - driven by a stand-in model that implements `hidden_states_at` on the CPU from the literal oracle's tuple."""
import ctypes as C
import os
import re
import socket
import subprocess
import sys
import types

import numpy as np
import pandas as pd
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from oracle import caduceus_oracle as O
from plantcaduceus_amd import embeddings, engine, sharding, xgb_predict, xgb_train, zero_shot
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_LAYER, D_MODEL, L_WIN, TOKEN = 3, 32, 24, 11


def test_header_declares_and_library_exports_the_layers_entries():
    hdr = open(os.path.join(ROOT, "include", "pcad.h")).read()
    for name in ("pcad_forward_layers", "pcad_layer_rows"):
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert name in engine.SIGNATURES
    lib = engine.load_library()
    for name in ("pcad_forward_layers", "pcad_layer_rows"):
        assert hasattr(lib, name), name
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T pcad_forward_layers" in syms and " T pcad_layer_rows" in syms


def test_layers_abi_validates_without_gpu():
    """PCAD_ERR_INVALID before any launch: levels that do not increase or lie outside [0, n_layer], both position forms or none,
    P of 0 or 17, a missing output; pcad_workspace_bytes is what it was before the call existed."""
    from test_mlm_eval import WORKSPACE_BYTES, _handle
    lib = engine.load_library()
    h = _handle(lib, 128, 0)                # n_layer 2
    i4 = lambda *v: (C.c_int32 * len(v))(*v)
    INVALID = -1                            # include/pcad.h PCAD_ERR_INVALID
    one = C.c_void_p(256)                   # never dereferenced: every call below is refused while its arguments are checked
    try:
        call = lambda pos, P, ppw, lay, NL, out=one: lib.pcad_forward_layers(h, one, 2, 32, pos, P, ppw, lay, NL, 0, out, one, 1 << 20, None)
        assert call(i4(1, 2), 2, None, i4(1, 1), 2) == INVALID          # not strictly increasing
        assert call(i4(1, 2), 2, None, i4(2, 1), 2) == INVALID
        assert call(i4(1, 2), 2, None, i4(0, 3), 2) == INVALID          # level 3 of a 2-layer model
        assert call(i4(1, 2), 2, None, i4(-1), 1) == INVALID
        assert call(i4(1, 2), 2, None, i4(0, 1, 2, 2), 4) == INVALID    # more levels than the tuple has
        assert call(i4(1, 2), 2, None, None, 2) == INVALID              # a count without a list
        assert call(i4(1, 2), 2, None, i4(1), 0) == INVALID             # a list without a count
        assert call(i4(1, 2), 2, one, i4(1), 1) == INVALID              # both position forms
        assert call(None, 2, None, i4(1), 1) == INVALID                 # neither
        assert call(None, 0, one, i4(1), 1) == INVALID                  # P == 0
        assert call(None, 17, one, i4(1), 1) == INVALID                 # P > PCAD_MAX_POSITIONS
        assert call(i4(1, 2), 2, None, i4(1), 1, None) == INVALID       # no output
        # well-formed arguments get past the checks: the next refusal is the unbound handle's
        assert call(i4(1, 2), 2, None, i4(0, 2), 2) == -2 and call(None, 16, one, None, 0) == -2          # PCAD_ERR_UNBOUND
        rows = lambda pos, P, ppw: lib.pcad_layer_rows(one, one, 2, 32, 64, pos, P, ppw, 0, 0, None, 0, None)
        assert rows(i4(1, 2), 2, one) == INVALID
        assert rows(None, 2, None) == INVALID
        assert rows(None, 17, one) == INVALID and rows(None, 0, one) == INVALID
        assert rows(i4(1, 32), 2, None) == INVALID                      # a shared position outside the window
        assert lib.pcad_layer_rows(one, one, 2, 32, 60, i4(1), 1, None, 0, 0, None, 0, None) == INVALID      # D % 8
    finally:
        lib.pcad_destroy(h)
    for (D, dt, split, B, L), want in WORKSPACE_BYTES.items():
        h = _handle(lib, D, dt, split)
        got = lib.pcad_workspace_bytes(h, B, L)
        lib.pcad_destroy(h)
        assert got == want, (D, dt, split, B, L, got)


# ---- host side: a stand-in with hidden_states_at ------------------------------------------------------------------------------
class _Out:
    def __init__(self, hidden_states):
        self.hidden_states = hidden_states


class TupleStandIn:
    """`.hidden_states` only (no supports_layer_hidden, no supports_positions): the full tuple of the literal oracle, every window run
    on its own so that a window's numbers do not depend on the batch or the rank it is evaluated in."""

    def __init__(self):
        cfg = make_config("x", d_model=D_MODEL, n_layer=N_LAYER)
        self.P = O.params_from_state_dict(synthetic_state_dict(cfg, seed=5), cfg)
        self.config = cfg
        self.calls = []

    def eval(self):
        return self

    def _levels(self, input_ids):
        ids = input_ids.long().cpu()
        per = [O.forward_literal(ids[i:i + 1], self.P, output_hidden_states=True)["all_hidden"] for i in range(ids.shape[0])]
        return [torch.cat([w[k] for w in per], dim=0) for k in range(N_LAYER + 1)]          # n_layer + 1 x [B, L, 2D]

    def __call__(self, input_ids=None, output_hidden_states=False, **kw):
        self.calls.append(("tuple", tuple(input_ids.shape)))
        return _Out(tuple(self._levels(input_ids)))


class LayerStandIn(TupleStandIn):
    """hidden_states_at on the CPU: the engine's own argument rules (engine.check_layer_request), then rows of the oracle's tuple;
    average=True restates the reference's strand averaging."""
    supports_layer_hidden = True

    def hidden_states_at(self, input_ids, layers=None, positions=None, positions_per_window=None, average=False):
        lv, P = engine.check_layer_request(layers, N_LAYER, positions, positions_per_window, int(input_ids.shape[0]))
        levels = self._levels(input_ids)
        L = levels[0].shape[1]
        if positions is not None:
            if any(not 0 <= int(p) < L for p in positions):
                raise RuntimeError("pcad_forward_layers failed (-1): position out of range")
            idx = torch.tensor([int(p) for p in positions]).expand(input_ids.shape[0], -1)
        else:
            idx = positions_per_window.long().clamp(0, L - 1)
        rows = torch.stack([torch.gather(levels[k], 1, idx[:, :, None].expand(-1, -1, 2 * D_MODEL))
                            for k in (lv if lv is not None else range(N_LAYER + 1))])
        self.calls.append(("at", tuple(rows.shape), bool(average)))
        if not average:
            return rows
        e = rows.float()
        return (e[..., :D_MODEL] + torch.flip(e[..., D_MODEL:], dims=[-1])) / 2


def _seqs(n, seed=0):
    rng = np.random.default_rng(seed)
    return ["".join(rng.choice(list("ACGTN"), size=L_WIN, p=[.24, .24, .24, .24, .04])) for _ in range(n)]


def _want(model, seqs, level):
    """the reference's embedding arithmetic (src/train_XGBoost.py:104-113) on level `level` of the oracle's tuple, window by window"""
    ids = torch.from_numpy(zero_shot.tokenize_masked(seqs, CaduceusTokenizer(), None))
    return O.averaged_embedding(model._levels(ids)[level], TOKEN).numpy()


def test_extract_embeddings_layer_shapes_values_and_negative_index():
    tok, seqs, m = CaduceusTokenizer(), _seqs(7), LayerStandIn()
    one = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=3, layer=2)
    assert one.shape == (7, D_MODEL) and one.dtype == np.float32
    np.testing.assert_array_equal(one, _want(m, seqs, 2))
    assert all(kind == "at" and shape[0] == 1 and shape[2:] == (1, 2 * D_MODEL) and avg for kind, shape, avg in m.calls), m.calls
    lst = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=3, layer=[0, 2])
    assert lst.shape == (7, 2, D_MODEL) and lst.dtype == np.float32
    np.testing.assert_array_equal(lst[:, 0], _want(m, seqs, 0))
    np.testing.assert_array_equal(lst[:, 1], one)
    single = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=3, layer=[2])
    assert single.shape == (7, 1, D_MODEL)
    np.testing.assert_array_equal(single[:, 0], one)
    # negative levels count from the end, as indexing the tuple would; the caller's order is kept
    np.testing.assert_array_equal(embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=4, layer=-2), one)
    neg = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=4, layer=[-1, 0])
    np.testing.assert_array_equal(neg[:, 0], _want(m, seqs, N_LAYER))
    np.testing.assert_array_equal(neg[:, 1], lst[:, 0])
    with pytest.raises(IndexError):
        embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, layer=N_LAYER + 1)
    with pytest.raises(IndexError):
        embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, layer=-(N_LAYER + 2))
    with pytest.raises(NotImplementedError, match="supports_layer_hidden"):
        embeddings.extract_embeddings(TupleStandIn(), seqs, "cpu", TOKEN, tok, layer=1)
    assert embeddings.extract_embeddings(m, [], "cpu", TOKEN, tok, layer=1).shape == (0, D_MODEL)


def test_extract_embeddings_default_path_is_unchanged():
    """layer=None: today's path (the model's forward, never hidden_states_at) and today's bytes - the last level's rows averaged as
    the reference does - whether or not the model could serve the request through hidden_states_at."""
    tok, seqs = CaduceusTokenizer(), _seqs(7)
    for m in (TupleStandIn(), LayerStandIn()):
        got = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=3)
        assert got.shape == (7, D_MODEL) and got.dtype == np.float32
        assert got.tobytes() == _want(m, seqs, N_LAYER).tobytes()
        assert m.calls and all(c[0] == "tuple" for c in m.calls), m.calls
    # ... and the layer path on the last level gives those bytes too
    m = LayerStandIn()
    assert embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=3, layer=-1).tobytes() == got.tobytes()


def test_hidden_states_at_argument_validation():
    m = LayerStandIn()
    ids = torch.randint(3, 7, (3, L_WIN))
    ppw = torch.zeros(3, 2, dtype=torch.long)
    ok = m.hidden_states_at(ids, layers=[0, N_LAYER], positions=[0, L_WIN - 1, 5])
    assert ok.shape == (2, 3, 3, 2 * D_MODEL)
    assert m.hidden_states_at(ids, positions_per_window=ppw, average=True).shape == (N_LAYER + 1, 3, 2, D_MODEL)
    for bad in ([1, 1], [2, 1], [0, 1, 1]):
        with pytest.raises(ValueError, match="strictly increasing"):
            m.hidden_states_at(ids, layers=bad, positions=[1])
    for bad in ([N_LAYER + 1], [-1], [0, N_LAYER + 1]):
        with pytest.raises(ValueError, match="inside"):
            m.hidden_states_at(ids, layers=bad, positions=[1])
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[], positions=[1])
    with pytest.raises(ValueError, match="exactly one"):
        m.hidden_states_at(ids, layers=[1], positions=[1], positions_per_window=ppw)
    with pytest.raises(ValueError, match="exactly one"):
        m.hidden_states_at(ids, layers=[1])
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions=[])
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions=list(range(17)))
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions_per_window=torch.zeros(3, 17, dtype=torch.long))
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions_per_window=torch.zeros(3, 0, dtype=torch.long))
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions_per_window=torch.zeros(2, 2, dtype=torch.long))          # B rows expected
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[1], positions_per_window=torch.zeros(3, 2))                            # not integers


# ---- sharded extraction --------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _embed_worker(rank, ws, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.set_num_threads(1)
        tok, seqs, m = CaduceusTokenizer(), _seqs(11), LayerStandIn()
        one = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=2, layer=1)
        lst = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=2, layer=[0, 3, 1])
        per = sharding.shard_bounds(11, rank, ws)[2]
        assert sum(shape[1] for _, shape, _ in m.calls) == 2 * per          # its own block (padded to the common size), twice
        np.savez(os.path.join(outdir, f"w{ws}_r{rank}.npz"), one=one, lst=lst)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 4])
def test_extract_embeddings_layer_gloo_worlds_bit_equal_world_1(tmp_path, ws):
    mp.spawn(_embed_worker, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    tok, seqs, m = CaduceusTokenizer(), _seqs(11), LayerStandIn()
    one = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=2, layer=1)
    lst = embeddings.extract_embeddings(m, seqs, "cpu", TOKEN, tok, batch_size=2, layer=[0, 3, 1])
    assert one.shape == (11, D_MODEL) and lst.shape == (11, 3, D_MODEL)
    np.testing.assert_array_equal(lst[:, 2], one)
    for r in range(ws):
        got = np.load(tmp_path / f"w{ws}_r{r}.npz")
        np.testing.assert_array_equal(got["one"], one)
        np.testing.assert_array_equal(got["lst"], lst)


# ---- the -layer file names -----------------------------------------------------------------------------------------------------
def test_with_layer_names():
    assert embeddings.with_layer("train_valid_embeddings.npz", None) == "train_valid_embeddings.npz"
    assert embeddings.with_layer("train_valid_embeddings.npz", 5) == "train_valid_embeddings_layer5.npz"
    assert embeddings.with_layer("te_chunk_200_embeddings.npz", 0) == "te_chunk_200_embeddings_layer0.npz"
    assert embeddings.with_layer("seed_7_XGBoost.json", 12) == "seed_7_XGBoost_layer12.json"
    assert xgb_train.parse_args([]).layer is None and xgb_predict.parse_args([]).layer is None
    assert xgb_train.parse_args(["-layer", "3"]).layer == 3 and xgb_predict.parse_args(["-layer", "0"]).layer == 0
    with pytest.raises(SystemExit):
        xgb_predict.parse_args(["-layer", "-1"])


def test_layer_option_file_names_of_both_commands(tmp_path, monkeypatch):
    """`-layer K`: every cache and result file carries `_layer<K>`, the embeddings are level K's, and a run without the option in the
    same directory neither reads nor overwrites them (today's names)."""
    from test_xgb import _StubXGBClassifier, _model_json, _tree
    import json
    model = LayerStandIn()
    monkeypatch.setattr(zero_shot, "load_model_and_tokenizer", lambda d, dev: (model, CaduceusTokenizer()))
    paths = {}
    for name, n, labels in (("tr", 8, [0, 1] * 4), ("va", 4, [1, 0] * 2), ("te", 5, [0, 1, 1, 0, 1])):
        paths[name] = tmp_path / f"{name}.tsv"
        pd.DataFrame({"sequences": _seqs(n, seed=len(name) + n), "label": labels}).to_csv(paths[name], sep="\t", index=False)
    te = list(pd.read_csv(paths["te"], delimiter="\t")["sequences"])
    # xgb_predict
    clf = tmp_path / "clf.json"
    json.dump(_model_json([_tree([1, -1, -1], [2, -1, -1], [3, 0, 0], [0.0, -1.0, 1.0], [1, 0, 0])], D_MODEL), open(clf, "w"))
    out = tmp_path / "pred"
    argv = ["-test", str(paths["te"]), "-model", "unused", "-classifier", str(clf), "-output", str(out), "-device", "cpu", "-batchSize", "2",
            "-tokenIdx", str(TOKEN)]
    xgb_predict.main(argv + ["-layer", "1"])
    assert sorted(os.listdir(out)) == ["te_embeddings_layer1.npz", "te_predictions_layer1.tsv"]
    np.testing.assert_array_equal(np.load(out / "te_embeddings_layer1.npz")["test"], _want(model, te, 1))
    xgb_predict.main(argv)
    assert sorted(os.listdir(out)) == ["te_embeddings.npz", "te_embeddings_layer1.npz", "te_predictions.tsv", "te_predictions_layer1.tsv"]
    np.testing.assert_array_equal(np.load(out / "te_embeddings.npz")["test"], _want(model, te, N_LAYER))
    xgb_predict.main(argv + ["-layer", "2", "-save_memory", "-chunk_size", "2"])
    assert {"te_chunk_0_embeddings_layer2.npz", "te_chunk_2_embeddings_layer2.npz", "te_chunk_4_embeddings_layer2.npz",
            "te_predictions_layer2.tsv"} <= set(os.listdir(out))
    # xgb_train
    stub = types.ModuleType("xgboost")
    stub.XGBClassifier = _StubXGBClassifier
    monkeypatch.setitem(sys.modules, "xgboost", stub)
    out = tmp_path / "train"
    argv = ["-train", str(paths["tr"]), "-valid", str(paths["va"]), "-test", str(paths["te"]), "-model", "unused", "-output", str(out),
            "-device", "cpu", "-batchSize", "4", "-seed", "7", "-tokenIdx", str(TOKEN)]
    xgb_train.main(argv + ["-layer", "0"])
    names = [n for n in os.listdir(out) if not n.endswith(".png")]          # the plots need matplotlib
    assert sorted(names) == sorted(["train_valid_embeddings_layer0.npz", "te_embeddings_layer0.npz", "seed_7_XGBoost_layer0.json",
                                    "seed_7_valid_predictions_layer0.npz", "seed_7_va_layer0_metrics.txt",
                                    "seed_7_te_predictions_layer0.npz", "seed_7_te_layer0_metrics.txt"])
    np.testing.assert_array_equal(np.load(out / "te_embeddings_layer0.npz")["test"], _want(model, te, 0))
    xgb_train.main(argv)
    names = [n for n in os.listdir(out) if not n.endswith(".png") and "_layer0" not in n]
    assert sorted(names) == sorted(["train_valid_embeddings.npz", "te_embeddings.npz", "seed_7_XGBoost.json", "seed_7_valid_predictions.npz",
                                    "seed_7_va_metrics.txt", "seed_7_te_predictions.npz", "seed_7_te_metrics.txt"])
    np.testing.assert_array_equal(np.load(out / "te_embeddings.npz")["test"], _want(model, te, N_LAYER))
