"""Nucleotide-probability head (csrc/probs.hip), the parts that need no GPU: the C ABI's declarations and exports,
and the host side - boundary_probs / sv_effect's sparse path - driven by a stand-in model that implements `nucleotide_probs` on the
CPU as softmax(logits[..., cols]) at the asked rows."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from plantcaduceus_amd import engine, sharding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L_WIN, FLANK = 40, 5


def test_header_declares_and_library_exports_the_probs_entries():
    hdr = open(os.path.join(ROOT, "include", "pcad.h")).read()
    for name in ("pcad_forward_probs", "pcad_probs_head"):
        assert re.search(r"^int\s+%s\(" % name, hdr, re.M), name
        assert name in engine.SIGNATURES
    lib = engine.load_library()
    for name in ("pcad_forward_probs", "pcad_probs_head"):
        assert hasattr(lib, name), name
    syms = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert " T pcad_forward_probs" in syms and " T pcad_probs_head" in syms


def test_probs_abi_validates_without_gpu():
    """PCAD_ERR_INVALID before any launch: cols outside the vocabulary, P outside its range, both position forms at once."""
    import ctypes as C
    from test_mlm_eval import _handle
    lib = engine.load_library()
    h = _handle(lib, 128, 0)
    i4 = lambda *v: (C.c_int32 * len(v))(*v)
    INVALID = -1                       # include/pcad.h PCAD_ERR_INVALID
    one = C.c_void_p(256)              # never dereferenced: every call below is refused while its arguments are checked
    try:
        call = lambda pos, P, ppw, cols: lib.pcad_forward_probs(h, one, 2, 32, pos, P, ppw, cols, one, None, one, 1 << 20, None)
        assert call(None, 0, None, i4(3, 4, 5, 8)) == INVALID          # PCAD_ERR_INVALID
        assert call(None, 0, None, i4(-1, 4, 5, 6)) == INVALID
        assert call(i4(1, 2), 2, one, i4(3, 4, 5, 6)) == INVALID       # both forms
        assert call(None, 17, one, i4(3, 4, 5, 6)) == INVALID          # P > PCAD_MAX_POSITIONS
        assert call(None, 0, one, i4(3, 4, 5, 6)) == INVALID           # per-window list without a length
        assert call(None, 3, None, i4(3, 4, 5, 6)) == INVALID          # a length without a list
        head = lambda pos, P, ppw, cols: lib.pcad_probs_head(one, one, one, one, one, cols, one, None, 2, 32, 64, C.c_float(1e-5), pos,
                                                              P, ppw, 0, None, None, 0, 0, 0, None)
        assert head(None, 0, None, i4(3, 4, 5, 8)) == INVALID
        assert head(i4(1, 2), 2, one, i4(3, 4, 5, 6)) == INVALID
        assert head(None, 17, one, i4(3, 4, 5, 6)) == INVALID
        assert head(i4(1, 32), 2, None, i4(3, 4, 5, 6)) == INVALID     # a shared position outside the window
    finally:
        lib.pcad_destroy(h)


# ---- host side: a stand-in with nucleotide_probs ------------------------------------------------------------------------------
class _Out:
    def __init__(self, logits):
        self.logits = logits


class DenseStandIn:
    """`.logits` only (no supports_nucleotide_probs): every window is run on its own through the CPU oracle, so that a window's
    numbers do not depend on the batch or the rank it is evaluated in."""

    def __init__(self):
        from oracle import caduceus_oracle as O
        from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
        cfg = make_config("x", d_model=32, n_layer=1)
        self.inner = O.OracleForMaskedLM(O.params_from_state_dict(synthetic_state_dict(cfg, seed=5), cfg))
        self.config = cfg
        self.calls = []

    def _logits(self, input_ids):
        return torch.cat([self.inner(input_ids=input_ids[i:i + 1]).logits.float() for i in range(input_ids.shape[0])], dim=0)

    def __call__(self, input_ids=None, **kw):
        self.calls.append(("logits", tuple(input_ids.shape)))
        return _Out(self._logits(input_ids))


class ProbsStandIn(DenseStandIn):
    """nucleotide_probs on the CPU: softmax(logits[..., cols]) at the asked rows; records the shape of every result it hands out."""
    supports_nucleotide_probs = True

    def nucleotide_probs(self, input_ids, cols, positions=None, positions_per_window=None, return_logits=False):
        assert positions is None or positions_per_window is None
        lg = self._logits(input_ids)
        if positions_per_window is not None:
            assert positions_per_window.shape[0] == input_ids.shape[0] and positions_per_window.shape[1] <= 16
            assert int(positions_per_window.min()) >= 0 and int(positions_per_window.max()) < lg.shape[1]
            lg = torch.gather(lg, 1, positions_per_window.long()[:, :, None].expand(-1, -1, lg.shape[2]))
        elif positions is not None:
            lg = lg[:, list(positions), :]
        p = torch.softmax(lg[..., list(cols)].float(), dim=-1)
        self.calls.append(("probs", tuple(p.shape)))
        return (p, lg) if return_logits else p


def _sv_table(n, seed=0):
    import pandas as pd
    rng = np.random.default_rng(seed)
    draw = lambda: "".join(rng.choice(list("ACGTacgtN"), size=L_WIN, p=[.2, .2, .2, .2, .04, .04, .04, .04, .04]))
    left = rng.integers(FLANK + 1, L_WIN // 2, size=n)
    right = rng.integers(L_WIN // 2, L_WIN - FLANK, size=n)
    left[0], right[0] = FLANK + 1, L_WIN - FLANK                 # rows 0 and L - 1 of the window are read
    return pd.DataFrame({"RefSeq": [draw() for _ in range(n)], "MutSeq": [draw() for _ in range(n)], "left": left, "right": right,
                         "label": rng.integers(0, 2, size=n)})


def _run_sv(model, df, tmp, tag, batch_size=4, **kw):
    import pandas as pd
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    out = os.path.join(str(tmp), f"sv_{tag}.tsv")
    res = pe.sv_effect(df, model, CaduceusTokenizer(), "cpu", batch_size=batch_size, flanking=FLANK, output=out, **kw)
    # the scores are float32 (the probabilities' dtype); their shortest decimal form in the table reads back to the same float32
    scores = pd.read_csv(out, sep="\t")["score"].to_numpy().astype(np.float32) if os.path.exists(out) else None
    return res, scores


def test_sv_effect_sparse_equals_dense_single_process(tmp_path):
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    df = _sv_table(11)
    sparse_m, dense_m = ProbsStandIn(), DenseStandIn()
    res_s, sc_s = _run_sv(sparse_m, df, tmp_path, "sparse")
    res_d, sc_d = _run_sv(dense_m, df, tmp_path, "dense")
    # the sparse path asked for [b, 2F, 4] rows only: no [n, L, 4] array and no logits call
    assert sparse_m.calls and all(kind == "probs" and shape[1:] == (2 * FLANK, 4) for kind, shape in sparse_m.calls), sparse_m.calls
    assert all(kind == "logits" for kind, _ in dense_m.calls)     # without the attribute: the old path
    assert abs(res_s["AUPRC"] - res_d["AUPRC"]) <= 1e-12
    np.testing.assert_allclose(sc_s, sc_d, rtol=0, atol=1e-12)
    assert abs(pe.auroc(df["label"], sc_s) - pe.auroc(df["label"], sc_d)) <= 1e-12
    # boundary_probs hands back exactly the rows of the dense array
    tok = CaduceusTokenizer()
    ref_pos, mut_pos = pe._sv_positions(df["left"], df["right"], L_WIN, FLANK)
    assert ref_pos.min() == 0 and ref_pos.max() == L_WIN - 1
    dense = pe.unmasked_probs(df["RefSeq"], tok, DenseStandIn(), "cpu", batch_size=3)
    rows = pe.boundary_probs(df["RefSeq"], ref_pos, tok, ProbsStandIn(), "cpu", batch_size=3)
    assert rows.shape == (11, 2 * FLANK, 4) and rows.dtype == np.float32
    np.testing.assert_array_equal(rows, dense[np.arange(11)[:, None], ref_pos])
    # masked_probs / unmasked_probs route through nucleotide_probs when the model has it, with the same numbers
    m = ProbsStandIn()
    np.testing.assert_array_equal(pe.unmasked_probs(df["RefSeq"], tok, m, "cpu", batch_size=3), dense)
    np.testing.assert_array_equal(pe.masked_probs(m, tok, list(df["RefSeq"]), [7, 3], "cpu", batch_size=4),
                                  pe.masked_probs(DenseStandIn(), tok, list(df["RefSeq"]), [7, 3], "cpu", batch_size=4))
    assert all(kind == "probs" for kind, _ in m.calls) and ("probs", (3, L_WIN, 4)) in m.calls and ("probs", (4, 2, 4)) in m.calls
    # sv_llr_boundary keeps its signature and results: the shared arithmetic on rows selected from the dense arrays
    mut_dense = pe.unmasked_probs(df["MutSeq"], tok, DenseStandIn(), "cpu", batch_size=3)
    np.testing.assert_array_equal(pe.sv_llr_boundary(df["left"], df["right"], df["MutSeq"], dense, mut_dense, FLANK).astype(np.float32), sc_d)


def test_sv_effect_keeps_the_dense_path_when_asked_to_save_or_too_wide(tmp_path):
    df = _sv_table(5)
    m = ProbsStandIn()
    res, _ = _run_sv(m, df, tmp_path, "save", save_ref_logits=str(tmp_path / "ref.npz"))
    assert np.load(tmp_path / "ref.npz")["logits"].shape == (5, L_WIN, 4)
    assert all(shape[1:] == (L_WIN, 4) for _, shape in m.calls)
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    m2 = ProbsStandIn()
    df2 = df.assign(left=12, right=28)
    pe.sv_effect(df2, m2, CaduceusTokenizer(), "cpu", batch_size=4, flanking=9)           # 18 positions > PCAD_MAX_POSITIONS
    assert all(shape[1:] == (L_WIN, 4) for _, shape in m2.calls)


def test_out_of_range_boundary_raises_before_any_collective(monkeypatch):
    """A boundary position that sv_llr_boundary's indexing would refuse raises IndexError before a model call or a gather."""
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    df = _sv_table(6)
    df.loc[3, "right"] = L_WIN - FLANK + 1                        # reads row L
    m = ProbsStandIn()

    def no_collective(*a, **k):
        raise AssertionError("a collective / sharded loop was entered before the positions were checked")

    monkeypatch.setattr(pe, "_sharded_rows", no_collective)
    monkeypatch.setattr(sharding, "all_gather_blocks", no_collective)
    with pytest.raises(IndexError, match="out of bounds"):
        pe.sv_effect(df, m, CaduceusTokenizer(), "cpu", batch_size=4, flanking=FLANK)
    assert m.calls == []
    with pytest.raises(IndexError, match="out of bounds"):
        pe.boundary_probs(df["RefSeq"], np.full((6, 2), L_WIN), CaduceusTokenizer(), m, "cpu")
    with pytest.raises(IndexError, match="out of bounds"):
        pe.boundary_probs(df["RefSeq"], np.full((6, 2), -1), CaduceusTokenizer(), m, "cpu")
    # the dense path refuses the same table (after its forwards)
    monkeypatch.undo()
    with pytest.raises(IndexError):
        pe.sv_effect(df, DenseStandIn(), CaduceusTokenizer(), "cpu", batch_size=4, flanking=FLANK)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _sv_worker(rank, ws, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        from plantcaduceus_amd import plantcad2_eval as pe
        from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
        torch.set_num_threads(1)
        pe.GATHER_CHUNK = 2                             # several gathers per call, ragged last chunk
        df = _sv_table(11)
        m = ProbsStandIn()
        res = pe.sv_effect(df, m, CaduceusTokenizer(), "cpu", batch_size=4, flanking=FLANK,
                           output=os.path.join(outdir, f"w{ws}.tsv"))
        ref_pos, _ = pe._sv_positions(df["left"], df["right"], L_WIN, FLANK)
        rows = pe.boundary_probs(df["RefSeq"], ref_pos, CaduceusTokenizer(), m, "cpu", batch_size=4)
        assert all(kind == "probs" and shape[1:] == (2 * FLANK, 4) for kind, shape in m.calls), m.calls
        a, b, _ = sharding.shard_bounds(11, rank, ws)
        assert sum(shape[0] for _, shape in m.calls) == 3 * (b - a)          # its own block only: ref, mut, ref again
        np.savez(os.path.join(outdir, f"w{ws}_r{rank}.npz"), auprc=res["AUPRC"], rows=rows)
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 4])
def test_sv_effect_sparse_gloo_worlds_bit_equal_world_1(tmp_path, ws):
    import pandas as pd
    from plantcaduceus_amd import plantcad2_eval as pe
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    mp.spawn(_sv_worker, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    df = _sv_table(11)
    res1, sc1 = _run_sv(ProbsStandIn(), df, tmp_path, "w1")
    res_d, sc_d = _run_sv(DenseStandIn(), df, tmp_path, "w1dense")
    ref_pos, _ = pe._sv_positions(df["left"], df["right"], L_WIN, FLANK)
    rows1 = pe.boundary_probs(df["RefSeq"], ref_pos, CaduceusTokenizer(), ProbsStandIn(), "cpu", batch_size=4)
    sc = pd.read_csv(tmp_path / f"w{ws}.tsv", sep="\t")["score"].to_numpy().astype(np.float32)            # written by rank 0
    np.testing.assert_array_equal(sc, sc1)
    np.testing.assert_allclose(sc, sc_d, rtol=0, atol=1e-12)
    for r in range(ws):
        got = np.load(tmp_path / f"w{ws}_r{r}.npz")
        assert float(got["auprc"]) == res1["AUPRC"] and abs(float(got["auprc"]) - res_d["AUPRC"]) <= 1e-12
        np.testing.assert_array_equal(got["rows"], rows1)
