"""CPU checks behind tests/test_gpu_pooled_logits.py and tests/test_gpu_feature_train.py: the float64 restatement of
tests/pooled_logits_ref.py is tests/seqcls_ref.py's head and its backward formulas are the derivatives (central finite differences);
pcad_pooled_logits / pcad_pooled_logits_bwd are declared, bound and exported under the same names and refuse bad arguments before any
device work; PCAD_TRAIN_FEATURES parses, and is refused with trained factors; the budget guard at its boundary; the index batches are
`LabelledBatches`' windows; and the feature pass over gloo gives every rank the one-process cache exactly."""
import os
import re
import socket
import subprocess

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import pooled_logits_ref as PL
import scan_bwd_ref as SB
import seqcls_ref as SR
from plantcaduceus_amd import engine, lora_predict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV = -1                               # include/pcad.h PCAD_ERR_INVALID
NEW = ("pcad_pooled_logits", "pcad_pooled_logits_bwd")


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


# ---- the restatement --------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bf", [False, True])
def test_restatement_is_seqcls_refs_head(bf):
    """tests/test_pool_bwd_ref.py's rule: below 1e-6 without roundings; with the bf16 rounding points the two round the same float64
    products at the same places, so the logits are equal"""
    c = PL.inputs(5, 3, 48, 5, bf=bf)
    dtype = torch.bfloat16 if bf else torch.float32
    got = PL.logits(c["pooled"], c["score_w"], bf)
    want = SR.score_ref(c["pooled"], c["score_w"], dtype)
    m = SB.metric(got, want)
    print(f"pooled logits restatement bf={bf}: {m:.3e}")
    if bf:
        assert torch.equal(got.float(), want)
    else:
        assert m < 1e-6


def test_backward_formulas_are_the_derivatives():
    """central differences of sum(dlogits * logits) of the unrounded forward in float64 over every coordinate of score_w and pooled,
    step 1e-6, held to 1e-6 of each gradient's maximum (as tests/test_pool_bwd_ref.py)"""
    c = PL.inputs(3, 2, 8, 3)
    dW, dP = PL.backward(c["pooled"], c["score_w"], c["dlogits"])
    assert torch.equal(dP[:, 0], dP[:, 1])

    def loss(d):
        return (PL.logits(d["pooled"], d["score_w"]) * d["dlogits"].double()).sum().item()
    eps = 1e-6
    for name, g in (("score_w", dW), ("pooled", dP)):
        base = c[name].double()
        fd = torch.zeros_like(base).reshape(-1)
        for i in range(base.numel()):
            vals = []
            for sign in (1.0, -1.0):
                t = base.clone().reshape(-1)
                t[i] += sign * eps
                vals.append(loss(dict(c, **{name: t.reshape(base.shape)})))
            fd[i] = (vals[0] - vals[1]) / (2 * eps)
        err = (fd.reshape(base.shape) - g).abs().max().item() / g.abs().max().item()
        print(f"finite differences {name}: {err:.3e}")
        assert err < 1e-6, name


# ---- the C entries ----------------------------------------------------------------------------------------------------------------------
def test_header_table_and_library_name_the_same_two_symbols():
    header = open(os.path.join(ROOT, "include", "pcad_bwd.h")).read()
    declared = set(re.findall(r"^(?:int|size_t|int64_t)\s+(pcad_\w+)\(", header, flags=re.M))
    assert set(NEW) <= declared and set(NEW) <= set(engine.BWD_SIGNATURES) and declared == set(engine.BWD_SIGNATURES)
    if not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.BWD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines() if " T " in ln and ln.split()[-1].startswith("pcad_")}
    assert set(NEW) <= exported and exported == declared
    # libpcad.so's arithmetic is restated, not exported
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    assert not any(name in out for name in NEW)


def test_entries_refuse_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor.  Every call below is
    refused before the launch (or has nothing to do): none may reach a device with these pointers."""
    p = 0x10000
    last = engine.load_library().pcad_last_error

    def fwd(pooled=p, W=p, lg=p, B=2, D=384, NL=5, dtype=0):
        return lib.pcad_pooled_logits(pooled, W, lg, B, D, NL, dtype, None)

    def bwd(pooled=p, W=p, dl=p, dW=p, dP=p, B=2, D=384, NL=5):
        return lib.pcad_pooled_logits_bwd(pooled, W, dl, dW, dP, B, D, NL, None)
    for name, word in (("pooled", b"pooled"), ("W", b"score_w"), ("lg", b"logits")):
        assert fwd(**{name: None}) == INV and b"pcad_pooled_logits: null " + word in last(), name
    for name, word in (("pooled", b"pooled"), ("W", b"score_w"), ("dl", b"dlogits")):
        assert bwd(**{name: None}) == INV and b"pcad_pooled_logits_bwd: null " + word in last(), name
    assert bwd(dW=None, dP=None) == INV and b"no output" in last() and b"dscore_w" in last() and b"dpooled" in last()
    for call in (fwd, bwd):
        assert call(NL=0) == INV and b"num_labels" in last()
        assert call(NL=257) == INV and b"num_labels" in last()
        assert call(D=12) == INV and b"D must be" in last() and b"D=12" in last()
        assert call(D=2056) == INV and b"2048" in last()
        assert call(D=0) == INV and call(B=-1) == INV and b"B must be" in last()
        for name in ("pooled", "W"):
            assert call(**{name: p + 8}) == INV and b"16-byte aligned" in last(), name
    assert fwd(dtype=7) == INV and b"dtype" in last()
    assert fwd(lg=p + 2) == INV and b"logits" in last()
    for name, word in (("dW", b"dscore_w"), ("dP", b"dpooled")):
        assert bwd(**{name: p + 8}) == INV and word + b" must be 16-byte aligned" in last(), name
    # no windows: OK, nothing is done; the per-window operands may then be NULL, the weight may not
    assert fwd(B=0) == 0 and fwd(B=0, pooled=None, lg=None) == 0 and fwd(B=0, W=None) == INV
    assert bwd(B=0) == 0 and bwd(B=0, pooled=None, dl=None, dP=None) == 0 and bwd(B=0, W=None) == INV


# ---- the knob, the guard, the batches ---------------------------------------------------------------------------------------------------
def test_train_features_knob():
    f = lora_predict.train_features_from_env
    assert lora_predict.FEATURES_ENV == "PCAD_TRAIN_FEATURES"
    for env in ({}, {"PCAD_TRAIN_FEATURES": ""}, {"PCAD_TRAIN_FEATURES": "off"}, {"PCAD_TRAIN_FEATURES": " OFF "}):
        assert f(env, True) is False and f(env, False) is False
    assert f({"PCAD_TRAIN_FEATURES": "cache"}, False) is True
    with pytest.raises(SystemExit, match="PCAD_TRAIN_FEATURES") as e:
        f({"PCAD_TRAIN_FEATURES": "cache"}, True)
    assert "--train_lora" in str(e.value)
    for junk in ("1", "on", "cached", "lazy"):
        with pytest.raises(SystemExit, match="PCAD_TRAIN_FEATURES"):
            f({"PCAD_TRAIN_FEATURES": junk}, False)


def test_cache_with_trained_factors_exits_before_anything_is_read(monkeypatch, tmp_path):
    monkeypatch.setenv("PCAD_TRAIN_FEATURES", "cache")
    with pytest.raises(SystemExit, match="PCAD_TRAIN_FEATURES") as e:
        lora_predict.main(["train", "--train_dir", str(tmp_path / "none.parquet"), "--valid_dir", str(tmp_path / "none.parquet"),
                           "--model_name", str(tmp_path / "none"), "--train_lora", "1"])
    assert "--train_lora" in str(e.value)


def test_feature_block_rule():
    f = lora_predict.feature_block_windows
    assert f(8192, {}) == 32 and f(512, {}) == 512 and f(69, {}) == 2 ** 18 // 69 and f(2 ** 18, {}) == 1 and f(2 ** 19, {}) == 1
    assert f(8192, {"PCAD_TRAIN_FEATURE_BATCH": "3"}) == 3 and f(8192, {"PCAD_TRAIN_FEATURE_BATCH": " "}) == 32
    for junk in ("0", "-2", "many", "1.5"):
        with pytest.raises(SystemExit, match="PCAD_TRAIN_FEATURE_BATCH"):
            f(8192, {"PCAD_TRAIN_FEATURE_BATCH": junk})


def test_budget_guard_at_its_boundary():
    """scheduled samples below N / 2 are refused: 2 * scheduled < N"""
    g = lora_predict.check_feature_budget
    g(50, 100), g(50, 99), g(8, 16), g(1, 2), g(1, 1), g(10 ** 9, 3)
    for scheduled, n in ((49, 100), (49, 99), (7, 16), (0, 1)):
        with pytest.raises(SystemExit, match="PCAD_TRAIN_FEATURES") as e:
            g(scheduled, n)
        assert str(scheduled) in str(e.value) and str(n) in str(e.value)


@pytest.mark.parametrize("seed", [0, 42, 7])
def test_index_batches_are_labelled_batches_windows(seed):
    n, L, batch, acc = 19, 5, 4, 2
    g = np.random.default_rng(seed)
    ids, labels = g.integers(3, 7, size=(n, L)).astype(np.int32), g.integers(0, 2, size=n).astype(np.int64)
    a = lora_predict.LabelledBatches(ids, labels, batch, acc, seed)
    b = lora_predict.LabelledIndexBatches(ids, labels, batch, acc, seed)
    assert b.steps_per_epoch == a.steps_per_epoch
    for step in (0, 1, 2, 3, 5, 11):
        wa, wb = a.windows(step), b.windows(step)
        assert len(wa) == len(wb) and all(np.array_equal(x, y) for x, y in zip(wa, wb))
        for (xa, ya, _), (idx, yb, none), w in zip(a.step_batches(step), b.step_batches(step), wa):
            assert none is None and idx.dtype == torch.int64 and np.array_equal(idx.numpy(), w)
            assert torch.equal(torch.from_numpy(ids[idx.numpy()]), xa) and torch.equal(ya, yb)


# ---- the feature pass over a process group ----------------------------------------------------------------------------------------------
WIDTH = 6
CASES = [(n, fb) for n in (1, 5, 8) for fb in (1, 3)]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _rows(n):
    return torch.randn(n, WIDTH, generator=torch.Generator().manual_seed(70 + n))


def _stand_in(data, calls=None):
    """a forward whose every row depends on its whole block"""
    def run(lo, hi):
        if calls is not None:
            calls.append((lo, hi))
        x = data[lo:hi]
        return x * x.sum() + x.mean(0)
    return run


def _pass_worker(rank, ws, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.set_num_threads(1)
        out = {}
        for n, fb in CASES:
            calls = []
            out[(n, fb)] = (lora_predict.feature_pass(n, fb, _stand_in(_rows(n), calls), WIDTH, "cpu"), calls)
        torch.save(out, os.path.join(outdir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_feature_pass_gives_every_rank_the_one_process_cache(tmp_path, ws):
    assert not dist.is_initialized()
    mp.spawn(_pass_worker, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt") for r in range(ws)]
    for n, fb in CASES:
        one = lora_predict.feature_pass(n, fb, _stand_in(_rows(n)), WIDTH, "cpu")
        assert one.shape == (n, WIDTH) and one.dtype == torch.float32
        calls = []
        for r in range(ws):
            rows, mine = got[r][(n, fb)]
            assert rows.shape == one.shape and torch.equal(rows, one), (n, fb, r)           # exactly, on every rank
            calls += mine
        assert calls == [(b0, min(b0 + fb, n)) for b0 in range(0, n, fb)]                   # the fixed blocks, each run once
