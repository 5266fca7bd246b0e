"""CPU checks of the LoRA dropout behind tests/test_gpu_lora_dropout*.py: the restated generator against Random123's
known answers; the mask's statistics and its dependence on seed and stream; the restated backward against float64 autograd; every
refusal of the five C entries, decided without a device; the slab rule and the scratch size as the header states them; header, table and
exports name the same symbols; the model's stream formula and its choice between the merged and the unmerged call; the environment
variable of `lora_predict train`."""
import math
import os
import re
import subprocess

import numpy as np
import pytest
import torch

import lora_dropout_ref as LD
from plantcaduceus_amd import engine, ops

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE
NAMES = {"pcad_lora_dropout_mask", "pcad_lora_down", "pcad_lora_down_bwd_scratch_bytes", "pcad_lora_down_bwd_slabs", "pcad_lora_down_bwd"}
# K of in_proj, x_proj, out_proj at PlantCAD2 Small and at l32, r = 8
REAL_K = (768, 1536, 1536, 1024, 2048, 2048)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def words(v):
    return " ".join(f"{int(w):08x}" for w in v)


def test_philox_known_answers():
    """Random123's kat_vectors for philox4x32-10"""
    f = 0xFFFFFFFF
    assert words(LD.philox4x32_10((0, 0, 0, 0), (0, 0))) == "6627e8d5 e169c58d bc57ac4c 9b00dbd8"
    assert words(LD.philox4x32_10((f, f, f, f), (f, f))) == "408f276d 41c83b0e a20bc7c6 6d5451fd"
    assert words(LD.philox4x32_10((0x243f6a88, 0x85a308d3, 0x13198a2e, 0x03707344), (0xa4093822, 0x299f31d0))) == \
        "d16cfe09 94fdcceb 5001e420 24126ea1"


def test_threshold_and_scale():
    assert LD.threshold(0.0) == 0 and LD.keep_scale(0.0) == 1.0
    assert LD.threshold(0.5) == 32768 and LD.keep_scale(0.5) == 2.0
    assert LD.threshold(0.1) == 6554 and LD.keep_scale(0.1) == np.float32(65536.0) / np.float32(58982.0)
    assert ops.lora_dropout_threshold(0.1) == 6554 and ops.lora_dropout_threshold(0.99999) == 65535
    for bad in (-0.1, 1.0, 0.999995, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            ops.lora_dropout_threshold(bad)
    with pytest.raises(ValueError):
        LD.threshold(1.0)


@pytest.mark.parametrize("M,K", [(65, 72), (257, 136), (33, 8)])
def test_drop_count_is_binomial(M, K):
    """within 4 sigma of N q (q = T / 65536, the probability actually drawn); observed 0.34, 1.96 and 0.49 sigma"""
    keep = LD.keep_mask(M, K, 0.1, 1234, 5)
    N, q = M * K, LD.threshold(0.1) / 65536.0
    dropped = N - int(keep.sum())
    sigma = math.sqrt(N * q * (1 - q))
    print(f"({M}, {K}): dropped {dropped} of {N}, expected {N * q:.1f}, {abs(dropped - N * q) / sigma:.2f} sigma")
    assert abs(dropped - N * q) <= 4 * sigma


def test_mask_depends_on_seed_and_stream_not_on_shape():
    base = LD.keep_mask(65, 72, 0.1, 1234, 5)
    assert not np.array_equal(base, LD.keep_mask(65, 72, 0.1, 1234, 6))
    assert not np.array_equal(base, LD.keep_mask(65, 72, 0.1, 1235, 5))
    assert not np.array_equal(base, LD.keep_mask(65, 72, 0.1, 1234 + (1 << 32), 5))          # the seed's high word is part of the key
    assert not np.array_equal(base, LD.keep_mask(65, 72, 0.1, 1234, 5 + (1 << 32)))
    assert np.array_equal(base, LD.keep_mask(65, 72, 0.1, 1234, 5))
    assert np.array_equal(base[:33, :8], LD.keep_mask(33, 8, 0.1, 1234, 5))                   # no dependence on M or K
    assert LD.keep_mask(65, 72, 0.0, 1234, 5).all()
    # a larger p drops a superset: the same 16 bits against a larger threshold
    assert not (LD.keep_mask(65, 72, 0.5, 1234, 5) & ~base).any()


@pytest.mark.parametrize("p", [0.0, 0.1, 0.5])
def test_restated_backward_against_float64_autograd(p):
    """linear_backward's dx, dA, dB against autograd through dense masked float64 ops"""
    g = torch.Generator().manual_seed(3)
    M, K, N, r, scale = 37, 24, 20, 8, 4.0
    x = torch.randn(M, K, generator=g, dtype=torch.float64, requires_grad=True)
    W = torch.randn(N, K, generator=g, dtype=torch.float64)
    A = torch.randn(r, K, generator=g, dtype=torch.float64, requires_grad=True)
    B = torch.randn(N, r, generator=g, dtype=torch.float64, requires_grad=True)
    dy = torch.randn(M, N, generator=g, dtype=torch.float64)
    keep, c = torch.from_numpy(LD.keep_mask(M, K, p, 7, 11)), LD.keep_scale(p)
    dropped = torch.nn.functional.linear(x * keep * float(c), A)
    y = torch.nn.functional.linear(x, W) + scale * torch.nn.functional.linear(dropped, B)
    y2, _ = LD.linear_forward(x.detach(), W, A.detach(), B.detach(), scale, keep, c)
    assert (y.detach() - y2).abs().max().item() < 1e-12
    (y * dy).sum().backward()
    dx, dA, dB = LD.linear_backward(x.detach(), W, A.detach(), B.detach(), scale, keep, c, dy)
    for got, ref in ((dx, x.grad), (dA, A.grad), (dB, B.grad)):
        assert (got - ref).abs().max().item() < 1e-12
    # a dropped element's dx is dx0's, exactly
    assert torch.equal(dx[~keep], (dy @ W)[~keep])


def test_header_signatures_and_library_name_the_entries(lib):
    text = open(os.path.join(ROOT, "include", "pcad_bwd.h")).read()
    hdr = re.sub(r"/\*.*?\*/", "", text, flags=re.S)
    declared = set(re.findall(r"\b(pcad_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", engine.BWD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert NAMES <= declared and NAMES <= set(engine.BWD_SIGNATURES) and NAMES <= exported
    assert all(hasattr(lib, n) for n in NAMES)
    assert {n for n in declared if "lora" in n} == NAMES == {n for n in engine.BWD_SIGNATURES if "lora" in n} == \
        {n for n in exported if n.startswith("pcad_lora")}
    assert "IN PLACE" in text and "csrc/lora.hip" in text                        # the header states the in-place dx update


def test_constants_match_the_kernels():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    got = {k: int(re.search(rf"LORA_{k} = (\d+)", src).group(1)) for k in ("CHUNK", "TARGET_BLOCKS", "MAX_SLABS", "SLAB_ROWS", "MAX_K")}
    assert got == {"CHUNK": 512, "TARGET_BLOCKS": 1024, "MAX_SLABS": 256, "SLAB_ROWS": 64, "MAX_K": 8192}   # the numbers the header states
    assert (ops.LORA_RANKS, ops.LORA_MIN_K, ops.LORA_MAX_K) == ((4, 8, 16), 8, 8192)


def test_entries_refuse_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor"""
    P = 0x10000
    last = engine.load_library().pcad_last_error

    def mask(keep=P, M=10, K=64, ldk=None, p=0.1):
        return lib.pcad_lora_dropout_mask(keep, M, K, K if ldk is None else ldk, p, 1, 2, None)

    def down(x=P, ldx=None, A=P, t=P, M=10, K=64, r=8, p=0.1, dtype=1):
        return lib.pcad_lora_down(x, K if ldx is None else ldx, A, t, M, K, r, p, 1, 2, dtype, None)

    def bwd(x=P, ldx=None, A=P, u=P, dx=P, lddx=None, dA=P, scratch=P - P % 256 + 256, nbytes=1 << 40, M=10, K=64, r=8, p=0.1, dtype=1):
        return lib.pcad_lora_down_bwd(x, K if ldx is None else ldx, A, u, dx, K if lddx is None else lddx, dA, scratch, nbytes, M, K, r, p, 1, 2,
                                      dtype, None)

    for call in (mask, down, bwd):
        for bad in (0, 4, 12, 100, 8200, -8):
            assert call(K=bad, **({"ldk": 8208} if call is mask else {"ldx": 8208})) == INV and b"K " in last(), (call.__name__, bad)
        for bad in (-1, 1 << 32):
            assert call(M=bad) == INV and b"M " in last(), (call.__name__, bad)
        for bad in (-0.01, 1.0, 0.999995, float("nan"), float("inf")):
            assert call(p=bad) == INV and b"p " in last(), (call.__name__, bad)
    assert mask(ldk=56) == INV and b"ldk" in last()
    assert mask(keep=None) == INV and b"keep_u8" in last()
    assert mask(keep=None, M=0) == 0                                           # nothing to write
    for call in (down, bwd):
        for bad in (0, 1, 2, 3, 5, 12, 32):
            assert call(r=bad) == INV and b"r " in last(), (call.__name__, bad)
        assert call(dtype=2) == INV and b"dtype" in last()
        assert call(ldx=68) == INV and b"ldx" in last()                        # not a multiple of 8
        assert call(ldx=56) == INV and b"ldx" in last()                        # < K
        for name in ("x", "A"):
            assert call(**{name: None}) == INV and name.encode() in last(), (call.__name__, name)
            assert call(**{name: P + 8}) == INV and name.encode() in last() and b"aligned" in last(), (call.__name__, name)
    assert down(t=None) == INV and b"null t" in last()
    assert down(t=P + 4) == INV and b"t must be" in last()
    assert down(M=0, x=None, t=None) == 0                                      # no rows: nothing is read or written
    assert bwd(u=None) == INV and b"null u" in last()
    assert bwd(u=P + 8) == INV and b"u must be" in last()
    assert bwd(dx=None, dA=None) == INV and b"dx and dA" in last()
    assert bwd(dx=P + 8) == INV and b"dx must be" in last()
    assert bwd(dA=P + 8) == INV and b"dA must be" in last()
    assert bwd(lddx=68) == INV and b"lddx" in last()
    assert bwd(lddx=56) == INV and b"lddx" in last()
    assert lib.pcad_lora_down_bwd_scratch_bytes(10, 64, 8) > 0
    assert bwd(scratch=P + 16) == WSP and bwd(scratch=None) == WSP and bwd(nbytes=1024) == WSP and b"scratch" in last()
    rows = engine.C.c_int64(7)
    assert lib.pcad_lora_down_bwd_slabs(10, 12, 8, engine.C.byref(rows)) == -1 and b"K " in last() and rows.value == 0
    assert lib.pcad_lora_down_bwd_slabs(10, 64, 3, engine.C.byref(rows)) == -1 and b"r " in last()
    assert lib.pcad_lora_down_bwd_slabs(-1, 64, 8, engine.C.byref(rows)) == -1 and b"M " in last()
    assert lib.pcad_lora_down_bwd_scratch_bytes(10, 12, 8) == 0 and lib.pcad_lora_down_bwd_scratch_bytes(10, 64, 3) == 0


def formula(M, K, r):
    """include/pcad_bwd.h: -> (slabs, rows_per_slab, scratch bytes)"""
    if M == 0:
        return 0, 0, 0
    chunks = -(-K // 512)
    want = min(256, max(1, 1024 // chunks))
    rows = -(-(-(-M // want)) // 64) * 64
    slabs = -(-M // rows)
    return slabs, rows, -(-(slabs * r * K * 4) // 256) * 256


def test_slabs_and_scratch_are_the_documented_formula(lib):
    seen = set()
    for K, r in [(k, 8) for k in REAL_K] + [(8, 4), (520, 16), (8192, 16)]:
        for M in (0, 1, 63, 64, 65, 8191, 8192, 8193, 16384, 16385, 65536, 43 * 8192 * 2, 2 ** 32 - 1):
            slabs, rows = ops.lora_down_bwd_slabs(M, K, r)
            nb = lib.pcad_lora_down_bwd_scratch_bytes(M, K, r)
            assert (slabs, rows, nb) == formula(M, K, r), (M, K, r)
            assert nb % 256 == 0 and (M == 0 or (rows % 64 == 0 and (slabs - 1) * rows < M <= slabs * rows and slabs <= 256))
            seen.add(slabs)
    assert ops.lora_down_bwd_slabs(65, 8, 8) == (2, 64) and ops.lora_down_bwd_slabs(65536, 1536, 8) == (256, 256)
    assert ops.lora_down_bwd_slabs(16385, 768, 8) == (129, 128)                 # around a boundary: 16384 rows are 256 slabs of 64
    assert {0, 1, 2, 128, 256} <= seen
    with pytest.raises(RuntimeError, match="K "):
        ops.lora_down_bwd_slabs(10, 12, 8)


def test_python_limits_are_value_errors():
    for K, r, p, word in ((64, 3, 0.1, "r must"), (12, 8, 0.1, "K must"), (8200, 8, 0.1, "K must"), (64, 8, 1.0, "p must")):
        with pytest.raises(ValueError, match=word):
            ops.lora_dropout_limits(K, r, p)
    ops.lora_dropout_limits(1536, 8, 0.1)
    with pytest.raises(RuntimeError, match="ROCm"):                              # there is no CPU path and no torch fallback
        ops.lora_dropout_linear_fn(torch.zeros(3, 16), torch.zeros(5, 16), torch.zeros(8, 16), torch.zeros(5, 8), 4.0, 0.1, 0, 0)


def toy_model(**kw):
    from plantcaduceus_amd.checkpoint import make_config
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    cfg = make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))
    return TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", device="cpu", **kw)


def test_model_stream_formula_and_defaults():
    m = toy_model(lora_dropout=0.1)
    assert (m.lora_dropout, m.dropout_seed, m.dropout_step) == (0.1, 0, 0)
    assert toy_model().lora_dropout == 0.0
    for step, layer, rev, mod in ((0, 0, False, "in_proj"), (0, 0, True, "x_proj"), (3, 1, True, "out_proj"), (70000, 1, False, "x_proj")):
        assert m.dropout_stream(step, layer, rev, mod) == LD.stream_id(step, layer, int(rev), LD.MODULES.index(mod))
    assert m.dropout_stream(3, 1, True, "out_proj") == 3 * 65536 + 3 * 3 + 2
    assert m.LORA_MODULES == LD.MODULES
    # construction refuses what the kernels would refuse
    with pytest.raises(ValueError, match="r must"):
        toy_model(lora_dropout=0.1, r=2)
    with pytest.raises(ValueError, match="p must"):
        toy_model(lora_dropout=1.0)
    toy_model(r=2)                                                               # without dropout any r stays accepted


def test_save_adapter_writes_the_rate(tmp_path):
    from plantcaduceus_amd import adapters
    for p in (0.0, 0.1):
        d = str(tmp_path / f"a{p}")
        toy_model(lora_dropout=p).save_adapter(d, "some/base")
        assert adapters.read_adapter_config(d)["lora_dropout"] == p


def test_linear_takes_the_unmerged_path_only_when_training_with_grad(monkeypatch):
    """the op is stubbed: which call `_linear` makes, and with which mask arguments"""
    m = toy_model(lora_dropout=0.1)
    m.dropout_seed = 99
    holder = m.caduceus.backbone.layers[1].mixer.submodule.mamba_rev.x_proj
    with torch.no_grad():                                                        # the trunk's holders are allocated, not initialised
        holder.weight.normal_()
        holder.lora_B.weight.normal_()
    calls = []

    def stub(x, W, A, B, scale, p, seed, stream):
        calls.append((scale, p, seed, stream))
        return ops.lora_linear_fn(x, W, A, B, scale)
    monkeypatch.setattr(ops, "lora_dropout_linear_fn", stub)
    x = torch.randn(2, 5, holder.weight.shape[1])
    merged = ops.lora_linear_fn(x, holder.weight, holder.lora_A.weight, holder.lora_B.weight, 4.0)
    stream = m.dropout_stream(7, 1, True, "x_proj")
    m.train()
    assert torch.equal(m._linear(x, holder, stream), merged) and calls == [(4.0, 0.1, 99, stream)]
    with torch.no_grad():
        assert torch.equal(m._linear(x, holder, stream), merged)
    m.eval()
    assert torch.equal(m._linear(x, holder, stream), merged)
    m.train()
    assert torch.equal(m._linear(x, holder), merged)                             # no stream: the forward decided against dropout
    assert len(calls) == 1
    m0 = toy_model()
    m0.train()
    assert m0._linear(x, m0.caduceus.backbone.layers[1].mixer.submodule.mamba_rev.x_proj, stream).shape == merged.shape
    assert len(calls) == 1                                                       # p = 0: the merged call, as before


def test_environment_variable():
    from plantcaduceus_amd import lora_predict as lp
    assert lp.DROPOUT_ENV == "PCAD_LORA_DROPOUT"
    assert lp.lora_dropout_from_env({}) == 0.0 and lp.lora_dropout_from_env({lp.DROPOUT_ENV: " "}) == 0.0
    assert lp.lora_dropout_from_env({lp.DROPOUT_ENV: "0.1"}) == 0.1 and lp.lora_dropout_from_env({lp.DROPOUT_ENV: "0"}) == 0.0
    assert lp.lora_dropout_from_env({lp.DROPOUT_ENV: "0"}, train_lora=False) == 0.0
    for bad in ("x", "-0.1", "1", "1.5", "nan", "0.999995"):
        with pytest.raises(SystemExit, match=lp.DROPOUT_ENV):
            lp.lora_dropout_from_env({lp.DROPOUT_ENV: bad})
    with pytest.raises(SystemExit) as e:
        lp.lora_dropout_from_env({lp.DROPOUT_ENV: "0.1"}, train_lora=False)
    assert lp.DROPOUT_ENV in str(e.value) and "--train_lora 0" in str(e.value)
    # the flag keeps refusing, and now names the variable
    with pytest.raises(SystemExit) as e:
        lp.main(["train", "--train_dir", "t", "--valid_dir", "v", "--model_name", "m", "--lora_dropout", "0.1"])
    assert "lora_dropout" in str(e.value) and lp.DROPOUT_ENV in str(e.value)


def test_trainer_hook_sets_the_one_process_index():
    """FinetuneTrainer.before_micro_step: dropout_step = step n + j; pretrain.Trainer's is a no-op"""
    from types import SimpleNamespace
    from plantcaduceus_amd import lora_predict as lp, pretrain
    model = SimpleNamespace(dropout_step=0)
    tr = SimpleNamespace(model=model, step=5)
    lp.FinetuneTrainer.before_micro_step(tr, 3, 8)
    assert model.dropout_step == 43
    assert pretrain.Trainer.before_micro_step(tr, 3, 8) is None and model.dropout_step == 43
