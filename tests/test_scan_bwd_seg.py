"""CPU checks behind tests/test_gpu_scan_bwd_seg.py: the three phases of the segmented backward, restated in float64 in
tests/scan_bwd_seg_ref.py, give the gradients of tests/scan_bwd_ref.py's autograd reference; the C entries of the segmented form
(include/pcad_bwd.h) cut segments, size their scratch and refuse bad arguments before any device work; the "auto" policy, the
PCAD_TRAIN_SCAN_SEGMENTS helper and the defaults of the models and of mamba_inner_fn."""
import inspect
import os
import re

import pytest
import torch

import scan_bwd_ref as SB
import scan_bwd_seg_ref as SS
from plantcaduceus_amd import engine, ops, pretrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


CASES = [(2, 64, 28, 4), (3, 64, 65, 3), (2, 64, 9, 4)]      # (Bsz, E, L, G): 4, 3 and 2 effective segments


def _inputs(Bsz, E, L, bare):
    x = SB.inputs(100 * Bsz + L, Bsz, E, L)
    if bare:
        x["z"] = x["D"] = x["delta_bias"] = None
    return x


@pytest.mark.parametrize("bare", [False, True])
@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_of_the_three_phases_is_the_gradient(case, reverse, bare):
    """float64 against float64: only the association of the carried values differs, so 1e-12 of each gradient's maximum"""
    Bsz, E, L, G = case
    x = _inputs(Bsz, E, L, bare)
    ref, got = SB.grads(x, reverse), SS.grads(x, G, reverse)
    for name in SB.NAMES:
        if ref[name] is None:
            assert got[name] is None, name
            continue
        m = SB.metric(got[name], ref[name])
        assert m < 1e-12, (name, m)


def test_restatement_notices_a_missing_hand_over():
    """what the 1e-12 above is worth: without H, without K, or without P_g in phase 2 the affected gradients are off by far more.
    (3, 64, 65, 3) has three segments - with two, K_0 = kappa_1 and a missing P_g would not show."""
    assert SS.CHUNK == ops.SCAN_BWD_CHUNK
    Bsz, E, L, G = CASES[1]
    assert -(-L // SS.seg_steps(L, G)) == 3
    x = _inputs(Bsz, E, L, False)
    ref = SB.grads(x, False)
    for drop, names in (("H", ("C", "A", "z")), ("K", ("u", "delta", "B")), ("P", ("u", "delta", "A"))):
        got = SS.grads(x, G, False, drop=drop)
        for name in names:
            assert SB.metric(got[name], ref[name]) > 1e-4, (drop, name)


STEPS = [((28, 4), 8), ((28, 3), 16), ((65, 2), 40), ((65, 3), 24), ((9, 4), 8), ((7, 4), 8), ((8192, 16), 512), ((8192, 64), 128),
         ((512, 64), 8), ((28, 0), 0), ((28, 65), 0)]


@pytest.mark.parametrize("LG,steps", STEPS)
def test_segment_steps(lib, LG, steps):
    L, G = LG
    assert lib.pcad_selective_scan_bwd_seg_steps(L, G) == steps
    assert ops.scan_bwd_seg_steps(L, G) == steps               # the host restatement the policy uses
    if steps:
        assert SS.seg_steps(L, G) == steps and steps % ops.SCAN_BWD_CHUNK == 0 and -(-L // steps) <= G


def test_constants_match_the_kernel():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int SCAN_BWD_MAX_SEGMENTS = (\d+);", src).group(1)) == ops.SCAN_BWD_MAX_SEGMENTS == 64
    assert ops.SCAN_BWD_SEG_MIN_STEPS > 0 and ops.SCAN_BWD_SEG_MIN_STEPS % ops.SCAN_BWD_CHUNK == 0


def test_scratch_bytes_cover_the_unsegmented_call_and_grow_with_segments(lib):
    f = lib.pcad_selective_scan_bwd_seg_scratch_bytes
    plain = engine.load_train_library().pcad_selective_scan_bwd_scratch_bytes
    for S, L, E in ((2, 64, 128), (3, 8192, 192)):
        sizes = [f(S, L, E, G) for G in (1, 2, 4, 8)]
        assert all(b % 256 == 0 for b in sizes) and sizes[0] >= plain(S, L, E) > 0
        assert sizes == sorted(sizes) and len(set(sizes)) == 4, sizes            # 1, 2, 4, 8 effective segments at these L
        # e, kappa and Dsum of every (strand, segment) besides the partials
        assert sizes[3] - sizes[0] >= S * 8 * (2 * 16 + 1) * E * 4
    assert f(2, 9, 128, 64) == f(2, 9, 128, 2)                                   # two effective segments either way
    assert f(0, 17, 128, 4) == 0 and f(2, 0, 128, 4) == 0 and f(2, 17, 96, 4) == 0 and f(2, 17, 128, 0) == 0 and f(2, 17, 128, 65) == 0


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null value stands for a tensor.  Every call here is refused (or has nothing
    to do) before a launch; a complete call is never made."""
    p = 0x10000
    last = engine.load_library().pcad_last_error          # the message is libpcad.so's, on the calling thread

    def call(E=128, u=p, dout=p, z=p, dz=p, bc=p, dbc=p, dA=p, dtype=0, scratch=p, nbytes=1 << 30, S=2, L=40, G=4):
        return lib.pcad_selective_scan_bwd_seg(u, p, z, E, bc, p, p, p, dout, p, p, dz, dbc, dA, p, p, scratch, nbytes, S, L, E, 0, dtype, G, None)
    for name in ("u", "dout", "dA"):
        assert call(**{name: None}) == INV and name.encode() in last(), name
    assert call(dz=None) == INV and b"dz" in last()
    assert call(z=None) == INV and b"dz" in last()
    for G in (0, -1, 65):
        assert call(G=G) == INV and b"segments" in last(), G
    assert call(E=96) == INV and b"E" in last()
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(bc=p + 4) == INV and b"bc" in last()
    assert call(dbc=p + 8) == INV and b"dbc" in last()
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    # the unsegmented call's size is too short for four segments
    assert call(nbytes=engine.load_train_library().pcad_selective_scan_bwd_scratch_bytes(2, 40, 128)) == WSP
    # nothing to do: OK before the scratch is looked at
    assert call(S=0, scratch=None, nbytes=0) == 0 and call(L=0, scratch=None, nbytes=0) == 0


def test_auto_policy_properties():
    slots, E = 2048, 1536
    M = ops.SCAN_BWD_SEG_MIN_STEPS
    for L in (8192, 4096, 1024, 512, 100, 8):
        prev = None
        for S in (1, 2, 3, 4, 8, 16, 43, 86, 172):
            G = ops.scan_bwd_auto_segments(S, L, E, slots)
            assert 1 <= G <= 64 and G & (G - 1) == 0, (S, L, G)
            if S * E // 64 >= slots:
                assert G == 1
            if G > 1:
                assert ops.scan_bwd_seg_steps(L, G) >= M, (S, L, G)
                assert S * (E // 64) * (G // 2) < slots                           # the smallest G that fills the slots, or one cut short by M
            if prev is not None:
                assert G <= prev, (S, L, G, prev)                                 # fewer strands never get fewer segments
            prev = G
    assert ops.scan_bwd_auto_segments(2, 8192, E, slots) == min(64, 8192 // M)    # 48 waves: as many segments as the length allows
    assert ops.scan_bwd_auto_segments(2, M, E, slots) == 1
    assert ops.scan_bwd_auto_segments(1, 1 << 20, 64, 1 << 20) == 64              # never more than 64


def test_environment_helper():
    f = pretrain.scan_segments_from_env
    name = pretrain.SCAN_SEGMENTS_ENV
    assert name == "PCAD_TRAIN_SCAN_SEGMENTS"
    assert f({}) == 1 and f({name: ""}) == 1 and f({name: "1"}) == 1
    assert f({name: "8"}) == 8 and f({name: "64"}) == 64 and f({name: " auto "}) == "auto" and f({name: "AUTO"}) == "auto"
    for bad in ("0", "65", "-2", "four", "2.5"):
        with pytest.raises(SystemExit) as e:
            f({name: bad})
        assert name in str(e.value), bad
    assert "--scan_bwd_segments" in pretrain.build_parser().format_help()
    assert pretrain.build_parser().get_default("scan_bwd_segments") is None       # absent: the environment decides


def test_defaults_are_off():
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM, TrainableCaduceusForSequenceClassification
    for fn, key in ((ops.mamba_inner_fn, "scan_bwd_segments"), (ops.selective_scan_fn, "segments"), (ops.selective_scan_bwd, "segments"),
                    (TrainableCaduceusForMaskedLM.__init__, "scan_bwd_segments"),
                    (TrainableCaduceusForSequenceClassification.__init__, "scan_bwd_segments")):
        assert inspect.signature(fn).parameters[key].default == 1, fn
    names = list(inspect.signature(ops.mamba_inner_fn).parameters)
    assert names.index("scan_bwd_segments") == names.index("reverse") + 1
    for bad in (0, 65, "many"):
        with pytest.raises(ValueError):
            ops._resolve_segments(bad, 2, 64, 64)
