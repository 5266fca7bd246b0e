"""CPU checks behind tests/test_gpu_scan_fwd_seg.py: the three phases of the segmented training forward, restated in
tests/scan_fwd_seg_ref.py, give the output of tests/scan_bwd_ref.py's plain recurrence; the C entries (include/pcad_bwd.h) size their
scratch and refuse bad arguments before any device work; the PCAD_TRAIN_SCAN_FWD_SEGMENTS helper, the parser flag and the defaults of the
operators and of the models."""
import inspect
import os
import re
import subprocess

import pytest
import torch

import scan_bwd_ref as SB
import scan_fwd_seg_ref as SF
import scan_ref as R
from plantcaduceus_amd import engine, ops, pretrain

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE
NAMES = {"pcad_selective_scan_fwd_seg_scratch_bytes", "pcad_selective_scan_fwd_seg"}
T = ops.SCAN_BWD_CHUNK
# (Bsz, E, L, G): the GPU file's hand-overs (a second segment of one step, part segments at the end, three and more effective segments)
# and its two shapes with three waves / three strands
CASES = [(2, 128, T + 1, 4), (2, 128, 3 * T + 4, 4), (2, 128, 3 * T + 4, 3), (2, 128, 8 * T + 1, 2), (2, 128, 8 * T + 1, 3),
         (2, 128, 8 * T + 1, 8), (2, 192, 3 * T + 4, 4), (3, 64, 8 * T + 1, 3)]


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def _inputs(Bsz, E, L, bare=False):
    def make():
        x = SB.inputs(100 * Bsz + L + E, Bsz, E, L)
        if bare:
            x["z"] = x["D"] = x["delta_bias"] = None
        return x
    return R.cached(("scan_fwd_seg_cpu", Bsz, E, L, bare), make)


def _ref(Bsz, E, L, bare, reverse):
    return R.cached(("scan_fwd_seg_cpu_ref", Bsz, E, L, bare, reverse), lambda: SB.forward(_inputs(Bsz, E, L, bare), reverse))


def _segments(L, G):
    return -(-L // ops.scan_bwd_seg_steps(L, G))


@pytest.mark.parametrize("reverse", [False, True])
@pytest.mark.parametrize("case", CASES)
def test_float64_restatement_of_the_three_phases_is_the_forward(case, reverse):
    """float64 against float64: only the association of the carried state (and exp2 for exp) differs, so 1e-12 of the output's maximum"""
    Bsz, E, L, G = case
    assert SF.SS.CHUNK == T and SF.SS.seg_steps(L, G) == ops.scan_bwd_seg_steps(L, G)
    for bare in (False, True):
        m = SB.metric(SF.forward(_inputs(Bsz, E, L, bare), G, reverse), _ref(Bsz, E, L, bare, reverse))
        assert m < 1e-12, (bare, m)


def test_restatement_notices_a_missing_hand_over():
    """what the 1e-12 above is worth: without P_g in the carry the output is off by far more than 1e-4 at every case of three or more
    segments (with two, H_1 = e_0 and P_g multiplies zero), and without H_g at every case"""
    seen = 0
    for Bsz, E, L, G in CASES:
        x, ref = _inputs(Bsz, E, L), _ref(Bsz, E, L, False, False)
        assert SB.metric(SF.forward(x, G, drop="H"), ref) > 1e-4, (L, G)
        m = SB.metric(SF.forward(x, G, drop="P"), ref)
        if _segments(L, G) >= 3:
            seen += 1
            assert m > 1e-4, (L, G, m)
        else:
            assert m < 1e-12, (L, G, m)
    assert seen >= 4


def test_fp32_restatement_has_room_under_the_fp32_bar():
    """the same three phases in fp32 against float64: at most a third of BAR_SCAN's fp32 3e-5 on these inputs, so that the device's own
    exp2 / log2 / rcp approximations (a few ulp each) have two thirds of the bar left and the GPU test is not met by luck"""
    worst = 0.0
    for Bsz, E, L, G in CASES:
        for reverse in (False, True):
            m = SB.metric(SF.forward(_inputs(Bsz, E, L), G, reverse, dtype=torch.float32), _ref(Bsz, E, L, False, reverse))
            worst = max(worst, m)
    print(f"fp32 restatement of the segmented forward against float64, worst case: {worst:.2e} [bar {R.BAR_SCAN[False]:.1e}]")
    assert worst <= R.BAR_SCAN[False] / 3, worst


def test_header_signatures_and_library_name_the_entries(lib):
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "pcad_bwd.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(pcad_[a-z0-9_]+)\s*\(", hdr))
    out = subprocess.run(["nm", "-D", "--defined-only", engine.BWD_LIB_PATH], capture_output=True, text=True, check=True).stdout
    exported = {ln.split()[-1] for ln in out.splitlines()}
    assert NAMES <= declared and NAMES <= set(engine.BWD_SIGNATURES) and NAMES <= exported
    assert all(hasattr(lib, n) for n in NAMES)


def test_scratch_bytes_are_aligned_and_monotone_in_segments(lib):
    f = lib.pcad_selective_scan_fwd_seg_scratch_bytes
    for S, L, E in ((2, 64, 128), (3, 8192, 192)):
        sizes = [f(S, L, E, G) for G in (1, 2, 4, 8)]
        assert all(b > 0 and b % 256 == 0 for b in sizes)
        assert sizes == sorted(sizes) and len(set(sizes)) == 4, sizes            # 1, 2, 4, 8 effective segments at these L
        assert sizes[3] >= S * 8 * (16 + 1) * E * 4                               # e / H and Dsum of every (strand, segment)
    prev = 0
    for G in range(1, 65):                                                       # monotone in the effective count, which the rule may repeat
        b = f(2, 8192, 128, G)
        assert b >= prev, G
        prev = b
    assert f(2, 9, 128, 64) == f(2, 9, 128, 2)                                   # two effective segments either way
    assert f(0, 17, 128, 4) == 0 and f(2, 0, 128, 4) == 0 and f(2, 17, 96, 4) == 0 and f(2, 17, 128, 0) == 0 and f(2, 17, 128, 65) == 0


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null value stands for a tensor.  Every call here is refused (or has nothing
    to do) before a launch; a complete call is never made."""
    p = 0x10000
    last = engine.load_library().pcad_last_error          # the message is libpcad.so's, on the calling thread

    def call(E=128, u=p, y=p, z=p, bc=p, dtype=0, scratch=p, nbytes=1 << 30, S=2, L=40, G=4):
        return lib.pcad_selective_scan_fwd_seg(u, p, z, E, bc, p, p, p, y, scratch, nbytes, S, L, E, 0, dtype, G, None)
    for name in ("u", "y"):
        assert call(**{name: None}) == INV and name.encode() in last(), name
    for G in (0, -1, 65):
        assert call(G=G) == INV and b"segments" in last(), G
    for E in (96, 0):
        assert call(E=E) == INV and b"E" in last()
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(bc=p + 4) == INV and b"bc" in last()
    assert call(S=1 << 24, E=8192) == INV and b"grid" in last()                  # 2^24 strands x 3 segments x 128 waves
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    assert call(nbytes=lib.pcad_selective_scan_fwd_seg_scratch_bytes(2, 40, 128, 1)) == WSP      # one segment's size is too short for three
    # nothing to do: OK before the scratch is looked at
    assert call(S=0, scratch=None, nbytes=0) == 0 and call(L=0, scratch=None, nbytes=0) == 0


def test_auto_policy_is_the_backwards_cut_back_where_few_segments_fill_the_device():
    slots, E = 2048, 1536
    fill = ops.SCAN_FWD_SEG_MIN_FILL
    assert fill == 8
    for L in (8192, 4096, 1024, 261, 100, 8):
        prev = None
        for S in (1, 2, 3, 4, 8, 16, 21, 22, 32, 43, 86, 172):
            G, Gb = ops.scan_fwd_auto_segments(S, L, E, slots), ops.scan_bwd_auto_segments(S, L, E, slots)
            few = S * (E // 64) * (fill // 2) >= slots               # fewer than `fill` segments fill the slots
            assert G == (1 if few else Gb), (S, L, G, Gb)
            if prev is not None:
                assert G <= prev, (S, L, G, prev)                     # fewer strands never get fewer segments
            prev = G
    # the timed shapes (profiles/scan_fwd_seg_timing.txt): 1, 4 and 8 windows keep the backward's count, 16 and 43 stay unsegmented
    assert [ops.scan_fwd_auto_segments(S, 8192, E, slots) for S in (2, 8, 16, 32, 86)] == [64, 16, 8, 1, 1]
    assert ops.scan_bwd_auto_segments(32, 8192, E, slots) == 4
    assert ops._resolve_segments("auto", 32, 8192, E, lambda S, L, E: ops.scan_fwd_auto_segments(S, L, E, slots)) == 1
    assert ops._resolve_segments(4, 32, 8192, E, ops.scan_fwd_auto_segments) == 4       # an explicit count is taken as given


def test_environment_helper_and_flag():
    f = pretrain.scan_segments_from_env
    name = pretrain.SCAN_FWD_SEGMENTS_ENV
    assert name == "PCAD_TRAIN_SCAN_FWD_SEGMENTS" and pretrain.SCAN_SEGMENTS_ENV == "PCAD_TRAIN_SCAN_SEGMENTS"
    assert f({}, name) == 1 and f({name: ""}, name) == 1 and f({name: "1"}, name) == 1
    assert f({name: "8"}, name) == 8 and f({name: "64"}, name) == 64 and f({name: " auto "}, name) == "auto" and f("AUTO", name) == "auto"
    for bad in ("0", "65", "-2", "four", "2.5"):
        with pytest.raises(SystemExit) as e:
            f({name: bad}, name)
        assert name in str(e.value), bad
    # each variable is its own setting: the backward's alone leaves the forward's off, and the other way round
    env = {pretrain.SCAN_SEGMENTS_ENV: "8"}
    assert f(env) == 8 and f(env, name) == 1
    assert f({name: "8"}) == 1 and f({name: "8"}, name=name) == 8
    assert inspect.signature(f).parameters["name"].default == pretrain.SCAN_SEGMENTS_ENV        # called as before: as before
    assert "--scan_fwd_segments" in pretrain.build_parser().format_help()
    assert pretrain.build_parser().get_default("scan_fwd_segments") is None       # absent: the environment decides


def test_defaults_are_off():
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM, TrainableCaduceusForSequenceClassification
    for fn, key in ((ops.mamba_inner_fn, "scan_fwd_segments"), (ops.selective_scan_fn, "fwd_segments"), (ops.selective_scan_fwd_seg, "segments"),
                    (ops._SelectiveScanFn.forward, "fwd_segments"),
                    (TrainableCaduceusForMaskedLM.__init__, "scan_fwd_segments"),
                    (TrainableCaduceusForMaskedLM.from_pretrained, "scan_fwd_segments"),
                    (TrainableCaduceusForSequenceClassification.__init__, "scan_fwd_segments")):
        assert inspect.signature(fn).parameters[key].default == 1, fn
    assert TrainableCaduceusForMaskedLM.scan_fwd_segments == 1 and TrainableCaduceusForSequenceClassification.scan_fwd_segments == 1
    names = list(inspect.signature(ops.mamba_inner_fn).parameters)
    assert names[-1] == "scan_fwd_segments" and names.index("scan_bwd_segments") == names.index("reverse") + 1
    assert list(inspect.signature(ops.selective_scan_fn).parameters)[-2:] == ["segments", "fwd_segments"]


def test_backward_setting_alone_leaves_the_forward_off(monkeypatch):
    """PCAD_TRAIN_SCAN_SEGMENTS alone: what both commands read for the forward is 1"""
    monkeypatch.setenv(pretrain.SCAN_SEGMENTS_ENV, "16")
    monkeypatch.delenv(pretrain.SCAN_FWD_SEGMENTS_ENV, raising=False)
    assert pretrain.scan_segments_from_env(os.environ) == 16
    assert pretrain.scan_segments_from_env(os.environ, pretrain.SCAN_FWD_SEGMENTS_ENV) == 1
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "lora_predict.py")).read()
    assert "scan_segments_from_env(os.environ, pretrain.SCAN_FWD_SEGMENTS_ENV)" in src
