"""CPU: the small-launch policy (which of the four layer walks a pcad_forward call runs) against its restatement in
tests/launch_forms.py, read off pcad_workspace_bytes - no device work.

This is the tripwire for tests/test_gpu_launch_forms.py: those cases are sized to sit on either side of the bounds in
csrc/kernels.hpp::scan_segments / scan_pair_wanted and csrc/convx.hip::convx_ksplit.  A bound moved there without moving the
restatement (and the GPU cases with it) fails here."""
import os

import pytest

from plantcaduceus_amd import engine
from launch_forms import Probe, chunk_for, convx_ksplit, predict, scan_pair_wanted, scan_segments

DS = [64, 128, 192, 384, 768, 1024, 1536, 2048]
LS = [1, 63, 64, 100, 127, 128, 192, 255, 256, 300, 512, 2047, 2048, 2080, 8192]


def dt_rank(D):
    return -(-D // 16)          # "auto": 1536 -> 96 (Rp 96), 2048 -> 128 (Rp 128: no fused conv + x_proj)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH):
        engine.build_library()
    return engine.load_library()


def batches(D, L):
    """Batch sizes on both sides of every bound for this (D, L): waves per direction = 2B * 2D / 64 = B * D / 16."""
    out = {1, 2, 3}
    for waves in (512, 768, 3584):
        b = waves * 16 // D
        out |= {b, b + 1}
    b = 64 // (2 * -(-L // 128))                  # conv row tiles = 2B * ceil(L / 128)
    out |= {b, b + 1}
    return sorted(x for x in out if x >= 1)


def test_restatement_matches_library_on_the_grid(lib):
    n, forms = 0, set()
    for D in DS:
        for bf16 in (False, True):
            p = Probe(lib, D, dt_rank(D), bf16)
            try:
                for L in LS:
                    for B in batches(D, L):
                        want = p.predict(B, L)
                        got = p.scratch(B, L)
                        assert got == want["scratch"], (D, "bf16" if bf16 else "fp32", L, B, got, want)
                        forms.add((want["G"] > 1, want["pair"], want["ks"] > 1))
                        n += 1
            finally:
                p.close()
    assert n > 1500
    # the grid reaches every form, alone and in the combinations the policy allows
    assert {(True, False, False), (True, False, True), (False, True, False), (False, True, True), (False, False, True),
            (False, False, False)} <= forms, forms


def test_restatement_matches_library_off_the_shipped_geometry(lib):
    """pcad_create also takes `expand` 1, 3, 4 (E = D, 3D, 4D: another wave count per strand, another K-tile count of the fused conv +
    x_proj kernel, another chunk cap, other scratch sizes) and `dt_rank` up to 256 (Rp 128, 160, 256: no fused kernel, hence neither
    the pair walk nor the K-split; the segmented scan stays).  The library's form scratch must equal the restatement there too:
    tests/test_gpu_geometries.py names the walk of each of its cases through `engaged_forms` (sizing only; the kernels are
    checked there)."""
    n, forms = 0, set()
    for D in (64, 128, 256, 1024):
        for expand in (1, 2, 3, 4):
            for R in (dt_rank(D), 100, 129, 256):
                if expand == 2 and R == dt_rank(D):
                    continue                                  # the grid above
                for bf16 in (False, True):
                    p = Probe(lib, D, R, bf16, expand=expand)
                    try:
                        for L in (63, 128, 256, 300, 512, 2080):
                            bs = {1, 2, 3, 9}
                            for waves in (512, 768, 3584):    # waves per direction = 2B * E / 64
                                b = waves * 32 // (expand * D)
                                bs |= {b, b + 1}
                            for B in sorted(x for x in bs if x >= 1):
                                want = p.predict(B, L)
                                got = p.scratch(B, L)
                                assert got == want["scratch"], (D, expand, R, "bf16" if bf16 else "fp32", L, B, got, want)
                                if R > 96:
                                    assert not want["pair"] and want["ks"] == 1
                                forms.add((expand, R > 96, want["G"] > 1, want["pair"], want["ks"] > 1))
                                n += 1
                    finally:
                        p.close()
    assert n > 3000
    for expand in (1, 3, 4):
        # every form is reached off E = 2D as well: segmented, pair, K-split on the fused walk; segmented and plain on the other
        got = {f[2:] for f in forms if f[0] == expand and not f[1]}
        assert {(True, False, False), (False, True, False), (False, False, True), (False, False, False)} <= got, (expand, got)
        assert {f[2:] for f in forms if f[0] == expand and f[1]} == {(True, False, False), (False, False, False)}, expand


def test_smallest_shapes_that_reach_each_form_off_the_shipped_geometry():
    """The restatement itself at the smallest shapes that reach each form with dt_rank > 96 or expand != 2 (hand-counted from
    csrc/kernels.hpp, like test_bounds_are_where_the_header_says)."""
    # dt_rank 100 (Rp 128), d_model 128: 2 windows of 300 bp = 16 waves -> 10 segments of one 32-step block, no K-split
    assert predict(128, 100, False, 2, 300)["G"] == 10 and predict(128, 100, True, 2, 300)["ks"] == 1
    assert predict(64, 100, False, 1, 2080)["G"] == 4              # one long window: segments of >= 16 blocks
    for bf16 in (False, True):
        f = predict(64, 4, bf16, 3, 128, expand=4)                 # E = 256: 24 waves, L % 64 == 0, L < 256 -> the pair walk
        assert f["pair"] and f["G"] == 1
        f = predict(64, 4, bf16, 3, 64, expand=1)                  # E = 64: one wave per strand, L < 128 -> the plain walk
        assert (f["G"], f["pair"], f["ks"]) == (1, False, 1)
    assert convx_ksplit(6, 64, 64, True) == 1 and convx_ksplit(6, 64, 64, False) == 1       # E = 64: one / two K-tiles, nothing to split
    assert scan_segments(6, 64, 64)[0] == 1


def test_bounds_are_where_the_header_says():
    """The restatement itself, at the bounds include/pcad.h documents (a guard against editing both sides into agreement with
    each other but not with the documentation)."""
    E = 2048                                                        # l32: 32 waves per strand
    assert scan_segments(16, 512, E) == (4, 4)                     # 8 windows of 512 bp: 512 waves, 4 segments of 4 blocks
    assert scan_segments(18, 512, E)[0] == 1 and scan_pair_wanted(18, 512, E)         # 9 windows: pair
    assert scan_pair_wanted(112, 512, E) and not scan_pair_wanted(114, 512, E)       # up to 56 windows of 512 bp
    assert scan_segments(24, 2048, E) == (3, 22)                    # 768 waves at L >= 2048 still cut ...
    assert scan_segments(26, 2048, E)[0] == 1                       # ... 832 not
    assert scan_segments(2, 2080, 128) == (4, 17)                   # long strands: segments of >= 16 blocks, a short last one
    assert scan_segments(2, 255, 128)[0] == 1 and scan_segments(2, 256, 128)[0] == 8
    assert not scan_pair_wanted(2, 127, 128) and scan_pair_wanted(2, 128, 128) and not scan_pair_wanted(2, 160, 128)
    assert convx_ksplit(16, 512, E, True) == 4                      # 64 row tiles: 256 blocks
    assert convx_ksplit(18, 512, E, True) == 1                      # 72 row tiles: none
    assert convx_ksplit(2, 512, E, True) == 16                      # one window at l32: 8 tiles x 16 blocks of 2 K-tiles
    assert convx_ksplit(6, 256, 384, True) == 3 and convx_ksplit(6, 256, 384, False) == 6     # not a power of two
    assert chunk_for(1024, 512, 2048, True) == 512 and chunk_for(1024, 512, 2048, False) == 256


@pytest.mark.parametrize("bf16", [False, True])
def test_policy_follows_the_call_not_the_chunk(lib, bf16):
    """"chunk_seqs" < B: the scratch is sized for the chunk's strands, but the forms (G, pair, ks) are those of the call's
    strands - every chunk of a call runs the same form (include/pcad.h "chunk_seqs")."""
    cases = [(1024, 512, 8, 1), (1024, 512, 8, 3), (1024, 512, 9, 1), (1024, 512, 56, 5), (1024, 512, 57, 2),
             (64, 128, 896, 100), (128, 300, 2, 1), (64, 2080, 3, 1), (128, 127, 3, 1), (384, 512, 22, 7)]
    for D, L, B, cs in cases:
        p = Probe(lib, D, dt_rank(D), bf16, chunk_seqs=cs)
        try:
            want = p.predict(B, L)
            assert want["chunk"] <= cs < B                                # even chunks of at most cs windows
            assert p.scratch(B, L) == want["scratch"], (D, L, B, cs, want)
            whole = predict(D, dt_rank(D), bf16, B, L)                       # the same call, default chunking
            assert (want["G"], want["pair"], want["ks"]) == (whole["G"], whole["pair"], whole["ks"])
            alone = predict(D, dt_rank(D), bf16, cs, L)                      # what a call of one chunk's windows would run
            if (D, L, B) in ((1024, 512, 8), (1024, 512, 9), (1024, 512, 56), (1024, 512, 57)):
                assert (alone["G"], alone["pair"], alone["ks"]) != (want["G"], want["pair"], want["ks"]), (D, L, B, cs)
        finally:
            p.close()


@pytest.mark.parametrize("bf16", [False, True])
def test_options_that_switch_the_forms_off(lib, bf16):
    pts = [(B, L) for L in (128, 256, 300, 512, 2048, 2080) for B in (1, 2, 8, 9, 20)]
    # "scan_segments" 0: no form scratch at all, whatever the call
    p = Probe(lib, 1024, 64, bf16, scan_segments=0)
    try:
        for B, L in pts:
            assert p.scratch(B, L) == 0 and p.predict(B, L)["scratch"] == 0
    finally:
        p.close()
    # dt_rank > 96: Rp = 128, no fused conv + x_proj kernel, hence neither the pair walk nor the K-split; the segmented scan stays
    for R in (97, 128):
        p = Probe(lib, 1024, R, bf16)
        try:
            seg = 0
            for B, L in pts:
                want = p.predict(B, L)
                assert not want["pair"] and want["ks"] == 1
                assert p.scratch(B, L) == want["scratch"], (R, B, L)
                seg += want["G"] > 1
            assert seg > 0
        finally:
            p.close()
    # dt_rank 96 (Rp 96) keeps all three
    p = Probe(lib, 1024, 96, bf16)
    try:
        assert p.predict(9, 512)["pair"] and p.predict(1, 512)["ks"] > 1
        for B, L in pts:
            assert p.scratch(B, L) == p.predict(B, L)["scratch"]
    finally:
        p.close()


def test_f32_gemm_split_model_keeps_the_policy(lib):
    """The fp32 + "f32_gemm_split" model runs the same forms as the plain fp32 model (the split-bf16 products change the GEMMs, not
    the scan / conv launches) and its chunk cap is the fp32 model's own."""
    p = Probe(lib, 1024, 64, False, f32_gemm_split=1)
    q = Probe(lib, 1024, 64, False)
    try:
        for L in (128, 256, 512, 2048):
            for B in (1, 2, 8, 9, 20, 56, 57, 1024):
                want = p.predict(B, L)
                assert p.scratch(B, L) == want["scratch"] == q.scratch(B, L), (B, L)
        assert p.predict(1024, 512)["chunk"] == 256
    finally:
        p.close()
        q.close()
