"""pcad_forward_layers stops its layer walk at the highest requested level without touching the ABI: the C symbols
libpcad.so exports are the ones include/pcad.h declared before, and pcad_workspace_bytes is what tests/test_mlm_eval.py records."""
import ctypes as C
import subprocess

from plantcaduceus_amd import engine

# the C ABI as it stood before the walk learned its depth
EXPORTS = """pcad_add_rmsnorm pcad_bind_weights pcad_build_hash pcad_causal_conv1d_silu pcad_causal_conv1d_silu_dir pcad_conv_xproj_bidir
pcad_conv_xproj_scratch_bytes pcad_create pcad_destroy pcad_final_head pcad_forward pcad_forward_all_hidden pcad_forward_at
pcad_forward_layers pcad_forward_loss pcad_forward_pooled pcad_forward_probs pcad_gather_rows pcad_gemm_nt pcad_gemm_nt_residual
pcad_gemm_nt_split pcad_gemm_nt_split_scratch_bytes pcad_last_error pcad_layer_rows pcad_loss_head pcad_loss_head_scratch_bytes
pcad_pooled_head pcad_pooled_head_scratch_bytes pcad_probs_head pcad_profile_enable pcad_profile_read pcad_selective_scan
pcad_selective_scan_dtproj pcad_set_option pcad_set_status_buffer pcad_version pcad_weight_arena_bytes pcad_workspace_bytes""".split()
# ... plus the operator entries added since for the engine's scan and conv + x_proj launch forms (tests/test_gpu_engine_forms.py):
# additions only, nothing above changed
EXPORTS += """pcad_conv_xproj_bidir_engine pcad_conv_xproj_split_scratch_bytes pcad_scan_pair_scratch_bytes pcad_scan_segment_scratch_bytes
pcad_selective_scan_engine pcad_selective_scan_pair""".split()
# ... and for the engine's GEMM launch forms (tests/test_gpu_gemm_forms.py): additions only again
EXPORTS += "pcad_gemm_nt_engine pcad_gemm_nt_residual_engine pcad_gemm_nt_two pcad_gemm_nt_xproj".split()


def test_exported_c_symbols_are_unchanged():
    engine.load_library()
    out = subprocess.run(["nm", "-D", "--defined-only", engine.LIB_PATH], capture_output=True, text=True, check=True).stdout
    got = sorted(line.split()[-1] for line in out.splitlines() if line.split()[-1].startswith("pcad_"))
    assert got == sorted(EXPORTS), set(got) ^ set(EXPORTS)
    assert set(EXPORTS) == set(engine.SIGNATURES)


def test_workspace_bytes_unchanged():
    from test_mlm_eval import WORKSPACE_BYTES, _handle
    lib = engine.load_library()
    assert len({(B, L) for (_, _, _, B, L) in WORKSPACE_BYTES}) >= 3
    for (D, dt, split, B, L), want in WORKSPACE_BYTES.items():
        h = _handle(lib, D, dt, split)
        got = lib.pcad_workspace_bytes(h, B, L)
        lib.pcad_destroy(h)
        assert got == want, (D, dt, split, B, L, got)


def test_truncated_request_passes_the_argument_checks():
    """a request whose highest level lies below n_layer is refused for the unbound handle only, like any well-formed one"""
    from test_mlm_eval import _handle
    lib = engine.load_library()
    h = _handle(lib, 128, 0)                # n_layer 2
    one = C.c_void_p(256)                   # never dereferenced
    i4 = lambda *v: (C.c_int32 * len(v))(*v)
    try:
        for lay in (i4(0), i4(1), i4(0, 1)):
            assert lib.pcad_forward_layers(h, one, 2, 32, i4(1, 2), 2, None, lay, len(lay), 0, one, one, 1 << 20, None) == -2      # PCAD_ERR_UNBOUND
    finally:
        lib.pcad_destroy(h)
