"""Untied directions without a GPU: merge_lora's arithmetic, the `lora_deltas="apply"` policy of adapters.load_adapter, the
option's effect on the engine's sizes (none while it is off), and the validity of the inputs tests/test_gpu_untied.py uses."""
import ctypes as C

import pytest
import torch

from plantcaduceus_amd import adapters, engine, lora_predict
from plantcaduceus_amd.checkpoint import layer_keys, load_state_dict, make_config, save_checkpoint, synthetic_state_dict
from untied_ref import rel, toy_case


@pytest.fixture(scope="module")
def base(tmp_path_factory):
    cfg = make_config("tiny", d_model=128, n_layer=2)
    path = str(tmp_path_factory.mktemp("base"))
    save_checkpoint(path, cfg, synthetic_state_dict(cfg, seed=3))
    return cfg, path


def _lora_of(path, cfg):
    acfg = adapters.read_adapter_config(path)
    aud = adapters.audit_adapter(adapters.read_adapter_weights(path), acfg, n_layer=cfg.n_layer, d_model=cfg.d_model)
    return aud["lora"], acfg


# ---- merge_lora -----------------------------------------------------------------------------------------------------
def test_merge_lora_arithmetic(base, tmp_path):
    cfg, bp = base
    ad = str(tmp_path / "ad")
    adapters.make_synthetic_adapter(ad, cfg, 2, base_path=bp, lora_b_scale=0.1)
    lora, acfg = _lora_of(ad, cfg)
    # layer 1's reverse direction carries no in_proj factors, layer 0's forward direction no out_proj factors
    del lora[(1, "rev", "in_proj")], lora[(0, "fwd", "out_proj")]
    base_sd = {k: v for k, v in load_state_dict(bp).items() if k.startswith("caduceus.")}
    r, alpha = acfg["r"], acfg["lora_alpha"]
    assert (r, alpha) == (8, 32)
    merged = adapters.merge_lora(base_sd, lora, r, alpha)
    assert set(merged) == set(base_sd)
    touched = set()
    for i in range(cfg.n_layer):
        for d in ("fwd", "rev"):
            k = layer_keys(i, d)
            for mod in ("x_proj", "in_proj", "out_proj"):
                W = base_sd[k[mod]].float()
                if (i, d, mod) in lora:
                    want = W + (alpha / r) * (lora[(i, d, mod)]["B"].float() @ lora[(i, d, mod)]["A"].float())
                    assert not torch.equal(want, W)
                else:
                    want = W                                                       # a direction without factors keeps W
                assert merged[k[mod]].dtype == torch.float32 and torch.equal(merged[k[mod]], want), (i, d, mod)
                touched.add(k[mod])
        f, rv = layer_keys(i, "fwd"), layer_keys(i, "rev")
        for mod in ("in_proj", "out_proj", "x_proj"):                             # per direction: distinct values, distinct storage
            assert not torch.equal(merged[f[mod]], merged[rv[mod]])
            assert merged[f[mod]].data_ptr() != merged[rv[mod]].data_ptr()
    for k in set(base_sd) - touched:                                               # everything else is handed through
        assert merged[k] is base_sd[k]
    assert all(torch.equal(base_sd[k], v) for k, v in load_state_dict(bp).items() if k in base_sd)     # the input is not modified


def test_merge_lora_casts_once_after_the_merge(base, tmp_path):
    cfg, bp = base
    ad = str(tmp_path / "ad")
    adapters.make_synthetic_adapter(ad, cfg, 2, base_path=bp, lora_b_scale=0.1)
    lora, acfg = _lora_of(ad, cfg)
    base_sd = {k: v for k, v in load_state_dict(bp).items() if k.startswith("caduceus.")}
    m32 = adapters.merge_lora(base_sd, lora, acfg["r"], acfg["lora_alpha"])
    m16 = adapters.merge_lora(base_sd, lora, acfg["r"], acfg["lora_alpha"], dtype=torch.bfloat16)
    differs = 0
    for i in range(cfg.n_layer):
        for d in ("fwd", "rev"):
            for mod in ("x_proj", "in_proj", "out_proj"):
                k = layer_keys(i, d)[mod]
                assert m16[k].dtype == torch.bfloat16 and torch.equal(m16[k], m32[k].to(torch.bfloat16))
                twice = (base_sd[k].to(torch.bfloat16).float() + (m32[k] - base_sd[k].float())).to(torch.bfloat16)
                differs += int(not torch.equal(m16[k], twice))
    assert differs > 0          # rounding the base first is a different (twice-rounded) tensor: the test can tell the two apart


def test_merge_lora_without_the_tied_duplicates(base, tmp_path):
    """A snapshot's state dict may lack mamba_rev.in_proj / out_proj (tied duplicates): they are taken from mamba_fwd's."""
    cfg, bp = base
    ad = str(tmp_path / "ad")
    adapters.make_synthetic_adapter(ad, cfg, 2, base_path=bp, lora_b_scale=0.1)
    lora, acfg = _lora_of(ad, cfg)
    full = {k: v for k, v in load_state_dict(bp).items() if k.startswith("caduceus.")}
    bare = {k: v for k, v in full.items() if ".mamba_rev.in_proj." not in k and ".mamba_rev.out_proj." not in k}
    a = adapters.merge_lora(full, lora, acfg["r"], acfg["lora_alpha"])
    b = adapters.merge_lora(bare, lora, acfg["r"], acfg["lora_alpha"])
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)


# ---- load_adapter ---------------------------------------------------------------------------------------------------
def test_load_adapter_apply(base, tmp_path, caplog):
    cfg, bp = base
    ad = str(tmp_path / "nz")
    adapters.make_synthetic_adapter(ad, cfg, 2, base_path=bp, lora_b_scale=0.1)
    with caplog.at_level("INFO", logger="plantcaduceus_amd.adapters"):
        m = adapters.load_adapter(ad, task_type="classification", lora_deltas="apply")
    info = m.adapter_info
    assert info["lora_deltas"] == "apply" and info["merged_pairs"] == 2 * 3 * cfg.n_layer and info["untied_directions"] is True
    assert len(info["nonzero_lora_B"]) == info["merged_pairs"] and info["max_abs_delta"] > 0
    assert "merged" in caplog.text and "untied_directions" in caplog.text
    assert m.config.engine_options["untied_directions"] == 1
    lora, acfg = _lora_of(ad, cfg)
    want = adapters.merge_lora({k: v for k, v in load_state_dict(bp).items() if k.startswith("caduceus.")}, lora, acfg["r"], acfg["lora_alpha"])
    got = m.state_dict()
    for i in range(cfg.n_layer):
        for d in ("fwd", "rev"):
            for mod in ("x_proj", "in_proj", "out_proj"):
                k = layer_keys(i, d)[mod]
                assert torch.equal(got[k], want[k]), k
        f, r = layer_keys(i, "fwd"), layer_keys(i, "rev")
        assert got[f["in_proj"]].data_ptr() != got[r["in_proj"]].data_ptr()
    # bf16: the merged weight is rounded once
    mb = adapters.load_adapter(ad, task_type="classification", lora_deltas="apply", dtype=torch.bfloat16)
    k = layer_keys(1, "rev")["out_proj"]
    assert torch.equal(mb.state_dict()[k], want[k].to(torch.bfloat16))
    # the other policies are what they were
    assert "lora_deltas" not in adapters.load_adapter(ad, task_type="classification", lora_deltas="ignore").adapter_info
    with pytest.raises(ValueError, match="lora_deltas='ignore'"):
        adapters.load_adapter(ad, task_type="classification")
    with pytest.raises(ValueError):
        adapters.load_adapter(ad, task_type="classification", lora_deltas="merge")


def test_load_adapter_apply_x_proj_only_stays_tied(base, tmp_path):
    cfg, bp = base
    ad = str(tmp_path / "xp")
    adapters.make_synthetic_adapter(ad, cfg, 2, base_path=bp, lora_b_scale=0.1, targets=("x_proj",))
    m = adapters.load_adapter(ad, task_type="classification", lora_deltas="apply")
    assert m.adapter_info["lora_deltas"] == "apply" and m.adapter_info["merged_pairs"] == 2 * cfg.n_layer
    assert m.adapter_info["untied_directions"] is False
    assert not (getattr(m.config, "engine_options", None) or {}).get("untied_directions")
    got, base_sd = m.state_dict(), load_state_dict(bp)
    f, r = layer_keys(0, "fwd"), layer_keys(0, "rev")
    assert got[f["in_proj"]].data_ptr() == got[r["in_proj"]].data_ptr()           # still one tied parameter
    assert not torch.equal(got[f["x_proj"]], base_sd[f["x_proj"]]) and not torch.equal(got[r["x_proj"]], base_sd[r["x_proj"]])
    # null deltas: nothing to merge, nothing untied
    adapters.make_synthetic_adapter(str(tmp_path / "zero"), cfg, 2, base_path=bp)
    z = adapters.load_adapter(str(tmp_path / "zero"), task_type="classification", lora_deltas="apply")
    assert z.adapter_info["merged_pairs"] == 0 and z.adapter_info["untied_directions"] is False


def test_cli_accepts_apply():
    p = lora_predict.build_parser()
    for cmd in ("predict", "evaluate"):
        assert p.parse_args([cmd, "--checkpoint_dir", "a", "--data_dir", "b", "--lora-deltas", "apply"]).lora_deltas == "apply"
        assert p.parse_args([cmd, "--checkpoint_dir", "a", "--data_dir", "b", "--lora_deltas", "apply"]).lora_deltas == "apply"
        assert p.parse_args([cmd, "--checkpoint_dir", "a", "--data_dir", "b"]).lora_deltas == "auto"
        with pytest.raises(SystemExit):
            p.parse_args([cmd, "--checkpoint_dir", "a", "--data_dir", "b", "--lora-deltas", "merge"])


# ---- configuration ----------------------------------------------------------------------------------------------------
def test_untied_config_is_accepted_and_audited(tmp_path):
    from plantcaduceus_amd.checkpoint import audit_snapshot
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    from untied_ref import untied_state_dict
    cfg = make_config("tiny", d_model=64, n_layer=2, bidirectional_weight_tie=False)
    cfg.check_supported()
    sd = untied_state_dict(cfg, seed=4)
    path = str(tmp_path / "untied")
    save_checkpoint(path, cfg, sd)
    assert audit_snapshot(path)["problems"] == []                                  # distinct mamba_rev tensors are the model
    m = CaduceusForMaskedLM.from_pretrained(path)
    k = layer_keys(1, "rev")
    assert torch.equal(m.state_dict()[k["in_proj"]], sd[k["in_proj"]]) and torch.equal(m.state_dict()[k["out_proj"]], sd[k["out_proj"]])
    # a tied configuration's report is what it was: distinct values are a problem
    tied = make_config("tiny", d_model=64, n_layer=2)
    p2 = str(tmp_path / "tied")
    save_checkpoint(p2, tied, sd)
    from safetensors.torch import load_file, save_file
    raw = load_file(p2 + "/model.safetensors")
    raw[k["in_proj"]] = sd[k["in_proj"]].contiguous()
    save_file(raw, p2 + "/model.safetensors", metadata={"format": "pt"})
    assert any("tied tensors stored with different values" in p for p in audit_snapshot(p2, strict=False)["problems"])


# ---- C ABI ----------------------------------------------------------------------------------------------------------------
def _handle(lib, D, dtype, **options):
    c = engine.PcadConfig(d_model=D, n_layer=2, d_state=16, d_conv=4, expand=2, dt_rank=(D + 15) // 16, vocab=8, eps=1e-5,
                          dtype=dtype, residual_in_fp32=1, complement=(C.c_int32 * 8)(0, 1, 2, 6, 5, 4, 3, 7))
    h = C.c_void_p()
    assert lib.pcad_create(C.byref(c), C.byref(h)) == 0
    for k, v in options.items():
        assert lib.pcad_set_option(h, k.encode(), v) == 0
    return h


# (d_model, dtype, f32_gemm_split, B, L) -> (pcad_workspace_bytes, pcad_weight_arena_bytes) of the library before the option existed
# (the workspace column is tests/test_seqcls.py's WORKSPACE_BYTES)
SIZES_OFF = {
    (768, 1, False, 40, 600): (1058112000, 26367232), (768, 0, True, 4, 8192): (3078750208, 65406208),
    (1024, 1, False, 32, 8192): (15353249792, 45641984), (128, 0, False, 3, 45): (3124224, 1595136),
}


def test_sizes_unchanged_with_the_option_off():
    lib = engine.load_library()
    for (D, dt, split, B, L), (ws, arena) in SIZES_OFF.items():
        for opts in (dict(), dict(untied_directions=0)):
            h = _handle(lib, D, dt, f32_gemm_split=int(split), **opts)
            got = (lib.pcad_workspace_bytes(h, B, L), lib.pcad_weight_arena_bytes(h))
            lib.pcad_destroy(h)
            assert got == (ws, arena), (D, dt, split, B, L, opts, got)


def test_sizes_with_the_option_on():
    """On: the arena grows by mamba_rev's in_proj + out_proj per layer (and their [hi | lo] copies under "f32_gemm_split"), the
    workspace by the second x / z pair (minus, for the bf16 model, what the norm-folded form no longer needs: never less than the
    "norm_fold" 0 workspace plus the pair)."""
    lib = engine.load_library()
    al = lambda v: (v + 255) // 256 * 256
    for (D, dt, split, B, L) in SIZES_OFF:
        E, esz = 2 * D, 2 if dt else 4
        off = _handle(lib, D, dt, f32_gemm_split=int(split), norm_fold=0)
        on = _handle(lib, D, dt, f32_gemm_split=int(split), untied_directions=1)
        grow = 2 * (al(2 * E * D * esz) + al(D * E * esz)) * (2 if split else 1)
        assert lib.pcad_weight_arena_bytes(on) - lib.pcad_weight_arena_bytes(off) == grow
        rows8 = (2 * B * L + 7) // 8 * 8
        assert lib.pcad_workspace_bytes(on, B, L) - lib.pcad_workspace_bytes(off, B, L) == 2 * al(rows8 * E * esz)
        lib.pcad_destroy(off)
        lib.pcad_destroy(on)


# ---- the GPU tests' inputs ------------------------------------------------------------------------------------------------
def test_gpu_test_inputs_can_tell_the_forms_apart():
    """tests/test_gpu_untied.py holds the engine to the oracle at 1e-4 of the output's range (fp32).  On its inputs the oracle with
    mamba_rev's own in_proj / out_proj and the oracle with mamba_rev := mamba_fwd must differ by at least 100x that, in the logits
    and in hidden_states[-1]: an engine that read 'the first of each pair' could not pass.  The literal RCPS form and the 2B-strand
    form agree on the untied weights (per-direction weights are per direction, not per strand).
    The bf16 runs tell option on from option off at 10x the bf16 bar (3e-2): that needs the plain variant of the checkpoint, on which
    the bf16-emulating oracles of the two forms are that far apart."""
    p = toy_case(stress=False)
    assert rel(p["tied_bf16"]["logits"], p["ref_bf16"]["logits"]) > 10 * 3e-2
    assert rel(p["tied_bf16"]["hidden"], p["ref_bf16"]["hidden"]) > 10 * 3e-2
    t = toy_case()
    assert rel(t["tied"]["logits"], t["ref"]["logits"]) >= 100 * 1e-4
    assert rel(t["tied"]["hidden"], t["ref"]["hidden"]) >= 100 * 1e-4
    assert rel(t["lit"]["logits"], t["ref"]["logits"]) < 1e-5 and rel(t["lit"]["hidden"], t["ref"]["hidden"]) < 1e-5
