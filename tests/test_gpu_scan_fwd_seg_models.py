"""-m gpu: `scan_fwd_segments` through both trainable models and `lora_predict train`.

Geometry: tests/test_gpu_scan_bwd_seg_models.py's - the toy model (n_layer 2, d_model 64, d_inner 128, dt_rank 4), B = 2, L = 69, so 4
segments are three of 24, 24 and 21 steps.  A model with scan_fwd_segments=4 runs every scan's forward through
pcad_selective_scan_fwd_seg: its loss is held to the default model's within that file's floor ((2 n_layer + 1) x BAR_SCAN fp32: every
scan output within the scan's bar of the plain call's, two summed directions per layer and the head), its gradients to the float64
whole-model graphs and bars of tests/test_gpu_training_model.py and tests/test_gpu_seqcls_training.py (that file's `_held`); with gradient
checkpointing on, the re-run blocks cut their scans the same way and everything is bit-equal to checkpointing off.  Every case prints
its figures before it asserts."""
import logging

import pytest
import torch

import model_bwd_ref as MB
import pool_bwd_ref as PB
import test_gpu_recompute as GR
import test_gpu_scan_bwd_seg_models as BM
import test_gpu_seqcls_training as GC
import test_gpu_training_model as GM
from plantcaduceus_amd.checkpoint import synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = GM.DEV


def _loss_held(tag, loss, base):
    m = abs(loss.item() - base.item()) / abs(base.item())
    print(f"{tag}: loss {loss.item():.8f} against the default model's {base.item():.8f}: {m:.2e} [{BM.FLOOR:.1e}]")
    assert m <= BM.FLOOR, (tag, m)


@pytest.fixture
def seg_calls(monkeypatch):
    """the segment counts ops.selective_scan_fwd_seg was called with: that a model does take the new entry (a loss that agrees to the
    last bit says nothing about it)"""
    from plantcaduceus_amd import ops
    calls, real = [], ops.selective_scan_fwd_seg

    def counted(*args, **kw):
        r = real(*args, **kw)
        calls.append(r.segments)
        return r
    monkeypatch.setattr(ops, "selective_scan_fwd_seg", counted)
    return calls


def test_masked_lm_model_with_four_forward_segments(seg_calls):
    cfg = GM.toy_config()
    sd = synthetic_state_dict(cfg)
    ids, labels, weights = GM.batch()
    assert ids.shape[1] == 69
    _, g64, dev32 = MB.reference("toy_f32", sd, cfg, ids, labels, weights)
    loss1, _ = BM._mlm_run(sd)
    assert seg_calls == []                                                # the default model: today's call
    loss4, got = BM._mlm_run(sd, scan_fwd_segments=4)
    assert seg_calls == [4] * (2 * GM.N_LAYER)                            # every layer's two directions, once each
    _loss_held("masked LM, 4 forward segments", loss4, loss1)
    assert set(got) == set(g64)
    BM._held("masked LM, 4 forward segments", got, g64, dev32, lambda k: sd[k].shape)
    loss4b, gotb = BM._mlm_run(sd, scan_fwd_segments=4, scan_bwd_segments=4)
    assert torch.equal(loss4, loss4b)                                     # the backward's setting changes no forward bit
    BM._held("masked LM, 4 forward and 4 backward segments", gotb, g64, dev32, lambda k: sd[k].shape)
    loss4r, gotr = BM._mlm_run(sd, scan_fwd_segments=4, gradient_checkpointing=True)
    assert torch.equal(loss4, loss4r)
    assert all(torch.equal(got[k], gotr[k]) for k in got)                 # a re-run block cuts its scans the same way
    assert seg_calls == [4] * (2 * GM.N_LAYER * (1 + 1 + 2))              # ... so with checkpointing every scan ran twice


def test_sequence_classification_model_with_four_forward_segments(seg_calls):
    task = "classification"
    cfg = GC.toy_config()
    sd = synthetic_state_dict(cfg)
    ids, labels = GC.batch(task)
    model1, loss1, _ = BM._seq_run(sd, task)
    _, _, g64, dev32 = PB.model_reference(task, GC.trainables(model1), sd, cfg, ids, labels, PB.TASKS[task][1])
    assert seg_calls == []
    model4, loss4, got = BM._seq_run(sd, task, scan_fwd_segments=4)
    assert seg_calls == [4] * (2 * cfg.n_layer)
    assert model4.scan_fwd_segments == 4 and model4.scan_bwd_segments == 1 and model1.scan_fwd_segments == 1
    _loss_held("sequence classification, 4 forward segments", loss4, loss1)
    assert set(got) == set(g64)
    BM._held("sequence classification, 4 forward segments", got, g64, dev32, lambda k: got[k].shape)
    _, loss4r, gotr = BM._seq_run(sd, task, scan_fwd_segments=4, gradient_checkpointing=True)
    assert torch.equal(loss4, loss4r)
    assert all(torch.equal(got[k], gotr[k]) for k in got)


def test_lora_train_command_under_four_forward_segments(tmp_path, monkeypatch, caplog):
    """`lora_predict train` for 3 steps under PCAD_TRAIN_SCAN_FWD_SEGMENTS=4: the setting is logged once, the backward's stays off, and
    the adapter loads back"""
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict, pretrain
    from plantcaduceus_amd.adapters import audit_adapter, read_adapter_config, read_adapter_weights
    GR.lora_inputs(tmp_path)
    caplog.set_level(logging.INFO, logger=lora_predict.logger.name)
    monkeypatch.setenv(pretrain.SCAN_FWD_SEGMENTS_ENV, "4")
    monkeypatch.delenv(pretrain.SCAN_SEGMENTS_ENV, raising=False)
    monkeypatch.setenv(lora_predict.RECOMPUTE_ENV, "0")
    out = tmp_path / "fwdseg4"
    GR.lora_command(tmp_path, out, "--max_steps", "3")
    said = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Segments of the scan's forward")]
    assert len(said) == 1 and said[0].endswith(": 4") and pretrain.SCAN_FWD_SEGMENTS_ENV in said[0], said
    print(said[0])
    back = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Segments of the scan's backward")]
    assert len(back) == 1 and back[0].endswith(": off"), back
    cfg = read_adapter_config(str(out))
    sd = read_adapter_weights(str(out))
    audit_adapter(sd, cfg, n_layer=GR.toy_config().n_layer, d_model=GR.toy_config().d_model)
    files = load_file(str(out / "adapter_model.safetensors"))
    assert any(v.any() for k, v in files.items() if ".lora_B." in k)     # the factors did train
    assert all(bool(torch.isfinite(v).all()) for v in files.values())
