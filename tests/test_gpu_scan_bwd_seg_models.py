"""-m gpu: `scan_bwd_segments` through both trainable models and `lora_predict train`.

Geometry: DESIGN.md §4n's toy model (tests/test_gpu_training_model.py: n_layer 2, d_model 64, d_inner 128, dt_rank 4), B = 2, L = 69, so 4
segments are three of 24, 24 and 21 steps.  A model with scan_bwd_segments=4 runs the forward of the default model - the same loss bits -
and its gradients are held to the float64 whole-model graphs and bars of tests/test_gpu_training_model.py and
tests/test_gpu_seqcls_training.py (their helpers and cached references, imported); with gradient checkpointing on, the re-run blocks use
the same segments and everything is bit-equal to checkpointing off.  Every case prints its figures before it asserts."""
import logging

import pytest
import torch

import model_bwd_ref as MB
import pool_bwd_ref as PB
import scan_bwd_ref as SB
import scan_ref as R
import test_gpu_recompute as GR
import test_gpu_seqcls_training as GC
import test_gpu_training_model as GM
from plantcaduceus_amd.checkpoint import synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = GM.DEV
F32 = torch.float32
FLOOR = (2 * GM.N_LAYER + 1) * R.BAR_SCAN[False]          # both files' floor: two summed directions per layer, and the head


def _mlm(sd, **kw):
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    m = TrainableCaduceusForMaskedLM(GM.toy_config(), dtype=F32, device=DEV, **kw)
    m.load_state_dict(sd)
    return m


def _mlm_run(sd, **kw):
    ids, labels, weights = GM.batch()
    model = _mlm(sd, **kw)
    out = model(ids.to(DEV), labels.to(DEV), weights.to(DEV))
    out.loss.backward()
    torch.cuda.synchronize()
    return out.loss.detach(), GM.grads_by_key(model)


def _held(tag, got, g64, dev32, shape_of):
    worst = 0.0
    for k in sorted(g64):
        m, bar = SB.metric(got[k], g64[k].reshape(shape_of(k))), max(FLOOR, R.ORACLE_FACTOR * dev32[k])
        worst = max(worst, m)
        print(f"  {tag} {k}: {m:.2e} [{bar:.2e}]")
        assert m <= bar, (k, m, bar)
    print(f"{tag}: worst fp32 gradient figure {worst:.2e} [floor {FLOOR:.1e}]")


def test_masked_lm_model_with_four_segments():
    cfg = GM.toy_config()
    sd = synthetic_state_dict(cfg)
    ids, labels, weights = GM.batch()
    assert ids.shape[1] == 69
    _, g64, dev32 = MB.reference("toy_f32", sd, cfg, ids, labels, weights)
    loss1, _ = _mlm_run(sd)
    loss4, got = _mlm_run(sd, scan_bwd_segments=4)
    assert torch.equal(loss1, loss4)                                      # no forward bit depends on the setting
    assert set(got) == set(g64)
    _held("masked LM, 4 segments", got, g64, dev32, lambda k: sd[k].shape)
    loss4r, gotr = _mlm_run(sd, scan_bwd_segments=4, gradient_checkpointing=True)
    assert torch.equal(loss4, loss4r)
    assert all(torch.equal(got[k], gotr[k]) for k in got)                 # a re-run block cuts its scans the same way


def _seq_run(sd, task, **kw):
    ids, labels = GC.batch(task)
    model = GC.trainable(sd, task, **kw)
    out = model(ids.to(DEV), labels.to(DEV))
    out.loss.backward()
    torch.cuda.synchronize()
    return model, out.loss.detach(), {k: p.grad for k, p in model.named_parameters() if p.grad is not None}


def test_sequence_classification_model_with_four_segments():
    task = "classification"
    cfg = GC.toy_config()
    sd = synthetic_state_dict(cfg)
    ids, labels = GC.batch(task)
    model1, loss1, _ = _seq_run(sd, task)
    _, _, g64, dev32 = PB.model_reference(task, GC.trainables(model1), sd, cfg, ids, labels, PB.TASKS[task][1])
    model4, loss4, got = _seq_run(sd, task, scan_bwd_segments=4)
    assert model4.scan_bwd_segments == 4 and model1.scan_bwd_segments == 1
    assert torch.equal(loss1, loss4)
    assert set(got) == set(g64)
    _held("sequence classification, 4 segments", got, g64, dev32, lambda k: got[k].shape)
    _, loss4r, gotr = _seq_run(sd, task, scan_bwd_segments=4, gradient_checkpointing=True)
    assert torch.equal(loss4, loss4r)
    assert all(torch.equal(got[k], gotr[k]) for k in got)


def test_lora_train_command_under_four_segments(tmp_path, monkeypatch, caplog):
    """`lora_predict train` for 3 steps under PCAD_TRAIN_SCAN_SEGMENTS=4: the setting is logged once and the adapter loads back"""
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict, pretrain
    from plantcaduceus_amd.adapters import audit_adapter, read_adapter_config, read_adapter_weights
    GR.lora_inputs(tmp_path)
    caplog.set_level(logging.INFO, logger=lora_predict.logger.name)
    monkeypatch.setenv(pretrain.SCAN_SEGMENTS_ENV, "4")
    monkeypatch.setenv(lora_predict.RECOMPUTE_ENV, "0")
    out = tmp_path / "seg4"
    GR.lora_command(tmp_path, out, "--max_steps", "3")
    said = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Segments of the scan's backward")]
    assert len(said) == 1 and said[0].endswith(": 4"), said
    print(said[0])
    cfg = read_adapter_config(str(out))
    sd = read_adapter_weights(str(out))
    audit_adapter(sd, cfg, n_layer=GR.toy_config().n_layer, d_model=GR.toy_config().d_model)
    files = load_file(str(out / "adapter_model.safetensors"))
    assert any(v.any() for k, v in files.items() if ".lora_B." in k)     # the factors did train
    assert all(bool(torch.isfinite(v).all()) for v in files.values())
