"""CPU checks of plantcaduceus_amd.pretrain and plantcaduceus_amd.optim's host side: the learning-rate schedules are
transformers.get_scheduler's, the batch source resumes bit for bit, the weight-decay rule on the real module tree's names, the
reference's flag names and defaults, and the key names of a saved snapshot."""
import dataclasses
import json
import os

import numpy as np
import pytest
import torch

from plantcaduceus_amd import mlm_eval, optim, pretrain
from plantcaduceus_amd.checkpoint import load_state_dict, make_config, synthetic_state_dict
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


@pytest.mark.parametrize("kind", pretrain.SCHEDULES)
def test_schedules_are_transformers_get_scheduler(kind):
    """every step of a 50-step run with 5 warm-up steps: the learning rate the t-th optimizer step runs at, exactly"""
    from transformers import get_scheduler
    total, warmup, lr = 50, 5, 3e-4
    p = torch.nn.Parameter(torch.zeros(1))
    opt = torch.optim.SGD([p], lr=lr)
    sched = get_scheduler(kind, opt, num_warmup_steps=warmup, num_training_steps=total)
    for t in range(total):
        assert lr * pretrain.lr_lambda(kind, t, warmup, total) == sched.get_last_lr()[0], (kind, t)
        opt.step()
        sched.step()
    assert pretrain.warmup_steps_of(0, 0.1, 50) == 5 and pretrain.warmup_steps_of(7, 0.1, 50) == 7 and pretrain.warmup_steps_of(0, 0.0, 50) == 0


def windows(n, L, seed=5):
    g = np.random.default_rng(seed)
    return ["".join(g.choice(list("ACGTacgtN"), size=L)) for _ in range(n)]


def source(batch=4, accumulation=2, seed=42, n=21, L=33):
    tok = CaduceusTokenizer()
    ids, special, w = mlm_eval.tokenize_windows(tok, windows(n, L), 0.5)
    return pretrain.BatchSource(ids, special, w, mlm_eval.make_collator(tok, 0.15), batch, accumulation, seed)


def test_batch_source_resumes_bit_for_bit():
    """window order and masks of steps k..n after a resume at step k equal the straight run's, across an epoch boundary; the global
    generator plays no part"""
    n_steps, k = 7, 3
    a = source()
    assert a.steps_per_epoch == 3                                  # ceil(21 / 4) = 6 micro-batches, 2 per step
    straight = [(a.windows(t), a.step_batches(t)) for t in range(n_steps)]
    b = source()
    torch.manual_seed(999)                                         # whatever else draws from the global generator
    for t in range(k):
        b.step_batches(t)
    saved = b.state()
    torch.rand(100)
    c = source()
    c.step_batches(0)                                              # a fresh process whose generator stands elsewhere
    c.load_state(saved)
    for t in range(k, n_steps):
        idx, batches = c.windows(t), c.step_batches(t)
        assert len(idx) == len(straight[t][0]) and all(np.array_equal(x, y) for x, y in zip(idx, straight[t][0])), t
        for got, ref in zip(batches, straight[t][1]):
            assert all(torch.equal(x, y) for x, y in zip(got, ref)), t
    # the order is a permutation per epoch, another one each epoch, and masks are drawn afresh for the same windows
    e0 = np.concatenate([np.concatenate(straight[t][0]) for t in range(3)])
    e1 = np.concatenate([np.concatenate(straight[t][0]) for t in range(3, 6)])
    assert len(set(e0.tolist())) == len(e0) == 21 and not np.array_equal(e0, e1)           # 6 micro-batches: 5 of 4 windows and one of 1
    ids, labels, w = straight[0][1][0]
    assert ids.dtype == torch.int32 and labels.dtype == torch.int32 and w.dtype == torch.float32 and ids.shape == (4, 33)
    assert bool((labels != -100).any()) and bool((labels == -100).any())
    assert source(seed=43).windows(0)[0].tolist() != straight[0][0][0].tolist()


def test_unequal_windows_are_refused():
    tok = CaduceusTokenizer()
    with pytest.raises(ValueError, match="unequal length"):
        mlm_eval.tokenize_windows(tok, ["ACGT", "ACGTA"], 1.0)


def test_decay_rule_on_the_real_module_tree():
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    model = TrainableCaduceusForMaskedLM(toy_config(), device="cpu")
    named = dict(model.named_parameters())
    off = {k for k, p in named.items() if not optim.applies_weight_decay(k, p)}
    want_off = {k for k in named if k.endswith(".bias") or k.endswith(".norm.weight") or k.endswith("norm_f.weight") or k.endswith(".A_log")
                or k.endswith(".D")}
    assert off == want_off
    leaves = {k.rsplit(".", 2)[-2] + "." + k.rsplit(".", 1)[-1] for k in off}
    assert leaves == {"conv1d.bias", "dt_proj.bias", "norm.weight", "norm_f.weight", "mamba_fwd.A_log", "mamba_fwd.D", "mamba_rev.A_log", "mamba_rev.D"}
    on = {k.rsplit(".", 2)[-2] for k in set(named) - off}
    assert on == {"in_proj", "conv1d", "x_proj", "dt_proj", "out_proj", "embedding"}     # tied tensors once: no lm_head, no second in_proj
    assert len({id(p) for p in named.values()}) == len(named)
    marked = torch.nn.Parameter(torch.zeros(2))
    marked._no_weight_decay = True
    assert not optim.applies_weight_decay("some.weight", marked) and optim.applies_weight_decay("some.weight", torch.nn.Parameter(torch.zeros(2)))
    with pytest.raises(RuntimeError, match="ROCm device"):
        optim.AdamW(model.named_parameters())                      # there is no CPU path


def test_parser_keeps_the_references_names_and_defaults():
    from transformers import TrainingArguments
    a = pretrain.build_parser().parse_args(["--dataset_name", "d", "--output_dir", "o"])
    want = dict(per_device_train_batch_size=8, per_device_eval_batch_size=8, gradient_accumulation_steps=1, learning_rate=5e-5, weight_decay=0.0,
                adam_beta1=0.9, adam_beta2=0.999, adam_epsilon=1e-8, max_grad_norm=1.0, num_train_epochs=3.0, max_steps=-1,
                lr_scheduler_type="linear", warmup_steps=0, logging_steps=500, save_steps=500, seed=42, resume_from_checkpoint=None,
                do_train=False, do_eval=False,
                mlm_probability=0.15, soft_masked_loss_weights_train=1.0, soft_masked_loss_weights_evaluation=1.0,      # HF_pre_train.py :224, :261-262
                max_train_samples=None, max_eval_samples=None, model_name_or_path=None, config_name=None, tokenizer_name=None,
                dataset_config_name=None, dtype="float32")
    for k, v in want.items():
        assert getattr(a, k) == v, k
    ta = {f.name: f.default for f in dataclasses.fields(TrainingArguments)}
    for k in ("per_device_train_batch_size", "gradient_accumulation_steps", "learning_rate", "weight_decay", "adam_beta1", "adam_beta2",
              "adam_epsilon", "max_grad_norm", "num_train_epochs", "max_steps", "warmup_steps", "logging_steps", "save_steps", "seed"):
        assert k in ta and ta[k] == getattr(a, k), (k, ta.get(k))
    assert str(getattr(ta["lr_scheduler_type"], "value", ta["lr_scheduler_type"])) == a.lr_scheduler_type
    with pytest.raises(SystemExit):
        pretrain.main(["--dataset_name", "d", "--output_dir", "o"])          # nothing to do


def test_saved_snapshot_has_caduceus_for_masked_lms_keys(tmp_path):
    from safetensors.torch import load_file
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    cfg = toy_config()
    sd = synthetic_state_dict(cfg, seed=3, stress=False)
    model = TrainableCaduceusForMaskedLM(cfg, device="cpu")
    model.load_state_dict(sd)
    out = str(tmp_path / "snap")
    pretrain.save_snapshot(model, CaduceusTokenizer(), out)
    ref_keys = set(CaduceusForMaskedLM(cfg).state_dict())
    stored = load_file(os.path.join(out, "model.safetensors"))
    assert set(stored) <= ref_keys and "lm_head.lm_head.weight" not in stored           # tied duplicates dropped, as in a real snapshot
    loaded = load_state_dict(out)
    assert set(loaded) == ref_keys == set(sd)
    assert all(torch.equal(loaded[k], sd[k]) for k in sd)
    with open(os.path.join(out, "config.json")) as f:
        assert json.load(f)["architectures"] == ["CaduceusForMaskedLM"]
    assert os.path.exists(os.path.join(out, "tokenizer_config.json"))
    m = CaduceusForMaskedLM.from_pretrained(out)
    assert set(m.state_dict()) == ref_keys
