"""-m gpu: gradient checkpointing in both trainable models (plantcaduceus_amd/training.py).  With the option on every block
keeps only its inputs and its forward runs again inside the backward, on the same operators - so everything below is held to
torch.equal against the same model with the option off, never to a tolerance.

Geometry: the toy config of tests/test_gpu_training_model.py (d_model 64, d_inner 128, dt_rank 4), B = 2, L = 69.
  masked LM       n_layer 1 and 3, fp32 and bf16, about 15 % of window 0 labelled and window 1 without any label, with loss_weights; one
                  state dict in both models: loss, sums, token_nll and every parameter's .grad, after one backward and again after a second
                  micro-batch accumulated on top
  classification  lora_B = 0.05 N(0, 1); the three problem types in fp32 and classification in bf16: logits, loss, every trainable
                  gradient; frozen parameters have no gradient.  Block 0's input does not require grad (frozen embedding)
  inertness       a counting wrapper around ops.selective_scan_fn sees 4 n_layer calls for a training step with the option on (two
                  directions, each block twice), 2 n_layer with train_lora=False and 2 n_layer under torch.no_grad()
  memory          masked LM, fp32, n_layer 8, B = 2, L = 512: peak bytes above the baseline of one forward + backward, on <= 0.5 x off.
                  The formula (training.stored_bytes_per_strand_position) gives (8 x 512 + 4 864) / (8 x 4 864) = 0.23; the half leaves
                  room for the weight gradients and the operators' transient copies, and still fails if an operator keeps its activations
  commands        `pretrain` 6 steps with and without --gradient_checkpointing: model.safetensors and the logged losses equal;
                  `lora_predict train` 6 steps under PCAD_TRAIN_RECOMPUTE=1 and =0, and resumed from checkpoint-3 under the other
                  setting: adapter_model.safetensors equal
Every case prints its figures before it asserts.

Observed on an MI355X: every comparison bit-equal (masked LM 19 of 19 and 53 of 53 gradients, LoRA model 25 of 25); selective_scan_fn
calls 8 / 4 / 4 / 4 at n_layer 2; memory: plain 92 636 160 bytes above the baseline, recompute 25 887 744, ratio 0.279 [0.5; the formula's
stored bytes 79 691 776 / 18 350 080 = 0.230]; pretrain's six losses 2.276136 .. 1.566795 in both runs."""
import json
import logging

import numpy as np
import pytest
import torch

import pool_bwd_ref as PB
from plantcaduceus_amd.checkpoint import make_config, save_checkpoint, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
B, L, SEED = 2, 69, 42


def toy_config(n_layer=2):
    return make_config("toy", d_model=64, n_layer=n_layer, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def same(a, b):
    return (a is None and b is None) or (a is not None and b is not None and a.dtype == b.dtype and torch.equal(a, b))


# ---- masked LM ------------------------------------------------------------------------------------------------------------------------
def mlm_batch(seed, length=L):
    """ids, labels (about 15 % of window 0; window 1 has none), loss_weights"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 7, (B, length), generator=g)
    keep = torch.rand(B, length, generator=g) < 0.15
    keep[0, 3] = True
    keep[1] = False
    labels = torch.where(keep, torch.randint(0, 8, (B, length), generator=g), torch.full((B, length), -100)).to(torch.int32)
    weights = torch.tensor([0.0, 0.1, 1.0, 2.5])[torch.randint(0, 4, (B, length), generator=g)]
    weights[0, 3] = 1.0
    return ids.to(DEV), labels.to(DEV), weights.to(DEV)


def mlm_model(cfg, sd, dtype, recompute):
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    m = TrainableCaduceusForMaskedLM(cfg, dtype=dtype, device=DEV, gradient_checkpointing=recompute)
    assert m.is_gradient_checkpointing is recompute
    m.load_state_dict(sd)
    return m


def mlm_run(cfg, sd, dtype, recompute):
    """two micro-batches, the second accumulated onto the first -> per micro-batch (loss, sums, token_nll, {name: grad clone})"""
    model = mlm_model(cfg, sd, dtype, recompute)
    out = []
    for seed in (17, 18):
        o = model(*mlm_batch(seed), return_token_nll=True)
        o.loss.backward()
        torch.cuda.synchronize()
        out.append((o.loss.detach().clone(), o.sums.detach().clone(), o.token_nll.detach().clone(),
                    {k: (p.grad.clone() if p.grad is not None else None) for k, p in model.named_parameters()}))
    return out


@pytest.mark.parametrize("dtype", [F32, BF], ids=["fp32", "bf16"])
@pytest.mark.parametrize("n_layer", [1, 3])
def test_masked_lm_is_bit_equal(n_layer, dtype):
    cfg = toy_config(n_layer)
    sd = synthetic_state_dict(cfg)
    on, off = mlm_run(cfg, sd, dtype, True), mlm_run(cfg, sd, dtype, False)
    for step, ((loss_a, sums_a, nll_a, g_a), (loss_b, sums_b, nll_b, g_b)) in enumerate(zip(on, off)):
        differ = [k for k in g_b if not same(g_a[k], g_b[k])]
        print(f"n_layer {n_layer} {dtype} after micro-batch {step + 1}: loss {loss_a.item():.7f} / {loss_b.item():.7f}; "
              f"{len(g_b) - len(differ)} of {len(g_b)} gradients bit-equal{': not ' + ', '.join(differ[:4]) if differ else ''}")
        assert torch.isfinite(loss_b) and sums_b[1, 2] == 0 and sums_b[0, 2] > 0            # window 1 has no label
        assert all(g is not None and g.dtype == dtype and bool(torch.isfinite(g).all()) for g in g_b.values())
        assert torch.equal(loss_a, loss_b) and torch.equal(sums_a, sums_b) and torch.equal(nll_a, nll_b)
        assert set(g_a) == set(g_b) and not differ, differ
    assert any(not torch.equal(on[0][3][k], on[1][3][k]) for k in on[0][3])                   # the second micro-batch did accumulate


# ---- sequence classification ------------------------------------------------------------------------------------------------------------
def cls_batch(task):
    g = torch.Generator().manual_seed(23)
    ids = torch.randint(3, 7, (B, L), generator=g)
    nl = PB.TASKS[task][0]
    labels = {"classification": torch.tensor([1, 0]), "regression": torch.randn(B, generator=g),
              "multi_label": (torch.rand(B, nl, generator=g) < 0.5).float()}[task]
    return ids.to(DEV), labels.to(DEV)


def cls_model(sd, task, dtype, recompute, n_layer=2, **kw):
    """the model with lora_B = 0.05 N(0, 1), seeded (tests/test_gpu_seqcls_training.py's)"""
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    nl, problem = PB.TASKS[task]
    m = TrainableCaduceusForSequenceClassification(toy_config(n_layer), nl, problem, dtype=dtype, device=DEV, gradient_checkpointing=recompute, **kw)
    assert m.is_gradient_checkpointing is recompute
    m.load_trunk({k: v for k, v in sd.items() if k.startswith("caduceus.")})
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".lora_B." in k:
                p.copy_((torch.randn(p.shape, generator=g) * 0.05).to(DEV))
    return m


@pytest.mark.parametrize("task,dtype", [("classification", F32), ("regression", F32), ("multi_label", F32), ("classification", BF)],
                         ids=["classification-fp32", "regression-fp32", "multi_label-fp32", "classification-bf16"])
def test_sequence_classification_is_bit_equal(task, dtype):
    sd = synthetic_state_dict(toy_config())
    ids, labels = cls_batch(task)
    res = {}
    for recompute in (True, False):
        model = cls_model(sd, task, dtype, recompute)
        out = model(ids, labels)
        out.loss.backward()
        torch.cuda.synchronize()
        res[recompute] = (out.loss.detach(), out.logits.detach(), {k: p.grad for k, p in model.named_parameters()},
                          {k for k, p in model.named_parameters() if p.requires_grad})
    (loss_a, logits_a, g_a, train_a), (loss_b, logits_b, g_b, train_b) = res[True], res[False]
    differ = [k for k in g_b if not same(g_a[k], g_b[k])]
    print(f"{task} {dtype}: loss {loss_a.item():.7f} / {loss_b.item():.7f}; {len(train_b)} trainable gradients, "
          f"{len(differ)} differ{': ' + ', '.join(differ[:4]) if differ else ''}")
    assert train_a == train_b and len(train_b) == 2 * 2 * 3 * 2 + 1
    for g in (g_a, g_b):
        assert all((g[k] is not None) == (k in train_b) for k in g)                          # frozen parameters: grad is None
        assert all(bool(g[k].abs().sum() > 0) for k in train_b), [k for k in train_b if not g[k].abs().sum() > 0]      # block 0's factors too
    assert torch.equal(loss_a, loss_b) and torch.equal(logits_a, logits_b) and logits_a.dtype == F32
    assert not differ, differ


# ---- nothing to differentiate means nothing re-run ------------------------------------------------------------------------------------
@pytest.fixture
def scan_calls(monkeypatch):
    from plantcaduceus_amd import ops
    calls, real = [], ops.selective_scan_fn

    def counted(*a, **kw):
        calls.append(bool(kw.get("reverse", False)))
        return real(*a, **kw)
    monkeypatch.setattr(ops, "selective_scan_fn", counted)
    return calls


def test_recompute_runs_each_block_twice_only_where_there_is_something_to_differentiate(scan_calls):
    n_layer = 2
    sd = synthetic_state_dict(toy_config(n_layer))
    ids, labels = cls_batch("classification")

    def count(fn):
        del scan_calls[:]
        out = fn()
        torch.cuda.synchronize()
        return len(scan_calls), out

    def step(model):
        out = model(ids, labels)
        out.loss.backward()
        return out.logits.detach()
    seen = {}
    on, off = cls_model(sd, "classification", F32, True), cls_model(sd, "classification", F32, False)
    seen["train, on"], _ = count(lambda: step(on))
    seen["train, off"], _ = count(lambda: step(off))
    with torch.no_grad():
        seen["no_grad, on"], lg_on = count(lambda: on(ids).logits)
        seen["no_grad, off"], lg_off = count(lambda: off(ids).logits)
    f_on, f_off = (cls_model(sd, "classification", F32, r, train_lora=False) for r in (True, False))
    seen["train_lora=False, on"], fl_on = count(lambda: step(f_on))
    seen["train_lora=False, off"], fl_off = count(lambda: step(f_off))
    # the masked LM's composed path calls the same entry point
    cfg = toy_config(n_layer)
    seen["masked LM train, on"], _ = count(lambda: mlm_model(cfg, sd, F32, True)(*mlm_batch(17)).loss.backward())
    seen["masked LM train, off"], _ = count(lambda: mlm_model(cfg, sd, F32, False)(*mlm_batch(17)).loss.backward())
    print("selective_scan_fn calls: " + "; ".join(f"{k} {v}" for k, v in seen.items()))
    assert seen == {"train, on": 4 * n_layer, "train, off": 2 * n_layer, "no_grad, on": 2 * n_layer, "no_grad, off": 2 * n_layer,
                    "train_lora=False, on": 2 * n_layer, "train_lora=False, off": 2 * n_layer,
                    "masked LM train, on": 4 * n_layer, "masked LM train, off": 2 * n_layer}
    assert torch.equal(lg_on, lg_off) and torch.equal(fl_on, fl_off)
    assert same(f_on.score.weight.grad, f_off.score.weight.grad) and f_on.score.weight.grad is not None
    # the switch is live: turned off, the same model runs each block once again
    on.gradient_checkpointing_disable()
    assert count(lambda: step(on))[0] == 2 * n_layer
    off.gradient_checkpointing_enable()
    assert count(lambda: step(off))[0] == 4 * n_layer


# ---- it frees memory ------------------------------------------------------------------------------------------------------------------
def test_recompute_halves_the_peak_at_least():
    from plantcaduceus_amd.training import stored_bytes_per_strand_position
    n_layer, length = 8, 512
    cfg = toy_config(n_layer)
    model = mlm_model(cfg, synthetic_state_dict(cfg), F32, False)
    batch = mlm_batch(17, length)

    def peak():
        """bytes one forward + backward reaches above what is allocated before it (the model, the inputs, the libraries' workspaces)"""
        model.zero_grad(set_to_none=True)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        model(*batch).loss.backward()
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - base
    peak()                                                                       # first use: workspaces and handles are created once
    off = peak()
    model.gradient_checkpointing_enable()
    on = peak()
    strands = 2 * B * length
    f_off = strands * stored_bytes_per_strand_position(cfg, F32, lora=False)
    f_on = strands * stored_bytes_per_strand_position(cfg, F32, lora=False, gradient_checkpointing=True)
    print(f"peak above the baseline: off {off} bytes, on {on} bytes, ratio {on / off:.3f} [0.5]; stored by the formula {f_off} / {f_on}, "
          f"ratio {f_on / f_off:.3f}")
    assert f_off == 8 * 4864 * 2048 and f_off > 79e6
    assert off >= f_off                                                          # the plain run keeps at least what the formula counts
    assert on <= 0.5 * off


# ---- the commands -----------------------------------------------------------------------------------------------------------------------
N_WIN, BATCH, LR = 8, 4, 1e-3


def test_pretrain_with_the_flag_is_bit_equal(tmp_path):
    """the fixtures of tests/test_gpu_pretrain.py: 8 windows of L = 69, batch 4, fp32, lr 1e-3, constant schedule, 6 steps"""
    from safetensors.torch import load_file
    from plantcaduceus_amd import pretrain
    g = np.random.default_rng(9)
    seqs = ["".join(g.choice(list("ACGTacgt"), size=L)) for _ in range(N_WIN)]
    data = tmp_path / "data"
    data.mkdir()
    with open(data / "train.tsv", "w") as f:
        f.write("seq\n" + "\n".join(seqs) + "\n")
    cfg = toy_config()
    save_checkpoint(str(tmp_path / "cfg"), cfg, synthetic_state_dict(cfg, seed=SEED, stress=False), with_tokenizer=False)
    hist = {}
    for name, extra in (("plain", []), ("recompute", ["--gradient_checkpointing"])):
        pretrain.main(["--config_name", str(tmp_path / "cfg" / "config.json"), "--dataset_name", str(data), "--do_train", "--output_dir",
                       str(tmp_path / name), "--per_device_train_batch_size", str(BATCH), "--learning_rate", str(LR), "--lr_scheduler_type",
                       "constant", "--max_steps", "6", "--logging_steps", "1", "--save_steps", "3", "--seed", str(SEED), "--device", DEV, *extra])
        with open(tmp_path / name / "trainer_state.json") as f:
            hist[name] = json.load(f)["log_history"]
    wa, wb = load_file(str(tmp_path / "plain" / "model.safetensors")), load_file(str(tmp_path / "recompute" / "model.safetensors"))
    la, lb = [e["loss"] for e in hist["plain"]], [e["loss"] for e in hist["recompute"]]
    print(f"pretrain: losses plain {[round(x, 6) for x in la]} recompute {[round(x, 6) for x in lb]}; "
          f"max |d parameter| {max((wa[k].double() - wb[k].double()).abs().max().item() for k in wa):.3e}")
    assert len(la) == 6 and la == lb and [e["grad_norm"] for e in hist["plain"]] == [e["grad_norm"] for e in hist["recompute"]]
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)


def lora_inputs(tmp):
    """the fixtures of tests/test_gpu_lora_train.py: 16 training and 8 validation windows of L = 69, labelled by G+C content"""
    import pyarrow as pa
    import pyarrow.parquet as pq
    g = np.random.default_rng(11)

    def draw(n):
        gc = g.uniform(0.15, 0.85, size=n)
        is_gc, first = g.random((n, L)) < gc[:, None], g.random((n, L)) < 0.5
        return np.where(is_gc, np.where(first, 4, 5), np.where(first, 3, 6)).astype(np.int32)
    tr, va = draw(16), draw(8)
    frac = lambda x: ((x == 4) | (x == 5)).mean(1)
    cut = float(np.median(frac(tr)))
    for name, x in (("train", tr), ("valid", va)):
        pq.write_table(pa.table({"input_ids": pa.array(list(x), type=pa.list_(pa.int32())), "label": pa.array((frac(x) > cut).astype(np.int64))}),
                       str(tmp / f"{name}.parquet"))
    save_checkpoint(str(tmp / "base"), toy_config(), synthetic_state_dict(toy_config(), seed=SEED, stress=False))


def lora_command(tmp, out, *extra):
    from plantcaduceus_amd import lora_predict
    return lora_predict.main(["train", "--train_dir", str(tmp / "train.parquet"), "--valid_dir", str(tmp / "valid.parquet"), "--model_name",
                              str(tmp / "base"), "--output_dir", str(out), "--train_batch_size", str(BATCH), "--eval_batch_size", "4",
                              "--gradient_accumulation_steps", "1", "--learning_rate", str(LR), "--lr_scheduler_type", "constant",
                              "--warmup_steps", "0", "--max_steps", "6", "--logging_steps", "1", "--eval_steps", "3", "--save_steps", "3",
                              "--seed", str(SEED), "--device", DEV, *extra])


def test_lora_train_under_either_setting_is_bit_equal(tmp_path, monkeypatch, caplog):
    from safetensors.torch import load_file
    from plantcaduceus_amd import lora_predict
    lora_inputs(tmp_path)
    caplog.set_level(logging.INFO, logger=lora_predict.logger.name)
    runs = (("on", "1", []), ("off", "0", []), ("auto", None, []),
            ("on_then_off", "0", ["--resume_from_checkpoint", str(tmp_path / "on" / "checkpoint-3")]),
            ("off_then_on", "1", ["--resume_from_checkpoint", str(tmp_path / "off" / "checkpoint-3")]))
    decided, files = {}, {}
    for name, env, extra in runs:
        if env is None:
            monkeypatch.delenv(lora_predict.RECOMPUTE_ENV, raising=False)
        else:
            monkeypatch.setenv(lora_predict.RECOMPUTE_ENV, env)
        caplog.clear()
        lora_command(tmp_path, tmp_path / name, *extra)
        said = [r.getMessage() for r in caplog.records if r.getMessage().startswith("Recompute blocks in the backward")]
        assert len(said) == 1, said
        decided[name] = said[0]
        files[name] = load_file(str(tmp_path / name / "adapter_model.safetensors"))
        with open(tmp_path / name / "trainer_state.json") as f:
            state = json.load(f)
        with open(tmp_path / name / "train_results.json") as f:
            results = json.load(f)
        assert not any("recompute" in k.lower() or "checkpointing" in k.lower() for k in list(state) + list(results))
    for name, text in decided.items():
        print(f"{name}: {text}")
    want = {"on": "on", "off": "off", "auto": "off", "on_then_off": "off", "off_then_on": "on"}         # auto is off at the toy sizes
    assert all(f"): {want[k]};" in decided[k] for k in want), decided
    ref = files["off"]
    assert any(v.any() for k, v in ref.items() if ".lora_B." in k)                                     # the factors did train
    for name in ("on", "auto", "on_then_off", "off_then_on"):
        worst = max((ref[k].double() - files[name][k].double()).abs().max().item() for k in ref)
        print(f"{name} against off: max |d parameter| {worst:.3e}")
        assert set(files[name]) == set(ref) and all(torch.equal(files[name][k], ref[k]) for k in ref), name
