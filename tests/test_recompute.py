"""CPU checks of gradient checkpointing behind tests/test_gpu_recompute.py: the stored-bytes formulas of §4n / §4p as code,
`lora_predict.recompute_policy`, the two commands' parsers, and the constructor keyword and HF-named methods on both trainable models.
Nothing here needs a device: the models are built on the CPU as tests/test_pool_bwd_ref.py builds them."""
import pytest
import torch

from plantcaduceus_amd import lora_predict, pretrain
from plantcaduceus_amd.checkpoint import make_config
from plantcaduceus_amd.training import (TrainableCaduceusForMaskedLM, TrainableCaduceusForSequenceClassification,
                                        stored_bytes_per_strand_position)

BF, F32 = torch.bfloat16, torch.float32


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def test_stored_bytes_formulas():
    small = make_config("pc2-small")                       # D 768, E 1 536, R 48, 24 layers, fp32 residual
    assert (small.d_model, small.d_inner, small.dt_rank, small.n_layer, bool(small.residual_in_fp32)) == (768, 1536, 48, 24, True)
    assert stored_bytes_per_strand_position(small, F32, lora=True) == 24 * 71296
    assert stored_bytes_per_strand_position(small, BF, lora=True) == 24 * 37184
    assert stored_bytes_per_strand_position(small, BF, lora=True, gradient_checkpointing=True) == 24 * 4608 + 37184
    l32 = make_config("l32")
    assert l32.d_model == 1024 and l32.residual_in_fp32
    assert stored_bytes_per_strand_position(l32, BF, lora=False) == l32.n_layer * 40 * 1024
    assert stored_bytes_per_strand_position(l32, BF, lora=False, gradient_checkpointing=True) == l32.n_layer * 6 * 1024 + 40 * 1024
    # r follows residual_in_fp32: a bf16 residual halves D r; an fp32 model's residual is fp32 either way
    lean = make_config("pc2-small", residual_in_fp32=False)
    assert stored_bytes_per_strand_position(lean, BF, lora=True) == 24 * (37184 - 2 * 768)
    assert stored_bytes_per_strand_position(lean, F32, lora=True) == 24 * 71296
    # the memory test's geometry (tests/test_gpu_recompute.py): 4 864 plain, 512 kept per layer
    toy = make_config("toy", d_model=64, n_layer=8, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))
    assert stored_bytes_per_strand_position(toy, F32, lora=False) == 8 * 4864
    assert stored_bytes_per_strand_position(toy, F32, lora=False, gradient_checkpointing=True) == 8 * 512 + 4864
    with pytest.raises(ValueError):
        stored_bytes_per_strand_position(small, torch.float16, lora=True)


def test_recompute_policy():
    policy, var = lora_predict.recompute_policy, lora_predict.RECOMPUTE_ENV
    assert var == "PCAD_TRAIN_RECOMPUTE"
    small = make_config("pc2-small")
    big = 2 * 8192 * stored_bytes_per_strand_position(small, BF, lora=True)            # 14.6e9 bytes per window
    toy = 2 * 69 * stored_bytes_per_strand_position(toy_config(), F32, lora=True)      # tests/test_gpu_lora_train.py: L 69, batch 4
    # the environment overrides whatever the bytes say
    for bytes_, batch, free, lora in ((big, 43, 288e9, True), (toy, 4, 288e9, True), (big, 43, 288e9, False), (toy, 4, 1, True)):
        assert policy(bytes_, batch, free, {var: "1"}, train_lora=lora) is True
        assert policy(bytes_, batch, free, {var: "0"}, train_lora=lora) is False
    # auto, spelled or unset
    for env in ({}, {var: "auto"}, {var: ""}):
        assert policy(toy, 4, 288e9, env) is False
        assert policy(big, 43, 288e9, env) is True
        assert policy(big, 43, 288e9, env, train_lora=False) is False
        assert policy(10 ** 15, 64, 1, env, train_lora=False) is False
    # exactly batch * bytes > free / 2
    assert policy(100, 5, 1000, {}) is False and policy(100, 5, 999, {}) is True
    with pytest.raises(ValueError, match=var):
        policy(toy, 4, 288e9, {var: "yes"})


def test_recompute_policy_reads_the_process_environment(monkeypatch):
    monkeypatch.setenv(lora_predict.RECOMPUTE_ENV, "1")
    assert lora_predict.recompute_policy(1, 1, 10 ** 12) is True
    monkeypatch.setenv(lora_predict.RECOMPUTE_ENV, "0")
    assert lora_predict.recompute_policy(10 ** 12, 64, 1) is False
    monkeypatch.delenv(lora_predict.RECOMPUTE_ENV)
    assert lora_predict.recompute_policy(1, 1, 10 ** 12) is False


def test_parsers():
    base = ["--dataset_name", "d", "--output_dir", "o"]
    assert pretrain.build_parser().parse_args(base).gradient_checkpointing is False
    assert pretrain.build_parser().parse_args(base + ["--gradient_checkpointing"]).gradient_checkpointing is True
    # `lora_predict train` gains no flag: exactly the set tests/test_pool_bwd_ref.py closes
    a = vars(lora_predict.build_parser().parse_args(["train", "--train_dir", "t", "--valid_dir", "v"]))
    assert set(a) == {name for name, _, _ in lora_predict.TRAIN_FLAGS} | {"cmd"}
    assert len(lora_predict.TRAIN_FLAGS) == 30 and not any("recompute" in k or "checkpointing" in k for k in a)
    with pytest.raises(SystemExit):
        lora_predict.build_parser().parse_args(["train", "--train_dir", "t", "--valid_dir", "v", "--gradient_checkpointing"])


def build(cls, **kw):
    if cls is TrainableCaduceusForMaskedLM:
        return cls(toy_config(), device="cpu", **kw)
    return cls(toy_config(), 2, "single_label_classification", device="cpu", **kw)


@pytest.mark.parametrize("cls", [TrainableCaduceusForMaskedLM, TrainableCaduceusForSequenceClassification])
def test_constructor_keyword_and_methods(cls):
    on = build(cls, gradient_checkpointing=True)
    assert on.is_gradient_checkpointing is True
    off = build(cls)
    assert off.is_gradient_checkpointing is False and build(cls, gradient_checkpointing=False).is_gradient_checkpointing is False
    off.gradient_checkpointing_enable()
    assert off.is_gradient_checkpointing is True
    off.gradient_checkpointing_disable()
    assert off.is_gradient_checkpointing is False
    on.gradient_checkpointing_disable()
    assert on.is_gradient_checkpointing is False
    # the option adds no parameter, buffer or state-dict key
    assert set(on.state_dict()) == set(off.state_dict())
    assert [k for k, _ in on.named_parameters()] == [k for k, _ in off.named_parameters()]


def test_from_pretrained_passes_the_keyword_through(tmp_path):
    from plantcaduceus_amd.checkpoint import save_checkpoint, synthetic_state_dict
    cfg = toy_config()
    save_checkpoint(str(tmp_path), cfg, synthetic_state_dict(cfg, stress=False), with_tokenizer=False)
    for kw, want in (({}, False), ({"gradient_checkpointing": True}, True)):
        assert TrainableCaduceusForMaskedLM.from_pretrained(str(tmp_path), device="cpu", **kw).is_gradient_checkpointing is want
        assert TrainableCaduceusForSequenceClassification.from_pretrained(str(tmp_path), 2, "single_label_classification", device="cpu",
                                                                          **kw).is_gradient_checkpointing is want
