"""CPU checks behind tests/test_gpu_pool_bwd.py, tests/test_gpu_seqcls_training.py and tests/test_gpu_lora_train.py: the
restatement of tests/pool_bwd_ref.py is tests/seqcls_ref.py's head and its autograd gradients are the derivatives (central finite
differences in float64); pcad_pooled_head_bwd sizes its scratch and refuses bad arguments before any device work; ops.lora_linear_fn's
backward formulas are autograd's through the merged weight; TrainableCaduceusForSequenceClassification writes an adapter that the
adapter loader's audit accepts; and `lora_predict train` has the reference train()'s flags and defaults."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import pool_bwd_ref as PB
import scan_bwd_ref as SB
import seqcls_ref as SR
from plantcaduceus_amd import adapters, engine, lora_predict, ops
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE


def toy_config(**kw):
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True), **kw)


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


@pytest.mark.parametrize("pooling", PB.POOLINGS)
@pytest.mark.parametrize("bf", [False, True])
def test_restatement_is_seqcls_refs_head(pooling, bf):
    """logits and pooled against seqcls_ref.pool_strands + score_ref on the same normed rows, fp32 and with bf16 rounding points"""
    c = PB.inputs(5, 3, 37, 48, 5, pooling, bf=bf)
    B, L, D = c["B"], c["L"], 48
    dtype = torch.bfloat16 if bf else torch.float32
    with torch.no_grad():
        lg, pooled = PB.head(c["h"], c["res"], c["norm_weight"], c["score_w"], B, L, pooling, c["eps"], bf=bf)
        v = (c["h"].double() + c["res"].double()).view(2 * B, L, D)
        o = SR.rnd((v * torch.rsqrt(v.pow(2).mean(-1, keepdim=True) + c["eps"]) * c["norm_weight"].double()).float(), dtype)
    want_pooled = SR.pool_strands(o[:B], o[B:], pooling, dtype)
    want = SR.score_ref(want_pooled, c["score_w"], dtype)
    m, p = SB.metric(lg, want), SB.metric(pooled, want_pooled)
    print(f"pooled head restatement {pooling} bf={bf}: logits {m:.3e}, pooled {p:.3e}")
    assert m < (2.0 ** -7 if bf else 1e-6) and p < (2.0 ** -8 if bf else 1e-6)


@pytest.mark.parametrize("pooling", PB.POOLINGS)
def test_restatement_gradients_are_the_derivatives(pooling):
    """central differences of sum(dlogits * logits) in float64 over every coordinate of h, res, norm_weight and score_w, step 1e-6,
    held to 1e-6 of each gradient's maximum (as tests/test_head_bwd_ref.py)"""
    c = PB.inputs(3, 2, 5, 8, 3, pooling)
    g = PB.grads(c)

    def loss(d):
        lg, _ = PB.head(d["h"], d["res"], d["norm_weight"], d["score_w"], d["B"], d["L"], pooling, d["eps"])
        return (lg * d["dlogits"].double()).sum().item()
    eps = 1e-6
    for name in PB.NAMES:
        base = c[name].double()
        fd = torch.zeros_like(base).reshape(-1)
        for i in range(base.numel()):
            vals = []
            for sign in (1.0, -1.0):
                t = base.clone().reshape(-1)
                t[i] += sign * eps
                vals.append(loss(dict(c, **{name: t.reshape(base.shape)})))
            fd[i] = (vals[0] - vals[1]) / (2 * eps)
        err = (fd.reshape(base.shape) - g[name]).abs().max().item() / g[name].abs().max().item()
        print(f"finite differences {pooling} {name}: {err:.3e}")
        assert err < 1e-6, name
    assert torch.equal(g["h"], g["res"])
    rows = g["h"].view(4, 5, -1)
    if pooling != "mean":                   # only the pooled row of each strand carries a gradient
        keep = 0 if pooling == "first" else 4
        assert all((rows[:, t] == 0).all() for t in range(5) if t != keep) and (rows[:, keep] != 0).any()


def test_straight_through_rounding_leaves_the_derivative():
    """the bf16 graph's gradients are the unrounded graph's formulas at the same operands: the roundings are identities in the
    derivative, and the cotangent of a row does not depend on any rounded forward value"""
    c = PB.inputs(9, 2, 7, 16, 2, "mean", bf=True)
    a, b = PB.grads(c), PB.grads(dict(c, bf=False))
    for k in ("h", "res", "norm_weight"):
        assert SB.metric(a[k], b[k]) < 1e-12, k
    assert SB.metric(a["score_w"], b["score_w"]) < 2.0 ** -7        # through pooled, which the forward rounded


def test_segment_matches_the_kernels():
    hpp = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    fwd = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "pool.hip")).read()
    seg = int(re.search(r"constexpr int POOL_BWD_SEG = (\d+);", hpp).group(1))
    assert seg == ops.POOL_BWD_SEG == PB.SEG == int(re.search(r"constexpr int POOL_SEG = (\d+);", fwd).group(1))


def scratch_formula(B, L, D, pooling):
    """the windows' cotangent rows [B, D], then one row of D fp32 partials per (window, strand, segment of POOL_BWD_SEG rows)
    - first / last: per (window, strand) -, each part rounded up to 256 bytes"""
    r256 = lambda n: (n + 255) // 256 * 256
    nseg = (L + ops.POOL_BWD_SEG - 1) // ops.POOL_BWD_SEG if pooling == 0 else 1
    return r256(B * D * 4) + r256(B * 2 * nseg * D * 4)


def test_scratch_bytes(lib):
    f, G = lib.pcad_pooled_head_bwd_scratch_bytes, ops.POOL_BWD_SEG
    for pooling in (0, 2, 3):
        prev = None
        for args in ((1, 1, 8), (2, 1, 8), (2, G, 8), (2, G + 1, 8), (2, G + 1, 384), (3, 2 * G + 5, 384), (4, 8192, 768), (4, 8192, 2048),
                     (4096, 8192, 2048)):
            n = f(*args, pooling)
            assert n > 0 and n % 256 == 0 and (prev is None or n >= prev), (args, pooling)
            assert n == scratch_formula(*args, pooling), (args, pooling)
            prev = n
    assert f(4096, 8192, 2048, 0) > 2 ** 32
    assert f(4, 8192, 768, 0) == 4 * 768 * 4 + 4 * 2 * 128 * 768 * 4 == 3158016                      # the figure DESIGN.md §4p states
    assert f(2, G + 1, 384, 0) > f(2, G, 384, 0) and f(2, G + 1, 384, 2) == f(2, G, 384, 2) == f(2, G, 384, 3)
    assert f(0, 5, 384, 0) == 0 and f(2, 0, 384, 0) == 0 and f(2, 5, 0, 0) == 0
    assert f(2, 5, 384, 1) == 0 and f(2, 5, 384, 9) == 0            # max pooling and unknown poolings have no backward


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor.  Every call below is
    refused before the launch (or has nothing to do): none may reach a device with these pointers."""
    p = 0x10000
    last = engine.load_library().pcad_last_error

    def call(h=p, res=p, w=p, W=p, pooled=p, dl=p, dh=p, dres=p, dw=p, dW=p, scratch=p, nbytes=1 << 40, B=2, L=70, D=384, NL=5, pooling=0,
             dtype=0, rdt=0):
        return lib.pcad_pooled_head_bwd(h, res, w, W, pooled, dl, dh, dres, dw, dW, scratch, nbytes, B, L, D, NL, 1e-5, pooling, dtype, rdt, None)
    for name, word in (("h", b"h"), ("res", b"res"), ("w", b"norm_weight"), ("W", b"score_w"), ("pooled", b"pooled"), ("dl", b"dlogits")):
        assert call(**{name: None}) == INV and b"null " + word in last(), name
    assert call(pooling=1) == INV and b"pooling" in last() and b"PCAD_POOL_MAX" in last()
    assert call(pooling=7) == INV and b"pooling" in last()
    assert call(dh=None, dres=None, dw=None, dW=None) == INV and b"no output" in last()
    assert call(NL=0) == INV and b"num_labels" in last()
    assert call(NL=257) == INV and b"num_labels" in last()
    assert call(D=388) == INV and b"D" in last()
    assert call(D=2056) == INV and b"2048" in last()
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(dtype=0, rdt=1) == INV and b"res_dtype" in last()
    for name in ("h", "res", "w", "dh", "dres"):
        assert call(**{name: p + 8}) == INV and b"16-byte aligned" in last(), name
    assert call(B=-1) == INV and call(L=0) == INV
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    assert call(nbytes=scratch_formula(2, 70, 384, 0) - 1) == WSP
    assert call(B=0, scratch=None, nbytes=0) == 0                    # nothing to do: OK before the scratch is looked at


def test_lora_linear_backward_is_autograd_through_the_merged_weight():
    """float64 on the CPU: dx = dy W_eff, dB = scale dy^T (x A^T), dA = scale (dy B)^T x against autograd of F.linear(x, W + scale B A)"""
    g = torch.Generator().manual_seed(2)
    mk = lambda *s: torch.randn(*s, generator=g, dtype=torch.float64)
    x, W, A, B, dy, scale = mk(3, 7, 12), mk(10, 12), mk(4, 12), mk(10, 4), mk(3, 7, 10), 32 / 8
    lv = [t.clone().requires_grad_(True) for t in (x, A, B)]
    (ops.lora_linear_fn(lv[0], W, lv[1], lv[2], scale) * dy).sum().backward()
    rv = [t.clone().requires_grad_(True) for t in (x, A, B)]
    Wl = W.clone().requires_grad_(True)
    ref = F.linear(rv[0], Wl + scale * rv[2] @ rv[1])
    (ref * dy).sum().backward()
    with torch.no_grad():
        assert SB.metric(ops.lora_linear_fn(x, W, A, B, scale), ref) < 1e-12         # the plain call
    for name, a, b in zip(("x", "A", "B"), lv, rv):
        m = SB.metric(a.grad, b.grad)
        print(f"lora_linear_fn d{name}: {m:.3e}")
        assert m < 1e-12 and a.grad.shape == a.shape and a.grad.dtype == a.dtype
    # W gets no gradient, and the factors are fp32 whatever x's dtype
    Wg = W.clone().requires_grad_(True)
    ops.lora_linear_fn(lv[0], Wg, lv[1], lv[2], scale).sum().backward()
    assert Wg.grad is None
    xb, Ab, Bb = x.bfloat16().requires_grad_(True), A.float().requires_grad_(True), B.float().requires_grad_(True)
    y = ops.lora_linear_fn(xb, W.bfloat16(), Ab, Bb, scale)
    y.float().sum().backward()
    assert y.dtype == torch.bfloat16 and xb.grad.dtype == torch.bfloat16 and Ab.grad.dtype == torch.float32 and Bb.grad.dtype == torch.float32
    assert torch.equal(y.detach(), F.linear(xb.detach(), (W.bfloat16().float() + scale * (B.float() @ A.float())).to(torch.bfloat16)))


def trainable(**kw):
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    cfg = toy_config()
    m = TrainableCaduceusForSequenceClassification(cfg, kw.pop("num_labels", 2), kw.pop("problem_type", "single_label_classification"), device="cpu", **kw)
    m.load_trunk({k: v for k, v in synthetic_state_dict(cfg).items() if k.startswith("caduceus.")})
    return m, cfg


def test_trainable_model_structure():
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification as T
    m, cfg = trainable()
    named = dict(m.named_parameters())
    factors = [k for k in named if ".lora_" in k]
    assert len(factors) == cfg.n_layer * 2 * 3 * 2 and all(adapters._LORA_RE.match(k) for k in factors)
    assert {k for k, p in named.items() if p.requires_grad} == set(factors) | {"score.weight"}
    assert all(named[k].dtype == torch.float32 for k in factors) and named["score.weight"].shape == (2, cfg.d_model)
    for k in factors:                       # PEFT's initial values: A ~ U(+-1/sqrt(in)), B = 0
        if ".lora_B." in k:
            assert not named[k].any()
        else:
            assert 0 < named[k].abs().max() <= named[k].shape[1] ** -0.5
    assert abs(named["score.weight"]).max() <= cfg.d_model ** -0.5
    frozen, _ = trainable(train_lora=False)
    assert [k for k, p in frozen.named_parameters() if p.requires_grad] == ["score.weight"]
    bf, _ = trainable(dtype=torch.bfloat16)
    nb = dict(bf.named_parameters())
    assert nb["caduceus.backbone.norm_f.weight"].dtype == torch.bfloat16 and nb["score.weight"].dtype == torch.float32
    assert all(nb[k].dtype == torch.float32 for k in factors)
    with pytest.raises(NotImplementedError, match="max"):
        T(cfg, 2, "single_label_classification", pooling_strategy="max", device="cpu")
    with pytest.raises(NotImplementedError):
        T(toy_config(bidirectional_weight_tie=False), 2, "single_label_classification", device="cpu")
    with pytest.raises(RuntimeError, match="ROCm"):
        m(torch.zeros(1, 8, dtype=torch.long))


def test_save_adapter_round_trip(tmp_path):
    m, cfg = trainable(num_labels=5, problem_type="multi_label_classification")
    d = str(tmp_path / "adapter")
    m.save_adapter(d, "some/base")
    ac = adapters.read_adapter_config(d)
    assert (ac["r"], ac["lora_alpha"], ac["task_type"], ac["lora_dropout"], ac["peft_type"], ac["bias"], ac["inference_mode"]) == \
        (8, 32, "SEQ_CLS", 0.0, "LORA", "none", True)
    assert ac["target_modules"] == sorted(adapters.TARGETS) and "score" in ac["modules_to_save"] and ac["base_model_name_or_path"] == "some/base"
    sd = adapters.read_adapter_weights(d)
    assert all(k.startswith("base_model.model.") for k in sd)
    aud = adapters.audit_adapter(sd, ac, n_layer=cfg.n_layer, d_model=cfg.d_model)
    assert set(aud["lora"]) == {(i, dr, mod) for i in range(cfg.n_layer) for dr in ("fwd", "rev") for mod in adapters.TARGETS}
    assert all(set(ab) == {"A", "B"} for ab in aud["lora"].values()) and tuple(aud["score"].shape) == (5, cfg.d_model)
    assert adapters.lora_delta_report(aud["lora"], ac["r"], ac["lora_alpha"]) == {"nonzero": [], "max_abs_delta": 0.0}
    # a perturbed model: merge_lora of what it saved is W + (alpha / r) B A, per direction
    g = torch.Generator().manual_seed(1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if ".lora_B." in k:
                p.copy_(torch.randn(p.shape, generator=g) * 0.05)
    m.save_adapter(d, "some/base")
    aud = adapters.audit_adapter(adapters.read_adapter_weights(d), ac, n_layer=cfg.n_layer, d_model=cfg.d_model)
    assert len(adapters.lora_delta_report(aud["lora"], 8, 32)["nonzero"]) == cfg.n_layer * 2 * 3
    base = {k: v for k, v in synthetic_state_dict(cfg).items() if k.startswith("caduceus.")}
    merged = adapters.merge_lora(base, aud["lora"], 8, 32)
    named = dict(m.named_parameters())
    for (i, dr, mod) in aud["lora"]:
        k = f"caduceus.backbone.layers.{i}.mixer.submodule.mamba_{dr}.{mod}"
        src = k + ".weight" if k + ".weight" in base else k.replace("mamba_rev", "mamba_fwd") + ".weight"
        want = base[src].float() + 4.0 * (named[k + ".lora_B.weight"].float() @ named[k + ".lora_A.weight"].float())
        assert torch.equal(merged[k + ".weight"], want), k
        assert torch.equal(ops._lora_merged(base[src], named[k + ".lora_A.weight"], named[k + ".lora_B.weight"], 4.0, torch.float32), want), k
    # and back into a fresh model
    other, _ = trainable(num_labels=5, problem_type="multi_label_classification", seed=7)
    other.load_adapter_weights(d)
    assert all(torch.equal(p, dict(other.named_parameters())[k]) for k, p in m.named_parameters())


# the reference train()'s signature (src/lora_fine_tune.py), copied as literals: name -> default; train_dir / valid_dir are required
REFERENCE_TRAIN = dict(output_dir="/tmp/pcv2-ft", model_name=None, task_type="classification", num_labels=None, train_batch_size=43,
                       eval_batch_size=3, eval_num_samples=0, max_steps=500, seed=42, use_wandb=False, learning_rate=1e-3, warmup_steps=50,
                       lr_scheduler_type="linear", gradient_accumulation_steps=64, bf16=True, num_train_epochs=3, weight_decay=0.01,
                       eval_strategy="steps", eval_steps=25, save_strategy="steps", save_steps=100, logging_steps=100,
                       resume_from_checkpoint=None)


def test_train_parser_has_the_references_flags_and_defaults():
    parse = lambda *extra: lora_predict.build_parser().parse_args(["train", "--train_dir", "t", "--valid_dir", "v", *extra])
    a = vars(parse())
    assert a["train_dir"] == "t" and a["valid_dir"] == "v"
    for k, v in REFERENCE_TRAIN.items():
        assert k in a, k
        if k == "bf16":                     # the stated departure: float32 is the default here, as for predict / evaluate
            assert a[k] is False
        else:
            assert a[k] == v and type(a[k]) is type(v), (k, a[k], v)
    extra = dict(device="cuda:0", pooling="mean", train_lora=1, max_grad_norm=1.0, lora_dropout=0.0)
    assert {k: a[k] for k in extra} == extra
    assert set(a) == set(REFERENCE_TRAIN) | set(extra) | {"cmd", "train_dir", "valid_dir"}
    assert lora_predict.SAVE_TOTAL_LIMIT == 5
    b = vars(parse("--bf16", "true", "--train-batch-size", "4", "--train_lora", "0", "--use_wandb", "False"))
    assert b["bf16"] is True and b["train_batch_size"] == 4 and b["train_lora"] == 0 and b["use_wandb"] is False
    with pytest.raises(SystemExit):
        lora_predict.build_parser().parse_args(["train", "--valid_dir", "v"])
    for flags, word in ((["--lora_dropout", "0.1"], "lora_dropout"), (["--pooling", "max"], "pooling"), (["--use_wandb", "true"], "use_wandb")):
        with pytest.raises(SystemExit, match=word):
            lora_predict.main(["train", "--train_dir", "t", "--valid_dir", "v", "--model_name", "m", *flags])
