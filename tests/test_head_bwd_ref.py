"""CPU checks behind tests/test_gpu_head_bwd.py and tests/test_gpu_training_model.py: the restatement of tests/head_bwd_ref.py is the
head the oracle computes and its autograd gradients are the derivatives (central finite differences in float64); the whole-model graph
of tests/model_bwd_ref.py is the oracle's forward; pcad_loss_head_bwd sizes its scratch and refuses bad arguments before any device
work; and TrainableCaduceusForMaskedLM has the reference's parameter names, ties and trainable parameters."""
import os
import re

import pytest
import torch
import torch.nn.functional as F

import head_bwd_ref as HB
import model_bwd_ref as MB
import scan_bwd_ref as SB
from oracle import caduceus_oracle as O
from plantcaduceus_amd import engine, ops
from plantcaduceus_amd.checkpoint import EMB_KEY, LMHEAD_KEY, layer_keys, make_config, synthetic_state_dict

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
INV, WSP = -1, -3                      # include/pcad.h PCAD_ERR_INVALID, PCAD_ERR_WORKSPACE


def toy_config(n_layer=2):
    return make_config("toy", d_model=64, n_layer=n_layer,
                       ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def test_head_restatement_is_the_oracles_head():
    """logits against forward_strands' head lines (rms_norm_fn + Hf @ emb.T + Hr_al @ emb[comp].T), nll against F.cross_entropy"""
    c = HB.inputs(11, 3, 37, 48, labels="mixed", weights=True)
    B, L, D = c["B"], c["L"], 48
    H = O.rms_norm_fn(c["h"].view(2 * B, L, D), c["norm_weight"], residual=c["res"].view(2 * B, L, D), eps=c["eps"], prenorm=False,
                      residual_in_fp32=True)
    Hf, Hr_al = H[:B], torch.flip(H[B:], dims=[1])
    comp = torch.tensor(HB.COMP, dtype=torch.long)
    ref = Hf @ c["emb"].t() + Hr_al @ c["emb"][comp].t()
    lab = c["labels"].long()
    ce_lab = torch.where(HB.labelled_mask(lab), lab, torch.full_like(lab, -100))      # a label of 9 contributes nothing
    for dtype in (torch.float64, torch.float32):
        lg = HB.head_logits(c["h"], c["res"], c["norm_weight"], c["emb"], B, L, c["eps"], dtype)
        m = SB.metric(lg, ref)
        want = F.cross_entropy(lg.reshape(-1, 8), ce_lab.view(-1), reduction="none", ignore_index=-100).view(B, L)
        n = SB.metric(HB.token_nll(lg, c["labels"]), want)
        print(f"head restatement {dtype}: logits {m:.3e}, nll {n:.3e}")
        assert m < 1e-6 and n < 1e-6
    assert (HB.token_nll(lg, c["labels"])[~HB.labelled_mask(c["labels"])] == 0).all()
    assert not HB.labelled_mask(c["labels"])[1].any() and (c["labels"] == 9).sum() == 1 and (c["labels"] == -1).any()


def test_label_sets_have_the_properties_the_gpu_tests_rely_on():
    g = torch.Generator().manual_seed(5)
    for B, L in ((1, 1), (3, 63), (1, 64), (3, 65), (3, 2 * HB.SEG + 5)):
        lab = HB.make_labels(g, B, L, "some")
        m = HB.labelled_mask(lab)
        assert m.any(1).all(), (B, L)                                    # every window has a labelled position
        if L > HB.SEG:
            assert not m[0, HB.SEG:2 * HB.SEG].any() and 0 < m.float().mean() < 0.4, (B, L)      # ... and one segment has none
        assert HB.labelled_mask(HB.make_labels(g, B, L, "all")).all()


@pytest.mark.parametrize("dnll", [False, True])
def test_head_restatement_gradients_are_the_derivatives(dnll):
    """central differences of the scalar in float64 over every coordinate of h, res, norm_weight and emb, step 1e-6, held to 1e-6 of
    each gradient's maximum (as tests/test_block_bwd_ref.py)"""
    c = HB.inputs(3, 2, 5, 8, labels="all", weights=True, dnll=dnll)
    c["labels"][0, 1], c["labels"][1, 3] = -100, 9
    g = HB.grads(c)

    def loss(d):
        lg = HB.head_logits(d["h"], d["res"], d["norm_weight"], d["emb"], d["B"], d["L"], d["eps"])
        up = d["dsum"].double()[:, None] * d["loss_weights"].double() + (d["dnll"].double() if d["dnll"] is not None else 0.0)
        return (up * HB.token_nll(lg, d["labels"])).sum().item()
    eps = 1e-6
    for name in HB.NAMES:
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
        print(f"finite differences {name}: {err:.3e}")
        assert err < 1e-6, name
    assert torch.equal(g["h"], g["res"])
    rows = g["h"].view(2 * c["B"], c["L"], -1)
    assert (rows[0, 1] == 0).all() and (rows[2 + 0, c["L"] - 1 - 1] == 0).all() and (rows[1, 3] == 0).all()      # unlabelled positions


def test_vjp_from_given_logits_is_the_gradient_when_the_logits_are_the_graphs_own():
    c = HB.inputs(4, 2, 9, 16, labels="mixed", weights=True, dnll=True)
    lg = HB.head_logits(c["h"], c["res"], c["norm_weight"], c["emb"], c["B"], c["L"], c["eps"])
    a, b = HB.grads(c), HB.grads(c, kernel_logits=lg)
    for k in HB.NAMES:
        assert SB.metric(b[k], a[k]) < 1e-12, k


def test_loss_seg_matches_the_kernels():
    src = open(os.path.join(ROOT, "plantcaduceus_amd", "csrc", "kernels.hpp")).read()
    assert int(re.search(r"constexpr int LOSS_SEG = (\d+);", src).group(1)) == ops.LOSS_SEG == HB.SEG


def scratch_formula(B, L, D):
    """one row of 9 D fp32 partials per (window, segment of LOSS_SEG positions) and one spare row, rounded up to 256 bytes"""
    return ((B * ((L + ops.LOSS_SEG - 1) // ops.LOSS_SEG) + 1) * 9 * D * 4 + 255) // 256 * 256


def test_scratch_bytes(lib):
    f, G = lib.pcad_loss_head_bwd_scratch_bytes, ops.LOSS_SEG
    prev = None
    for args in ((1, 1, 8), (2, 1, 8), (2, G, 8), (2, G + 1, 8), (2, G + 1, 384), (3, 2 * G + 5, 384), (3, 2 * G + 5, 2048), (256, 512, 1024),
                 (4096, 2048, 2048)):
        n = f(*args)
        assert n > 0 and n % 256 == 0 and (prev is None or n >= prev), args
        assert n == scratch_formula(*args), args
        prev = n
    assert f(4096, 2048, 2048) > 2 ** 32
    assert f(256, 512, 1024) == 75534336                              # the figure DESIGN.md §4n states
    assert f(2, G + 1, 384) > f(2, G, 384) and f(3, G, 384) > f(2, G, 384) and f(2, G, 768) > f(2, G, 384)
    assert f(0, 5, 384) == 0 and f(2, 0, 384) == 0 and f(2, 5, 0) == 0


def test_entry_refuses_bad_arguments_without_a_device(lib):
    """pointers are never dereferenced on the host: any non-null 16-byte-aligned value stands for a tensor"""
    p = 0x10000
    last = engine.load_library().pcad_last_error

    def call(h=p, res=p, w=p, emb=p, comp=p, labels=p, lw=p, dsum=p, dnll=p, dh=p, dres=p, dw=p, demb=p, scratch=p, nbytes=1 << 40, B=2, L=70,
             D=384, dtype=0, rdt=0):
        return lib.pcad_loss_head_bwd(h, res, w, emb, comp, labels, lw, -100, dsum, dnll, dh, dres, dw, demb, scratch, nbytes, B, L, D, 1e-5, dtype,
                                      rdt, None)
    for name, word in (("h", b"h"), ("res", b"res"), ("w", b"norm_weight"), ("emb", b"emb_f32"), ("comp", b"complement"), ("labels", b"labels"),
                       ("dsum", b"dsum")):
        assert call(**{name: None}) == INV and b"null " + word in last(), name
    assert call(dh=None, dres=None, dw=None, demb=None) == INV and b"no output" in last()
    assert call(D=388) == INV and b"D" in last()
    assert call(D=2056) == INV and b"D" in last() and b"2048" in last()
    assert call(dtype=7) == INV and b"dtype" in last()
    assert call(rdt=7) == INV and b"res_dtype" in last()
    assert call(dtype=0, rdt=1) == INV and b"res_dtype" in last()    # an fp32 model keeps an fp32 residual stream
    assert call(h=p + 8) == INV and b"h must be" in last()
    assert call(dres=p + 4) == INV and b"dres" in last()
    assert call(B=-1) == INV
    assert call(scratch=p + 16) == WSP and call(scratch=None) == WSP and call(nbytes=1024) == WSP
    assert b"scratch" in last()
    assert call(nbytes=scratch_formula(2, 70, 384) - 1) == WSP
    # nothing to do: OK before the scratch is looked at
    assert call(B=0, scratch=None, nbytes=0) == 0 and call(L=0, scratch=None, nbytes=0) == 0


def test_trainable_model_structure():
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    cfg = toy_config()
    sd = synthetic_state_dict(cfg)
    model = TrainableCaduceusForMaskedLM(cfg, dtype=torch.float32, device="cpu")
    own = model.state_dict()
    assert set(own) == set(sd)
    assert all(tuple(own[k].shape) == tuple(sd[k].shape) for k in sd)
    assert all(p.requires_grad for p in model.parameters())
    named = dict(model.named_parameters(remove_duplicate=False))
    assert named[LMHEAD_KEY] is named[EMB_KEY]
    for i in range(cfg.n_layer):
        f, r = layer_keys(i, "fwd"), layer_keys(i, "rev")
        assert named[r["in_proj"]] is named[f["in_proj"]] and named[r["out_proj"]] is named[f["out_proj"]]
        assert named[r["conv_w"]] is not named[f["conv_w"]]
    model.load_state_dict(sd)
    assert all(torch.equal(model.state_dict()[k], sd[k]) for k in sd)
    assert own[LMHEAD_KEY].data_ptr() == own[EMB_KEY].data_ptr()
    # one gradient per tied pair: the optimizer's view has each tensor once
    assert len(list(model.parameters())) == len(sd) - 1 - 2 * cfg.n_layer
    with pytest.raises(RuntimeError, match="ROCm"):
        model(torch.zeros(1, 8, dtype=torch.long), torch.zeros(1, 8, dtype=torch.long))
    with pytest.raises(NotImplementedError):
        TrainableCaduceusForMaskedLM(make_config("toy", d_model=64, n_layer=1, bidirectional_weight_tie=False,
                                                 ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True)), device="cpu")


def test_model_restatement_is_the_oracles_forward():
    """the whole-model graph in fp32 against forward_strands(..., tie_fold=False): logits < 1e-6 at the toy geometry of the GPU test"""
    cfg = toy_config()
    sd = synthetic_state_dict(cfg)
    B, L = 2, ops.CONV_BWD_SEG + 5
    g = torch.Generator().manual_seed(3)
    ids = torch.randint(0, 8, (B, L), generator=g)
    labels = HB.make_labels(g, B, L, "some")
    ref = O.forward_strands(ids, O.params_from_state_dict(sd, cfg), tie_fold=False)["logits"]
    with torch.no_grad():
        out = MB.forward(MB.leaves(sd, cfg, torch.float32), cfg, ids, labels, dtype=torch.float32)
    m = SB.metric(out["logits"], ref)
    print(f"model restatement fp32 against forward_strands: {m:.3e}")
    assert m < 1e-6
    assert SB.metric(out["nll"], HB.token_nll(ref.double(), labels)) < 1e-5
