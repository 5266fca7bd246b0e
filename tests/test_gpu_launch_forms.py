"""-m gpu: every small-launch form of the layer walk against the oracle, at its boundaries.

A pcad_forward call picks its layer walk from the windows of the call (tests/launch_forms.py): the segmented scan, the pair walk
(both directions in one launch, half a strand each, twice; never the last layer), the K-split of the fused conv + x_proj kernel,
or the plain walk.  These forms serve every call of a few windows (ISM, notebooks, PlantCAD2's 8 192-bp batches, the tail batch of a
table), so each case below first asserts - through the workspace the library carves - that it runs the form its id names, then
checks every entry point against the oracle (nl = 2, stress weights, masked centre position):
  1. logits and the last hidden state: fp32 1e-4 of max, arg-max exact at the masked position; bf16 3e-2 of max against the
     bf16-emulating oracle in the engine's order (tied out_proj applied once to y_fwd + y_rev: tie_fold; "reference_order" 1 keeps
     that fold);
  2. a positions list (last-layer shortcut): bit-identical to slicing the full output;
  3. per-window positions (pcad_forward_at): bit-identical to the full output at each window's position;
  4. materialize_all_hidden_states: every level against the oracle at the same bars; fp32 logits bit-identical to the run
     without it;
  5. the pooled head (mean, max) against the head restatement on the oracle's hidden state;
  6. "poison_workspace": bit-identical, finite;
  7. "chunk_seqs" 1: bit-identical to the default chunking (fp32; bf16 when L % 128 == 0: include/pcad.h "chunk_seqs").
The oracle runs once per (case, dtype) and is shared by the option sets."""
import time

import pytest
import torch

from launch_forms import engaged_forms
from oracle import caduceus_oracle as O
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.engine import load_library
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM, CaduceusForSequenceClassification
from seqcls_ref import head_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NL = 2

# id: (D, L, B, G, pair, ks fp32, ks bf16)
CASES = {
    "pair-tiny":                (64, 128, 1, 1, True, 2, 1),
    "pair-odd-halves":          (64, 192, 3, 1, True, 2, 1),
    "pair-upper-bound":         (64, 128, 896, 1, True, 1, 1),        # exactly 3 584 waves
    "pair-padded-fold":         (384, 512, 22, 1, True, 1, 1),        # 528 waves; bf16 fold padded to 512 columns
    "pair-l32-width":           (1024, 512, 9, 1, True, 1, 1),        # 576 waves
    "seg4-at-bound-ks4":        (1024, 512, 8, 4, False, 4, 4),       # exactly 512 waves, 64 row tiles
    "seg10-partial-block-ks":   (128, 300, 2, 10, False, 4, 2),
    "seg4x2-at-512-waves":      (128, 256, 64, 4, False, 1, 1),
    "seg8-ks-not-pow2":         (192, 256, 3, 8, False, 6, 3),
    "seg4x17-long-strand":      (64, 2080, 1, 4, False, 2, 1),        # last segment shorter, partial 32-step block
    "ksplit-only":              (128, 127, 3, 1, False, 4, 2),
}
MODES = {  # id: (dtype, engine options)
    "fp32": (torch.float32, {}),
    "fp32-split": (torch.float32, {"f32_gemm_split": 1}),
    "bf16": (torch.bfloat16, {}),
    "bf16-reforder1": (torch.bfloat16, {"reference_order": 1}),
}
_ORACLE = {}


def case_setup(name):
    D, L, B = CASES[name][:3]
    cfg = make_config("x", d_model=D, n_layer=NL)
    sd = synthetic_state_dict(cfg, seed=D + L + B, stress=True)
    g = torch.Generator().manual_seed(L + B)
    ids = torch.randint(3, 7, (B, L), generator=g)
    ids[:, L // 2] = 1                                                        # [MASK] at the centre
    return cfg, sd, ids


def rcps(x, B):
    """strand-major [2B, L, D] -> the RCPS layout [B, L, 2D]"""
    return torch.cat([x[:B], torch.flip(x[B:], dims=[1, 2])], dim=-1)


def oracle(name, bf16):
    """-> dict(logits, hidden, levels): levels = the n_layer + 1 hidden states of output_hidden_states."""
    key = (name, bf16)
    if key not in _ORACLE:
        cfg, sd, ids = case_setup(name)
        t = time.time()
        if bf16:
            cap = {}
            r = O.forward_strands(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16, tie_fold=True,
                                  capture=cap)
            P = O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16)
            B = ids.shape[0]
            emb = O.round_bf16(P.emb[O.strands(ids, P.complement)])
            levels = [rcps(emb, B)] + [rcps(m, B) for m in cap["mix"][:-1]] + [r["hidden"]]
        else:
            r = O.forward_literal(ids, O.params_from_state_dict(sd, cfg), output_hidden_states=True)
            levels = r["all_hidden"]
        _ORACLE[key] = dict(logits=r["logits"], hidden=r["hidden"].float(), levels=[x.float() for x in levels])
        print(f"oracle {name} {'bf16' if bf16 else 'fp32'}: {time.time() - t:.1f} s")
    return _ORACLE[key]


def mlm(cfg, sd, dtype, opts, all_hidden=False):
    cfg.engine_options = dict(opts)
    cfg.materialize_all_hidden_states = all_hidden
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(sd, strict=False)
    m.tie_weights()
    return m.to(dtype).to(DEV).eval()


def seqcls(cfg, sd, dtype, opts, pooling):
    cfg.engine_options = dict(opts)
    cfg.num_labels = 3
    m = CaduceusForSequenceClassification(cfg, pooling_strategy=pooling)
    m.load_state_dict({k: v for k, v in sd.items() if k.startswith("caduceus.")}, strict=False)
    with torch.no_grad():
        m.score.weight.copy_(torch.randn(3, cfg.d_model, generator=torch.Generator().manual_seed(5)) * 0.05)
    return m.to(dtype).to(DEV).eval()


def rel(a, b):
    return ((a.float() - b.float()).abs().max() / b.float().abs().max()).item()


@pytest.mark.parametrize("mode", list(MODES))
@pytest.mark.parametrize("name", list(CASES))
def test_launch_form_vs_oracle(name, mode):
    t0 = time.time()
    D, L, B, G, pair, ks32, ks16 = CASES[name]
    dtype, opts = MODES[mode]
    bf16 = dtype == torch.bfloat16
    cfg, sd, ids = case_setup(name)
    # the form this case is named for, before anything is compared
    f = engaged_forms(load_library(), cfg, B, L, dtype, **opts)
    assert (f["G"], f["pair"], f["ks"]) == (G, pair, ks16 if bf16 else ks32), (name, mode, f)
    ref = oracle(name, bf16)
    bar = 3e-2 if bf16 else 1e-4
    c = L // 2
    dev_ids = ids.to(DEV)

    m = mlm(cfg, sd, dtype, opts)
    out = m(input_ids=dev_ids, output_hidden_states=True)
    lg, hid = out.logits.float().cpu(), out.hidden_states[-1].float().cpu()
    assert torch.isfinite(lg).all() and torch.isfinite(hid).all()
    # 1. against the oracle
    e_l, e_h = rel(lg, ref["logits"]), rel(hid, ref["hidden"])
    assert e_l <= bar and e_h <= bar, (name, mode, e_l, e_h)
    if not bf16:
        assert torch.equal(lg[:, c, 3:7].argmax(-1), ref["logits"][:, c, 3:7].argmax(-1))
    # 2. a positions list (the last layer's shortened walks)
    pos = sorted({c, 0, L - 1, max(0, c - 1)})
    o2 = m(input_ids=dev_ids, output_hidden_states=True, positions=pos)
    assert torch.equal(o2.logits.float().cpu(), lg[:, pos]) and torch.equal(o2.hidden_states[-1].float().cpu(), hid[:, pos])
    # 3. one position per window (pcad_forward_at)
    per = torch.tensor([(c + 37 * b) % L for b in range(B)])
    o3 = m(input_ids=dev_ids, output_hidden_states=True, positions=per.to(DEV))
    rows = torch.arange(B)
    assert torch.equal(o3.logits.float().cpu()[:, 0], lg[rows, per]) and torch.equal(o3.hidden_states[-1].float().cpu()[:, 0],
                                                                                      hid[rows, per])
    # 6. poisoned workspace
    eng = m._engine()
    eng.set_option("poison_workspace", 1)
    o6 = m(input_ids=dev_ids, output_hidden_states=True)
    eng.set_option("poison_workspace", 0)
    assert torch.equal(o6.logits.float().cpu(), lg) and torch.equal(o6.hidden_states[-1].float().cpu(), hid)
    # 7. one window per chunk: the forms are those of the call (include/pcad.h "chunk_seqs")
    if B > 1 and (not bf16 or L % 128 == 0):
        eng.set_option("chunk_seqs", 1)
        o7 = m(input_ids=dev_ids, output_hidden_states=True)
        eng.set_option("chunk_seqs", 0)
        assert torch.equal(o7.logits.float().cpu(), lg), (name, mode, rel(o7.logits.cpu(), lg))
        assert torch.equal(o7.hidden_states[-1].float().cpu(), hid)
    del m, eng
    # 4. every hidden level (pcad_forward_all_hidden)
    ma = mlm(cfg, sd, dtype, opts, all_hidden=True)
    o4 = ma(input_ids=dev_ids, output_hidden_states=True)
    assert len(o4.hidden_states) == NL + 1
    for i, (got, want) in enumerate(zip(o4.hidden_states, ref["levels"])):
        e = rel(got.cpu(), want)
        assert e <= bar, (name, mode, "level", i, e)
    if not bf16:
        assert torch.equal(o4.logits.cpu(), lg)
    del ma
    # 5. the pooled head on the same forward
    for pooling in ("mean", "max"):
        sc = seqcls(cfg, sd, dtype, opts, pooling)
        got = sc(input_ids=dev_ids).logits.float().cpu()
        want, _ = head_ref(ref["hidden"].to(dtype) if bf16 else ref["hidden"], sc.score.weight.detach().float(), pooling, dtype)
        e = rel(got, want)
        assert e <= bar, (name, mode, pooling, e)
        del sc
    print(f"{name} {mode}: forms G={f['G']} pair={f['pair']} ks={f['ks']}; logits {e_l:.1e} hidden {e_h:.1e}; "
          f"{time.time() - t0:.1f} s")


@pytest.mark.parametrize("dtype,opts", [(torch.float32, {}), (torch.bfloat16, {}), (torch.bfloat16, {"gate_each": 1})],
                         ids=["fp32", "bf16", "bf16-gate-each"])
def test_window_result_across_batch_sizes(dtype, opts):
    """The batch-size contract of include/pcad.h "scan_segments" at the l32 width (D 1024, 2 layers, L 512): window 0 scored
    inside batches of 1 (segmented, K-split), 8 (segmented at the bound, ks 4), 9 and 56 (pair), 57 (plain).  fp32: within 5e-6
    of max across all of them, bit-identical where the forms are the same (9 vs 56); bf16: within 2e-2; bf16 "gate_each" 1: the
    pair and plain walks add the same two rounded addends - bit-identical (9, 56 vs 57)."""
    cfg = make_config("x", d_model=1024, n_layer=2)
    sd = synthetic_state_dict(cfg, seed=17, stress=True)
    ids = torch.randint(3, 7, (57, 512), generator=torch.Generator().manual_seed(3))
    ids[:, 255] = 1
    lib = load_library()
    forms = {B: engaged_forms(lib, cfg, B, 512, dtype, **opts) for B in (1, 8, 9, 56, 57)}
    assert forms[1]["G"] > 1 and forms[1]["ks"] > 1
    assert (forms[8]["G"], forms[8]["ks"]) == (4, 4)
    assert forms[9]["pair"] and forms[56]["pair"] and forms[9]["ks"] == forms[56]["ks"] == 1
    assert (forms[57]["G"], forms[57]["pair"], forms[57]["ks"]) == (1, False, 1)
    m = mlm(cfg, sd, dtype, opts)
    got = {}
    for B in forms:
        o = m(input_ids=ids[:B].to(DEV), output_hidden_states=True)
        got[B] = (o.logits[0].float().cpu(), o.hidden_states[-1][0].float().cpu())
    lg0, h0 = got[57]
    assert torch.isfinite(lg0).all()
    bf16 = dtype == torch.bfloat16
    for B, (lg, h) in got.items():
        e_l, e_h = rel(lg, lg0), rel(h, h0)
        print(f"{dtype} {opts} B={B}: logits {e_l:.1e} hidden {e_h:.1e} vs B=57")
        assert max(e_l, e_h) <= (2e-2 if bf16 else 5e-6), (B, e_l, e_h)
    if not bf16:
        assert torch.equal(got[9][0], got[56][0]) and torch.equal(got[9][1], got[56][1])
    if opts.get("gate_each"):
        for B in (9, 56):
            assert torch.equal(got[B][0], lg0) and torch.equal(got[B][1], h0), B
