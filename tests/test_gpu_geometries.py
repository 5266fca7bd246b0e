"""-m gpu: every model geometry pcad_create accepts, through pcad_forward* against the oracle.

The other model-level tests build their models with make_config("x", d_model=D): expand 2, dt_rank ceil(D / 16), residual_in_fp32,
D <= 1536.  pcad_create takes more (include/pcad.h pcad_config), and CaduceusConfig forwards ssm_cfg.expand, ssm_cfg.dt_rank and
residual_in_fp32 straight into it, so a snapshot with such values loads and runs.  Four regions of that space:
  1. dt_rank > 96 (Rp 128 .. 256; d_model 2048 reaches it with dt_rank "auto"): no fused conv + x_proj kernel - conv.hip with blocked
     input and output, x_proj as a GEMM on a blocked operand, the scan's run-time-layout (bf16) or Rp-generic (fp32) instantiation;
     the segmented scan, the last-layer shortcut, the norm fold, "reference_order" and "f32_gemm_split" still apply to that walk;
  2. dt_rank 65 .. 96 with L % 8 != 0 in bf16: the fused kernel at Rp 96, then the scan's run-time-layout instantiation;
  3. expand != 2 (E = D, 3D, 4D): the in_proj split point, the fold's tile conditions, the K-tile count of the fused kernel, the
     waves per strand, every scratch size;
  4. residual_in_fp32 = False on the bf16 model: a bf16 residual stream through every norm and head kernel, never folded.
Each case is the smallest shape at which its path can still go wrong (nl = 2, stress weights, [MASK] at L // 2, one [UNK]).  A case
first names the walk it runs - the launch forms through the workspace the library carves (tests/launch_forms.py), the x_proj GEMM and
the folded out_proj through the engine's profile counters - and then checks, at the bars of tests/test_gpu_launch_forms.py (fp32
1e-4 of the reference's max with the arg-max exact at the masked position: forward_literal; bf16 3e-2 of max, finite: the
bf16-emulating forward_strands in the engine's order; d_model 2048: the C oracle):
  1. logits and the last hidden state of the full forward;
  2. the positions list [c, 0, L - 1, c - 1] (last-layer shortcut): bit-identical to slicing 1;
  3. one position per window (pcad_forward_at): bit-identical to 1;
  4. materialize_all_hidden_states: every level at the same bar; fp32 logits bit-identical to 1;
  5. "poison_workspace" 1: bit-identical;
  6. "chunk_seqs" 1 with B > 1: bit-identical (fp32; bf16 when L % 128 == 0).
The oracle runs once per (case, dtype, order) and is shared by the option sets."""
import math
import time

import pytest
import torch

import mlm_ref
from launch_forms import engaged_forms, padded_dt_rank
from oracle import caduceus_oracle as O
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.engine import load_library
from seqcls_ref import head_ref
from test_gpu_launch_forms import mlm, rcps, rel, seqcls
from test_gpu_layers import averaged, gather, window_positions
from test_gpu_mlm_loss import rand_labels, rand_weights
from test_gpu_probs import COLS, positions_for

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NL = 2
DTYPES = {"fp32": torch.float32, "bf16": torch.bfloat16}
BAR = {"fp32": 1e-4, "bf16": 3e-2}

# id: (D, expand, dt_rank (None: "auto"), residual_in_fp32, B, L, {dtype: (G, pair, ks)}, bf16 default form folds the norm)
CASES = {
    "rp128-ragged":     (128, 2, 100, True, 3, 45, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, False),   # R % 32 != 0 (zero-padded K), L % 8 != 0
    "rp128-tiles":      (256, 2, 128, True, 2, 128, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, True),   # whole 256-row tiles: the fold wraps the walk
    "rp160":            (128, 2, 129, True, 2, 64, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, True),    # the first Rp past 128
    "rp256":            (64, 2, 256, True, 2, 40, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, False),    # the largest dt_rank; E = 128
    "rp128-seg":        (128, 2, 100, True, 2, 300, {"fp32": (10, False, 1), "bf16": (10, False, 1)}, False),    # partial last 32-step block
    "rp128-seg-long":   (64, 2, 100, True, 1, 2080, {"fp32": (4, False, 1)}, False),                         # long-strand segmentation
    "rp96-ragged":      (128, 2, 80, True, 3, 77, {"bf16": (1, False, 2), "fp32": (1, False, 4)}, False),    # region 2
    "expand1-one-wave": (64, 1, None, True, 3, 64, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, False),   # E = 64: one wave per strand, one K-tile (bf16)
    "expand1-fold":     (256, 1, None, True, 2, 128, {"fp32": (1, True, 4), "bf16": (1, True, 2)}, True),    # E = D
    "expand3":          (128, 3, None, True, 2, 96, {"fp32": (1, False, 6), "bf16": (1, False, 3)}, False),  # E = 384: no power of two
    "expand3-fold":     (256, 3, None, True, 2, 128, {"bf16": (1, True, 6)}, True),                          # E = 768 with the fold
    "expand4-pair":     (64, 4, None, True, 3, 128, {"fp32": (1, True, 4), "bf16": (1, True, 2)}, True),     # E = 256: the pair walk
    "res-bf16":         (128, 2, None, False, 3, 45, {"bf16": (1, False, 2)}, False),                        # region 4, ragged
    "res-bf16-tiles":   (256, 2, None, False, 2, 128, {"bf16": (1, True, 4)}, False),                        # would fold if it could
}
D2048 = (2048, 2, None, True, 2, 64, {"fp32": (1, False, 1), "bf16": (1, False, 1)}, True)     # dt_rank "auto" = 128; K = 4096 sums
# id: (dtype, engine options) on top of each case's plain dtypes
OPTION_SETS = {
    "fp32-split":     ("fp32", {"f32_gemm_split": 1}),
    "bf16-reforder1": ("bf16", {"reference_order": 1}),
    "bf16-reforder2": ("bf16", {"reference_order": 2}),       # against the oracle in the reference's own order (tie_fold=False)
    "bf16-gate-each": ("bf16", {"gate_each": 1}),
    "fp32-noseg":     ("fp32", {"scan_segments": 0}),
    "bf16-noseg":     ("bf16", {"scan_segments": 0}),
}
CASE_OPTIONS = {
    "rp128-ragged": ["fp32-split", "bf16-reforder1", "bf16-reforder2", "bf16-gate-each"],
    "rp128-tiles":  ["fp32-split", "bf16-reforder1", "bf16-reforder2", "bf16-gate-each"],
    "rp128-seg":    ["fp32-split", "fp32-noseg", "bf16-noseg"],
    "expand4-pair": ["fp32-noseg", "bf16-noseg"],
}
# "scan_segments" 0 against the default walk: (fp32, bf16) bars of test_segmented_scan_equals_single_walk / test_pair_walk_equals_plain_walk
SWITCH_BAR = {"rp128-seg": {"fp32": 2e-5, "bf16": 2e-2}, "expand4-pair": {"fp32": 5e-6, "bf16": 2e-2}}
RUNS = [(name, key) for name, c in CASES.items() for key in c[6]] + [(name, mode) for name, modes in CASE_OPTIONS.items() for mode in modes]
EXTRA = [(name, key) for name in ("rp128-ragged", "rp128-tiles", "expand3", "res-bf16") for key in CASES[name][6]]
_ORACLE, _WEIGHTS = {}, {}


def mode_of(mode):
    """-> (dtype key, engine options)"""
    return OPTION_SETS[mode] if mode in OPTION_SETS else (mode, {})


def case_setup(case):
    """-> (a fresh config, state dict, ids [B, L]) of a row of CASES"""
    D, expand, R, res32, B, L = case[:6]
    cfg = make_config("x", d_model=D, n_layer=NL, residual_in_fp32=res32,
                      ssm_cfg=dict(d_state=16, d_conv=4, expand=expand, dt_rank="auto" if R is None else R, bias=False, conv_bias=True))
    assert (cfg.d_inner, cfg.dt_rank, bool(cfg.residual_in_fp32)) == (expand * D, R or math.ceil(D / 16), res32)
    if case[:6] not in _WEIGHTS:                                                  # built once, read only
        ids = torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(L + B))
        ids[:, L // 2] = 1                                                        # [MASK] at the centre
        ids[0, 0] = 2                                                             # one [UNK]
        _WEIGHTS[case[:6]] = (synthetic_state_dict(cfg, seed=D + expand + cfg.dt_rank + L, stress=True), ids)
    sd, ids = _WEIGHTS[case[:6]]
    return cfg, sd, ids


def oracle(name, key, strict=False):
    """-> dict(logits, hidden, levels): levels = the n_layer + 1 hidden states of output_hidden_states.  strict (bf16): the
    reference's own order, each direction through its own tied out_proj ("reference_order" 2)."""
    k = (name, key, strict)
    if k not in _ORACLE:
        cfg, sd, ids = case_setup(CASES[name])
        t = time.time()
        if key == "bf16":
            cap = {}
            P = O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16)
            r = O.forward_strands(ids, P, rnd=O.round_bf16, tie_fold=not strict, capture=cap)
            B = ids.shape[0]
            emb = O.round_bf16(P.emb[O.strands(ids, P.complement)])
            levels = [rcps(emb, B)] + [rcps(m, B) for m in cap["mix"][:-1]] + [r["hidden"]]
        else:
            r = O.forward_literal(ids, O.params_from_state_dict(sd, cfg), output_hidden_states=True)
            levels = r["all_hidden"]
        _ORACLE[k] = dict(logits=r["logits"], hidden=r["hidden"].float(), levels=[x.float() for x in levels])
        print(f"oracle {name} {key}{' strict' if strict else ''}: {time.time() - t:.1f} s")
    return _ORACLE[k]


def counters(eng):
    torch.cuda.synchronize()
    st = {k: v[0] for k, v in eng.profile_read().items()}
    eng.profile(False)
    return st


def named_walk(case, key, opts, st):
    """The path a case runs, stated before anything is compared: the launch forms its table row names, the x_proj GEMM launches of
    the unfused walk (two per layer) or none of them, and the folded out_proj of every layer but the last, or none."""
    cfg, _, _ = case_setup(case)
    B, L, forms, folds = case[4], case[5], case[6], case[7]
    f = engaged_forms(load_library(), cfg, B, L, DTYPES[key], **opts)
    want = (1, False, 1) if opts.get("scan_segments") == 0 else forms[key]
    assert (f["G"], f["pair"], f["ks"]) == want, (f, want)
    fused = padded_dt_rank(cfg.dt_rank) <= 96
    assert st["gemm_x_proj"] == (0 if fused else 2 * NL) and st["conv1d_bidir"] == NL, st
    fold = key == "bf16" and folds and "reference_order" not in opts
    assert st["gemm_out_proj_res"] == (NL - 1 if fold else 0), st
    # the full-size tied out_proj: twice per layer in the strict reference order, once per layer otherwise (folded: the last layer's only)
    assert st["gemm_out_proj"] == (2 * NL if opts.get("reference_order") == 2 else 1 if fold else NL), st
    return f, fold


def run_checks(case, key, opts, ref, tag, model=None, checks=(1, 2, 3, 4, 5, 6)):
    """Checks 1 - 6 of the module docstring on one (case, dtype, option set).  -> (logits, hidden) of check 1 on the CPU."""
    t0 = time.time()
    cfg, sd, ids = case_setup(case)
    B, L = ids.shape
    dtype, bar, bf16 = DTYPES[key], BAR[key], key == "bf16"
    c = L // 2
    dev_ids = ids.to(DEV)
    m = model if model is not None else mlm(cfg, sd, dtype, opts)
    eng = m._engine()
    eng.profile(1)
    out = m(input_ids=dev_ids, output_hidden_states=True)
    f, fold = named_walk(case, key, opts, counters(eng))
    lg, hid = out.logits.float().cpu(), out.hidden_states[-1].float().cpu()
    assert out.hidden_states[-1].dtype == dtype and lg.shape == (B, L, 8) and hid.shape == (B, L, 2 * cfg.d_model)
    assert torch.isfinite(lg).all() and torch.isfinite(hid).all()
    # 1. against the oracle
    e_l, e_h = rel(lg, ref["logits"]), rel(hid, ref["hidden"])
    print(f"{tag}: forms G={f['G']} pair={f['pair']} ks={f['ks']} fold={fold}; logits {e_l:.2e} hidden {e_h:.2e} (bar {bar:.0e})")
    assert e_l <= bar and e_h <= bar, (tag, e_l, e_h)
    if not bf16:
        assert torch.equal(lg[:, c, 3:7].argmax(-1), ref["logits"][:, c, 3:7].argmax(-1)), tag
    # 2. a positions list (the last layer's shortened walks)
    pos = [c, 0, L - 1, c - 1]
    o2 = m(input_ids=dev_ids, output_hidden_states=True, positions=pos)
    assert torch.equal(o2.logits.float().cpu(), lg[:, pos]) and torch.equal(o2.hidden_states[-1].float().cpu(), hid[:, pos]), tag
    # 3. one position per window (pcad_forward_at)
    if 3 in checks:
        per = torch.tensor([(c + 37 * b) % L for b in range(B)])
        o3 = m(input_ids=dev_ids, output_hidden_states=True, positions=per.to(DEV))
        rows = torch.arange(B)
        assert torch.equal(o3.logits.float().cpu()[:, 0], lg[rows, per]), tag
        assert torch.equal(o3.hidden_states[-1].float().cpu()[:, 0], hid[rows, per]), tag
    # 5. poisoned workspace
    eng.set_option("poison_workspace", 1)
    o5 = m(input_ids=dev_ids, output_hidden_states=True)
    eng.set_option("poison_workspace", 0)
    assert torch.equal(o5.logits.float().cpu(), lg) and torch.equal(o5.hidden_states[-1].float().cpu(), hid), tag
    # 6. one window per chunk: the forms are those of the call (include/pcad.h "chunk_seqs")
    if 6 in checks and B > 1 and (not bf16 or L % 128 == 0):
        eng.set_option("chunk_seqs", 1)
        o6 = m(input_ids=dev_ids, output_hidden_states=True)
        eng.set_option("chunk_seqs", 0)
        assert torch.equal(o6.logits.float().cpu(), lg), (tag, rel(o6.logits.cpu(), lg))
        assert torch.equal(o6.hidden_states[-1].float().cpu(), hid), tag
    m.check_status()
    del m, eng
    # 4. every hidden level (pcad_forward_all_hidden)
    if 4 in checks:
        ma = mlm(cfg, sd, dtype, opts, all_hidden=True)
        o4 = ma(input_ids=dev_ids, output_hidden_states=True)
        assert len(o4.hidden_states) == NL + 1
        errs = [rel(got.cpu(), want) for got, want in zip(o4.hidden_states, ref["levels"])]
        print(f"{tag}: levels " + " ".join(f"{e:.2e}" for e in errs) + f"; {time.time() - t0:.1f} s")
        assert max(errs) <= bar, (tag, errs)
        assert rel(o4.logits.cpu(), ref["logits"]) <= bar, tag
        if not bf16:
            assert torch.equal(o4.logits.cpu(), lg), tag
        del ma
    return lg, hid


@pytest.mark.parametrize("name,mode", RUNS, ids=[f"{n}-{m}" for n, m in RUNS])
def test_geometry_vs_oracle(name, mode):
    key, opts = mode_of(mode)
    case = CASES[name]
    ref = oracle(name, key, strict=opts.get("reference_order") == 2)
    lg, hid = run_checks(case, key, opts, ref, f"{name} {mode}")
    cfg, sd, ids = case_setup(case)
    if opts.get("scan_segments") == 0:
        # the same function as the default walk (segmented scan / pair walk + K-split), which the plain run of this case checked
        d = mlm(cfg, sd, DTYPES[key], {})(input_ids=ids.to(DEV), output_hidden_states=True)
        e_l, e_h = rel(lg, d.logits.float().cpu()), rel(hid, d.hidden_states[-1].float().cpu())
        print(f"{name} {mode}: against the default walk: logits {e_l:.2e} hidden {e_h:.2e} (bar {SWITCH_BAR[name][key]:.0e})")
        assert max(e_l, e_h) <= SWITCH_BAR[name][key], (name, mode, e_l, e_h)
    if name == "res-bf16-tiles":
        # a bf16 residual stream is never folded: "norm_fold" 0 changes nothing, bit for bit
        o = mlm(cfg, sd, DTYPES[key], {"norm_fold": 0})(input_ids=ids.to(DEV), output_hidden_states=True)
        assert torch.equal(o.logits.float().cpu(), lg) and torch.equal(o.hidden_states[-1].float().cpu(), hid)


@pytest.fixture(scope="module", params=["fp32", "bf16"])
def d2048(request):
    """d_model 2048 (about 50 M parameters in two layers): the model and the C oracle's result, built once per dtype"""
    from oracle.c_oracle import COracle
    key = request.param
    cfg, sd, ids = case_setup(D2048)
    assert cfg.dt_rank == 128
    t = time.time()
    kw = dict(dtype=torch.bfloat16, emulate_bf16=True) if key == "bf16" else {}
    lg_ref, hid_ref = COracle(sd, cfg, blas=True, **kw).forward(ids.numpy(), want_hidden=True)
    model = mlm(cfg, sd, DTYPES[key], {})
    print(f"d2048 {key}: oracle and model in {time.time() - t:.1f} s")
    return key, model, dict(logits=torch.from_numpy(lg_ref), hidden=torch.from_numpy(hid_ref))


def test_d2048_vs_c_oracle(d2048):
    """The one natural configuration on the unfused walk: checks 1, 2 and 5 (the full last layer, the last-layer shortcut, the
    poisoned workspace) against the C oracle (fp32; bf16: its bf16-emulating mode in the engine's order)."""
    key, model, ref = d2048
    run_checks(D2048, key, {}, ref, f"d2048 {key}", model=model, checks=(1, 2, 5))


@pytest.mark.parametrize("name,key", EXTRA, ids=[f"{n}-{k}" for n, k in EXTRA])
def test_entry_points_vs_restatements(name, key):
    """The other entry points on four of the geometries, each against the restatement it already has, fed the oracle's outputs:
    the pooled head (mean, max; seqcls_ref.head_ref on the oracle's hidden state, the logit bar); pcad_forward_loss (mlm_ref on the
    oracle's logits; |d nll| <= 2 max |d logit|: twice the logit bar, as tests/test_gpu_mlm_loss.py derives it, and the per-window
    sums with it); pcad_forward_probs with a list of positions per window (float64 softmax of the oracle's logits; |dp| <= max
    |d logit|: the logit bar as an absolute number, never above 1, as tests/test_gpu_probs.py); pcad_forward_layers at the middle
    level, assembled and averaged, shared and per-window positions (the oracle's level, the hidden-state bar)."""
    case = CASES[name]
    cfg, sd, ids = case_setup(case)
    B, L = ids.shape
    dtype, bar, bf16 = DTYPES[key], BAR[key], key == "bf16"
    ref = oracle(name, key)
    dev_ids = ids.to(DEV)
    g = torch.Generator().manual_seed(L)
    for pooling in ("mean", "max"):
        sc = seqcls(case_setup(case)[0], sd, dtype, {}, pooling)
        got = sc(input_ids=dev_ids).logits.float().cpu()
        want, _ = head_ref(ref["hidden"].to(dtype) if bf16 else ref["hidden"], sc.score.weight.detach().float(), pooling, dtype)
        e = rel(got, want)
        print(f"{name} {key}: pooled head ({pooling}) {e:.2e} (bar {bar:.0e})")
        assert e <= bar, (name, key, pooling, e)
        sc.check_status()
        del sc
    m = mlm(cfg, sd, dtype, {})
    scale = ref["logits"].abs().max().item()
    # the loss head
    labels = rand_labels(B, L, 0.3, g)
    labels[:, L // 2] = ids[:, (L // 2) - 1].to(torch.int32)                   # the masked position is always labelled
    for weights in (None, rand_weights(B, L, g)):
        out = m(input_ids=dev_ids, labels=labels.to(DEV), loss_weights=None if weights is None else weights.to(DEV),
                return_token_nll=True, return_window_sums=True)
        lbar = 2 * bar * scale
        e_tok = (out["token_nll"].cpu().double() - mlm_ref.token_nll(ref["logits"], labels)).abs().max().item()
        e_loss = abs(out.loss.item() - mlm_ref.loss(ref["logits"], labels, weights).item())
        sums, want = out["window_sums"].cpu().double(), mlm_ref.window_sums(ref["logits"], labels, weights)
        e_sum = ((sums[:, 0] - want[:, 0]).abs() / want[:, 1].clamp_min(1e-30)).max().item()     # per unit of weight
        print(f"{name} {key} weights={weights is not None}: |d nll| {e_tok:.2e} |d loss| {e_loss:.2e} |d sum| / weight {e_sum:.2e} (bar {lbar:.2e})")
        assert e_tok <= lbar and e_loss <= lbar and e_sum <= lbar, (name, key)
        torch.testing.assert_close(sums[:, 1], want[:, 1], rtol=1e-5, atol=0)
        assert torch.equal(sums[:, 2:], mlm_ref.window_sums(out.logits.cpu(), labels, weights)[:, 2:])
        assert torch.equal(out.logits.cpu(), m(input_ids=dev_ids).logits.cpu())
    # the probability head, every window its own positions (0 and L - 1 among them)
    own = torch.stack([torch.tensor(positions_for(L, 5, g)) for _ in range(B)])
    p_all = m.nucleotide_probs(dev_ids, COLS).cpu()
    p_own = m.nucleotide_probs(dev_ids, COLS, positions_per_window=own.to(DEV)).cpu()
    idx = own.long()[:, :, None].expand(-1, -1, 4)
    assert torch.equal(p_own, torch.gather(p_all, 1, idx))
    want_p = torch.softmax(ref["logits"][..., list(COLS)].double(), dim=-1)
    pbar = min(bar * scale, 1.0)
    e_p = max((p_all.double() - want_p).abs().max().item(), (p_own.double() - torch.gather(want_p, 1, idx)).abs().max().item())
    print(f"{name} {key}: |dp| {e_p:.2e} (bar {pbar:.2e})")
    assert e_p <= pbar, (name, key, e_p)
    # the middle level of hidden_states at the evaluated positions
    mid = NL // 2
    want_l = ref["levels"][mid]
    hs = want_l.abs().max()
    pos, ownw = [L // 2, 0, L - 1, 5, 5], window_positions(B, L)
    for kind, idx2, kw in (("shared", torch.tensor([pos] * B), dict(positions=pos)),
                           ("per-window", ownw, dict(positions_per_window=ownw.to(DEV)))):
        rows = m.hidden_states_at(dev_ids, layers=[mid], **kw)
        avg = m.hidden_states_at(dev_ids, layers=[mid], average=True, **kw)
        assert rows.dtype == dtype and rows.shape == (1, B, idx2.shape[1], 2 * cfg.d_model) and avg.dtype == torch.float32
        want_rows = gather(want_l, idx2)
        e_r = ((rows[0].float().cpu() - want_rows).abs().max() / hs).item()
        e_a = ((avg[0].cpu() - averaged(want_rows)).abs().max() / hs).item()
        print(f"{name} {key}: level {mid} {kind}: rows {e_r:.2e} averaged {e_a:.2e} (bar {bar:.0e})")
        assert e_r <= bar and e_a <= bar, (name, key, kind, e_r, e_a)
        assert torch.equal(avg[0].cpu(), averaged(rows[0].cpu()))                      # the reference's arithmetic on the engine's own rows
    m.check_status()
