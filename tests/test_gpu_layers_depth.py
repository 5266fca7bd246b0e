"""pcad_forward_layers below the top level on the MI355X: the walk stops after block K - 1 for the highest requested
level K < n_layer, block K - 1 is shortened like the last layer of pcad_forward, and the token ids are checked by a kernel of their
own - while every returned byte stays what pcad_forward_all_hidden's rows are.

Shapes: 4 layers (one more than tests/test_gpu_layers.py, so that "below the top" has room), d_model 128 and 192, L 64 and 96, B 1,
3 and 9 ("chunk_seqs" 4: three uneven chunks), bf16 and fp32; L 128 where the pair walks engage; L 25 for chunk starts that are
not 16-byte aligned."""
import numpy as np
import pytest
import torch

from oracle import caduceus_oracle as O
from plantcaduceus_amd import embeddings, engine
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
from untied_ref import untied_state_dict

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NL = 4
DTYPES = [torch.bfloat16, torch.float32]
LAYER_SETS = ([0], [1], [2], [3], [1, 3], [0, 2], [2, 4], None)


def mlm(D, dtype, seed=11, **options):
    cfg = make_config("tiny", d_model=D, n_layer=NL)
    cfg.engine_options = dict(options)
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed), strict=False)
    m.tie_weights()
    return m.to(dtype).to(DEV).eval()


def rand_ids(B, L, seed):
    return torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(seed))


def gather(x, idx):
    """x [..., B, L, W], idx [B, P] -> [..., B, P, W]"""
    ix = idx[:, :, None].expand(*x.shape[:-3], -1, -1, x.shape[-1])
    return torch.gather(x, -2, ix)


def averaged(x):
    D = x.shape[-1] // 2
    return (x[..., :D].float() + x[..., D:].float().flip(-1)) / 2


def full_tuple(eng, ids):
    """the whole hidden_states tuple through pcad_forward_all_hidden, [n_layer + 1, B, L, 2D] on the CPU"""
    _, last, allh = eng.forward(ids, want_hidden=True, want_logits=False, all_hidden=True)
    return torch.cat([allh, last[None]], dim=0).cpu()


def window_positions(B, L):
    return torch.tensor([[(5 + 11 * b) % L, (L - 1) if b % 2 else 0] for b in range(B)], dtype=torch.int64)


def counts(eng):
    st = eng.profile_read()
    return st["selective_scan"][0], st["gemm_in_proj"][0]


def check_levels(eng, ids, full, layers, tag, average=(False, True), **kw):
    """every level of forward_layers(layers, **kw) against the rows of `full`, plain and averaged, bit for bit"""
    B, L = ids.shape
    lv = list(range(NL + 1)) if layers is None else layers
    if "positions" in kw:
        idx = torch.tensor([list(kw["positions"])] * B)
    else:
        idx = kw["positions_per_window"].cpu().long()
    want = gather(full[lv], idx)
    for avg in average:
        got = eng.forward_layers(ids, layers, average=avg, **kw).cpu()
        ref = averaged(want) if avg else want
        assert got.shape == ref.shape and got.dtype == ref.dtype, (tag, layers, avg)
        for i, k in enumerate(lv):
            assert torch.equal(got[i], ref[i]), (tag, layers, "level", k, "average" if avg else "plain", sorted(kw))


# ---- 1. launch counts -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_launch_counts_follow_the_highest_level(dtype):
    """K blocks for the highest requested level K: 2 K scan launches and K in_proj launches per chunk (the parent commit ran all four
    blocks: 8 and 4); K = n_layer and layers=None as before."""
    D, L = 128, 64
    m = mlm(D, dtype, scan_segments=0)
    eng = m._engine()
    for B, chunk, nchunks in ((3, 0, 1), (9, 4, 3)):
        eng.set_option("chunk_seqs", chunk)
        ids = rand_ids(B, L, 40 + B).to(DEV)
        eng.profile(1)
        eng.profile_read()
        for layers, K in (([0], 0), ([1], 1), ([2], 2), ([3], 3), ([4], 4), (None, 4), ([0, 2], 2), ([1, 3], 3)):
            m.hidden_states_at(ids, layers=layers, positions=[L // 2])
            assert counts(eng) == (2 * K * nchunks, K * nchunks), (B, layers)
        # per-window lists truncate the walk too (the block below the level stays whole)
        m.hidden_states_at(ids, layers=[1], positions_per_window=window_positions(B, L).to(DEV))
        assert counts(eng) == (2 * nchunks, nchunks), B
        eng.profile(False)
    m.check_status()


# ---- 2. bytes -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [64, 96])
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 192])
def test_levels_equal_all_hidden(D, dtype, L):
    """Every level of every request is bit-equal to indexing and flipping pcad_forward_all_hidden's output in torch on the CPU.
    [L // 2] gives walk_len < L on the shortened block; [0] and [L - 1] force the whole walk."""
    m = mlm(D, dtype)
    eng = m._engine()
    for B in (1, 3, 9):
        eng.set_option("chunk_seqs", 4 if B == 9 else 0)
        ids = rand_ids(B, L, 100 * L + B).to(DEV)
        full = full_tuple(eng, ids)
        assert full.shape == (NL + 1, B, L, 2 * D)
        own = window_positions(B, L).to(DEV)
        for layers in LAYER_SETS:
            for pos in ([L // 2], [0], [L - 1], [3, L // 2, L - 2]):
                check_levels(eng, ids, full, layers, (D, dtype, L, B), positions=pos)
            check_levels(eng, ids, full, layers, (D, dtype, L, B), positions_per_window=own)
    m.check_status()


# ---- 3. forms -------------------------------------------------------------------------------------------------------------------
FORMS = [("reference_order_2", torch.bfloat16, 3, dict(reference_order=2)), ("reference_order_2", torch.float32, 3, dict(reference_order=2)),
         ("split", torch.float32, 3, dict(f32_gemm_split=1)), ("split_strict", torch.float32, 3, dict(f32_gemm_split=1, reference_order=2)),
         ("segmented", torch.bfloat16, 1, dict(scan_segments=1)), ("segmented", torch.float32, 1, dict(scan_segments=1)),
         ("B72", torch.bfloat16, 72, {}), ("B72", torch.float32, 72, {})]


@pytest.mark.parametrize("name,dtype,B,options", FORMS, ids=[f"{n}-{str(d)[6:]}" for n, d, _, _ in FORMS])
def test_forms_of_the_shortened_block(name, dtype, B, options):
    """layers=[2] at [L // 2] under every form that can reach the shortened block: the strict order's own shortcut branch, the split
    GEMMs (the scan must not write out_proj's operand on that block), the segmented scan (which ignores walk_len), 576 scan waves per
    direction (B 72)."""
    D, L = 128, (256 if name == "segmented" else 64)          # the scan is cut into segments from L 256 on
    m = mlm(D, dtype, **options)
    eng = m._engine()
    ids = rand_ids(B, L, 7).to(DEV)
    full = full_tuple(eng, ids)
    for layers in ([2], [1, 3]):
        check_levels(eng, ids, full, layers, name, positions=[L // 2])
        check_levels(eng, ids, full, layers, name, positions=[3, L // 2])
    m.check_status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_untied_directions(dtype):
    cfg = make_config("x", d_model=128, n_layer=NL)
    cfg.engine_options = dict(untied_directions=1)
    sd = untied_state_dict(cfg, seed=31)
    eng = engine.Engine(cfg, {k: v for k, v in sd.items() if k.startswith("caduceus.")}, dtype, torch.device(DEV))
    B, L = 3, 64
    ids = rand_ids(B, L, 8).to(DEV)
    full = full_tuple(eng, ids)
    for layers in ([2], [1, 3], [0]):
        check_levels(eng, ids, full, layers, "untied", positions=[L // 2])
    eng.check_status()


@pytest.mark.parametrize("dtype,options", [(torch.bfloat16, {}), (torch.float32, {}), (torch.float32, dict(f32_gemm_split=1))],
                         ids=["bfloat16", "float32", "float32-split"])
def test_pair_walk_range_keeps_the_bytes(dtype, options):
    """L 128, B 3: 24 scan waves per direction, so blocks 0 .. 2 of pcad_forward_all_hidden run as pair walks, which round the
    gate-once sum elsewhere than plain walks do.  A truncated call runs that same form on its last block (it stays whole there): the
    bytes are pcad_forward_all_hidden's, and the walk still stops at the highest level."""
    D, L, B = 128, 128, 3
    m = mlm(D, dtype, **options)
    eng = m._engine()
    ids = rand_ids(B, L, 12).to(DEV)
    full = full_tuple(eng, ids)
    for layers in ([1], [2], [1, 3], [0, 2]):
        check_levels(eng, ids, full, layers, "pair", positions=[L // 2])
    eng.profile(1)
    eng.profile_read()
    m.hidden_states_at(ids, layers=[2], positions=[L // 2])
    assert counts(eng) == (4, 2)
    eng.profile(False)
    m.check_status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_shortcut_off_same_bytes_same_depth(dtype):
    """"last_layer_shortcut" 0: block K - 1 runs whole, the walk still stops after it, the bytes are the same."""
    D, L, B = 128, 64, 3
    m = mlm(D, dtype, scan_segments=0)
    eng = m._engine()
    ids = rand_ids(B, L, 9).to(DEV)
    full = full_tuple(eng, ids)
    on = m.hidden_states_at(ids, layers=[2], positions=[L // 2]).cpu()
    eng.set_option("last_layer_shortcut", 0)
    eng.profile(1)
    eng.profile_read()
    off = m.hidden_states_at(ids, layers=[2], positions=[L // 2]).cpu()
    assert counts(eng) == (4, 2)
    eng.profile(False)
    assert torch.equal(on, off) and torch.equal(off[0], full[2][:, [L // 2]])
    m.check_status()


# ---- 4. independence ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_window_rows_do_not_depend_on_the_call(dtype):
    """"scan_segments" 0: window 0's rows are bit-identical alone, in a batch of 9, under "chunk_seqs" 4 and with every workspace byte
    0xFF before the call (the compact rows, the gathered operand and the split operand are written before they are read)."""
    D, L, B = 192, 96, 9
    m = mlm(D, dtype, scan_segments=0)
    eng = m._engine()
    ids = rand_ids(B, L, 5).to(DEV)

    def run(x):
        return [m.hidden_states_at(x, layers=lay, positions=pos, average=avg).cpu()[:, :1]
                for lay in ([2], [1, 3], [0]) for pos in ([L // 2], [3, L - 2]) for avg in (False, True)]

    base = run(ids[:1])
    for opts in (dict(), dict(chunk_seqs=4), dict(chunk_seqs=4, poison_workspace=1), dict(chunk_seqs=0, poison_workspace=1)):
        for k, v in opts.items():
            eng.set_option(k, v)
        for a, b in zip(run(ids), base):
            assert torch.isfinite(a.float()).all(), opts
            assert torch.equal(a, b), opts
    m.check_status()


# ---- 5. status ------------------------------------------------------------------------------------------------------------------
def expect_bad_token(m, ids, clean, **kw):
    m.hidden_states_at(ids, **kw)
    assert m.status_bits() == engine.STATUS_BAD_TOKEN, kw
    with pytest.raises(IndexError):
        m.check_status()
    m.hidden_states_at(clean, **kw)
    assert m.status_bits() == 0, kw


@pytest.mark.parametrize("L", [64, 25])
def test_bad_token_is_reported_without_the_head(L):
    """A token id of 99 in window 2 of 9 under "chunk_seqs" 4 with layers=[1] - no head runs - is PCAD_STATUS_BAD_TOKEN, and the next
    clean call leaves the word at 0.  L 25 under "chunk_seqs" 1 and 3: chunks start 100 b / 300 b bytes into the ids, so every
    alignment of a chunk's first id occurs, and the ids behind the last whole 16-byte piece are checked too - each id of windows 1, 2
    and 3 in turn, as 99 and as -1."""
    D, B = 128, 9
    m = mlm(D, torch.float32)
    eng = m._engine()
    clean = rand_ids(B, L, 3).to(DEV)
    eng.set_option("chunk_seqs", 4)
    bad = clean.clone()
    bad[2, 7] = 99
    expect_bad_token(m, bad, clean, layers=[1], positions=[3])
    expect_bad_token(m, bad, clean, layers=[0], positions=[3])                  # no block at all
    expect_bad_token(m, bad, clean, layers=[1], positions_per_window=window_positions(B, L).to(DEV))
    if L == 25:
        for chunk in (1, 3):
            eng.set_option("chunk_seqs", chunk)
            for w in (1, 2, 3):
                for t in range(L):
                    bad = clean.clone()
                    bad[w, t] = 99 if t % 2 else -1
                    m.hidden_states_at(bad, layers=[1], positions=[3])
                    assert m.status_bits() == engine.STATUS_BAD_TOKEN, (chunk, w, t)
                    with pytest.raises(IndexError):
                        m.check_status()
            m.hidden_states_at(clean, layers=[1], positions=[3])
            assert m.status_bits() == 0, chunk


def test_bad_position_is_clamped_and_reported():
    D, L, B = 128, 64, 3
    m = mlm(D, torch.float32)
    ids = rand_ids(B, L, 9).to(DEV)
    good = window_positions(B, L)
    bad = good.clone()
    bad[1, 1] = L + 3                       # window 1's slot that holds L - 1
    bad[2, 1] = -2                          # window 2's slot that holds 0
    want = m.hidden_states_at(ids, layers=[1], positions_per_window=good.to(DEV)).cpu()
    m.check_status()
    got = m.hidden_states_at(ids, layers=[1], positions_per_window=bad.to(DEV)).cpu()
    assert m.status_bits() == engine.STATUS_BAD_POSITION
    with pytest.raises(IndexError, match="position"):
        m.check_status()
    assert torch.equal(got, want)


# ---- 6. the oracle --------------------------------------------------------------------------------------------------------------
def test_level_against_the_oracle_fp32():
    """layers=[2] at [L // 2] against the literal-RCPS torch oracle's hidden_states[2]: tests/test_gpu_model.py's 1e-4 of the level's
    largest value."""
    D, L, B = 128, 64, 3
    cfg = make_config("tiny", d_model=D, n_layer=NL)
    sd = synthetic_state_dict(cfg, seed=11)
    m = mlm(D, torch.float32)
    ids = rand_ids(B, L, 21)
    want = O.forward_literal(ids, O.params_from_state_dict(sd, cfg), output_hidden_states=True)["all_hidden"][2]
    got = m.hidden_states_at(ids.to(DEV), layers=[2], positions=[L // 2]).cpu()
    err = ((got[0, :, 0] - want[:, L // 2]).abs().max() / want.abs().max()).item()
    print(f"fp32 level 2 at {L // 2}: {err:.3e} of max |h| {want.abs().max().item():.3f}")
    assert err < 1e-4
    m.check_status()


def test_level_against_the_oracle_bf16():
    """The same against the oracle that rounds to bf16 where the reference's bf16 model stores a tensor: tests/test_gpu_model.py's bf16
    bar, 3e-2 of the range."""
    D, L, B = 128, 64, 3
    cfg = make_config("tiny", d_model=D, n_layer=NL)
    sd = synthetic_state_dict(cfg, seed=11)
    m = mlm(D, torch.bfloat16)
    ids = rand_ids(B, L, 21)
    want = O.forward_literal(ids, O.params_from_state_dict(sd, cfg, dtype=torch.bfloat16), rnd=O.round_bf16,
                             output_hidden_states=True)["all_hidden"][2].float()
    got = m.hidden_states_at(ids.to(DEV), layers=[2], positions=[L // 2]).float().cpu()
    err = ((got[0, :, 0] - want[:, L // 2]).abs().max() / want.abs().max()).item()
    print(f"bf16 level 2 at {L // 2}: {err:.3e} of max |h| {want.abs().max().item():.3f}")
    assert err < 3e-2
    m.check_status()


# ---- 7. python ------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_extract_embeddings_layer_1_runs_one_block(dtype):
    m = mlm(128, dtype)
    eng = m._engine()
    tok = CaduceusTokenizer()
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGTN"), size=64, p=[.24, .24, .24, .24, .04])) for _ in range(5)]
    ids = torch.from_numpy(tok.encode_batch(seqs, mask_index=None)).long().to(DEV)
    want = averaged(full_tuple(eng, ids)[1][:, 31])
    eng.profile(1)
    eng.profile_read()
    got = embeddings.extract_embeddings(m, seqs, DEV, 31, tok, layer=1)
    scans, in_projs = counts(eng)
    eng.profile(False)
    assert got.dtype == np.float32 and got.shape == (5, 128)
    assert torch.equal(torch.from_numpy(got), want)
    assert (scans, in_projs) == (2, 1)
