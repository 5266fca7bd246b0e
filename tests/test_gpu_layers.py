"""Per-layer hidden states at the evaluated positions on the MI355X (csrc/layers.hip): the row kernel as an operator
(pcad_layer_rows against indexing and flipping in torch on the CPU), and pcad_forward_layers / hidden_states_at against
pcad_forward_all_hidden, pcad_forward, pcad_forward_at and the live torch oracle, on synthetic checkpoints.

Shapes: d_model 128 and 192 (D / 8 even and odd), n_layer 3, L 64 and 96 (96: no pair walk), B 1, 3 and 9 (9 under "chunk_seqs" 4:
three uneven chunks), bf16 and fp32; a shared list with unsorted and repeated entries, and per-window lists whose rows differ and
include 0 and L - 1."""
import numpy as np
import pytest
import torch

from oracle import caduceus_oracle as O
from plantcaduceus_amd import embeddings, engine, ops
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
NL = 3
DTYPES = [torch.bfloat16, torch.float32]


def mlm(D, dtype, n_layer=NL, seed=11, **options):
    cfg = make_config("tiny", d_model=D, n_layer=n_layer)
    cfg.engine_options = dict(options)
    m = CaduceusForMaskedLM(cfg)
    m.load_state_dict(synthetic_state_dict(cfg, seed=seed), strict=False)
    m.tie_weights()
    return m.to(dtype).to(DEV).eval()


def rand_ids(B, L, seed):
    return torch.randint(3, 7, (B, L), generator=torch.Generator().manual_seed(seed))


def shared_positions(L):
    return [0, L - 1, 5, 5, L // 2]                      # unsorted, one repeated


def window_positions(B, L):
    """[B, 3]: every window its own list, 0 and L - 1 in changing slots"""
    rows = []
    for b in range(B):
        r = [0, L - 1, (5 + 11 * b) % L]
        rows.append(r[b % 3:] + r[:b % 3])
    return torch.tensor(rows, dtype=torch.int64)


def gather(x, idx):
    """x [..., B, L, W], idx [B, P] -> [..., B, P, W]"""
    ix = idx[:, :, None].expand(*x.shape[:-3], -1, -1, x.shape[-1])
    return torch.gather(x, -2, ix)


def averaged(x):
    """the reference's strand averaging of rows in hidden_states' layout (src/train_XGBoost.py:106-113), on the CPU"""
    D = x.shape[-1] // 2
    return (x[..., :D].float() + x[..., D:].float().flip(-1)) / 2


def full_tuple(eng, ids):
    """the whole hidden_states tuple through pcad_forward_all_hidden, [n_layer + 1, B, L, 2D] on the CPU"""
    _, last, allh = eng.forward(ids, want_hidden=True, want_logits=False, all_hidden=True)
    return torch.cat([allh, last[None]], dim=0).cpu()


# ---- the row kernel alone ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_layer_rows_operator(dtype):
    """Random h: the plain form is bit-equal to indexing the two strands' rows and flipping the reverse-complement one's channels;
    the averaged form to (x[..., :D].float() + x[..., D:].float().flip(-1)) / 2 of that row; the assembled input form to its input
    (plain) and to the same average.  D 64 (most lanes idle), 128, 192 (24 / 48 pieces: a partly filled wave), 1032 (more than one
    piece per lane in bf16: 129 pieces), more than one block."""
    g = torch.Generator().manual_seed(7)
    for D, L, B in ((64, 7, 1), (128, 64, 3), (192, 96, 9), (1032, 5, 2)):
        h = torch.randn(2 * B * L, D, generator=g).to(dtype)
        hd = h.to(DEV)
        hv = h.view(2, B, L, D)
        want_full = torch.cat([hv[0], hv[1].flip(1, 2)], dim=-1)                       # [B, L, 2D]: row (b, p) = [fwd | rc reversed]
        pos = shared_positions(L) if L > 5 else [0, L - 1, 2, 2]
        own = window_positions(B, L)
        for kind, idx, kw in (("shared", torch.tensor([pos] * B), dict(positions=pos)),
                              ("per-window", own, dict(positions_per_window=own.to(DEV)))):
            want = gather(want_full, idx)
            plain = ops.layer_rows(hd, B, L, **kw)
            assert plain.dtype == dtype and plain.shape == (B, idx.shape[1], 2 * D)
            assert torch.equal(plain.cpu(), want), (D, L, B, kind)
            avg = ops.layer_rows(hd, B, L, average=True, **kw)
            assert avg.dtype == torch.float32 and avg.shape == (B, idx.shape[1], D)
            assert torch.equal(avg.cpu(), averaged(want)), (D, L, B, kind, "average")
            # the last level's form: rows that are already assembled
            assert torch.equal(ops.layer_rows(plain, B, L, assembled=True, **kw).cpu(), want), (D, L, B, kind, "assembled")
            assert torch.equal(ops.layer_rows(plain, B, L, assembled=True, average=True, **kw).cpu(), averaged(want)), (D, L, B, kind)
    # a per-window position outside the window: clamped and reported, the other windows untouched
    B, L, D = 3, 64, 128
    hd = torch.randn(2 * B * L, D, generator=g).to(dtype).to(DEV)
    good = window_positions(B, L)
    bad = good.clone()
    bad[1, good[1].tolist().index(L - 1)] = L + 3        # the slots of window 1 / 2 that hold L - 1 / 0
    bad[2, good[2].tolist().index(0)] = -2
    status = torch.zeros(1, dtype=torch.int32, device=DEV)
    ref = ops.layer_rows(hd, B, L, positions_per_window=good.to(DEV), status=status)
    assert int(status.item()) == 0
    got = ops.layer_rows(hd, B, L, positions_per_window=bad.to(DEV), status=status)
    assert int(status.item()) == engine.STATUS_BAD_POSITION
    assert torch.equal(got, ref)
    with pytest.raises(RuntimeError, match="out of range"):
        ops.layer_rows(hd, B, L, positions=[1, L])


# ---- levels against pcad_forward_all_hidden ------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
@pytest.mark.parametrize("D", [128, 192])
def test_levels_equal_all_hidden(D, dtype):
    """All levels, and layers=[0, 2]: every level is bit-equal to the rows of pcad_forward_all_hidden's output (hidden_out for the
    last level) on the same batch under the same options, in both position forms; the averaged form is the reference's arithmetic
    on those rows, bit for bit."""
    m = mlm(D, dtype)
    eng = m._engine()
    for L in (64, 96):
        for B in (1, 3, 9):
            eng.set_option("chunk_seqs", 4 if B == 9 else 0)
            ids = rand_ids(B, L, 100 * L + B).to(DEV)
            full = full_tuple(eng, ids)
            assert full.shape == (NL + 1, B, L, 2 * D)
            pos, own = shared_positions(L), window_positions(B, L)
            for layers in (None, [0, 2]):
                lv = list(range(NL + 1)) if layers is None else layers
                for kind, idx, kw in (("shared", torch.tensor([pos] * B), dict(positions=pos)),
                                      ("per-window", own, dict(positions_per_window=own.to(DEV)))):
                    want = gather(full[lv], idx)
                    got = m.hidden_states_at(ids, layers=layers, **kw)
                    assert got.dtype == dtype and got.shape == (len(lv), B, idx.shape[1], 2 * D)
                    for i, k in enumerate(lv):
                        assert torch.equal(got[i].cpu(), want[i]), (D, dtype, L, B, kind, "level", k)
                    avg = m.hidden_states_at(ids, layers=layers, average=True, **kw)
                    assert avg.dtype == torch.float32 and avg.shape == (len(lv), B, idx.shape[1], D)
                    assert torch.equal(avg.cpu(), averaged(want)), (D, dtype, L, B, kind, "average")
    m.check_status()


# ---- the last level alone: pcad_forward's / pcad_forward_at's walk -------------------------------------------------------------
@pytest.mark.parametrize("dtype,D,L,B", [(torch.bfloat16, 256, 128, 2),          # 512 token-rows, D % 256 == 0: the norm fold engages
                                         (torch.bfloat16, 128, 64, 3), (torch.bfloat16, 192, 96, 9),
                                         (torch.float32, 128, 96, 3), (torch.float32, 192, 64, 9)])
def test_last_level_only_equals_forward(dtype, D, L, B):
    m = mlm(D, dtype)
    eng = m._engine()
    if B == 9:
        eng.set_option("chunk_seqs", 4)
    ids = rand_ids(B, L, 3).to(DEV)
    pos, own = shared_positions(L), window_positions(B, L)
    # shared list: pcad_forward(positions=...)'s hidden_out (norm fold and last-layer shortcut as that call chooses them)
    want = eng.forward(ids, positions=pos, want_hidden=True, want_logits=False)[1]
    got = m.hidden_states_at(ids, layers=[NL], positions=pos)
    assert got.shape == (1, B, len(pos), 2 * D) and torch.equal(got[0], want)
    assert torch.equal(m.hidden_states_at(ids, layers=[NL], positions=pos, average=True)[0].cpu(), averaged(want.cpu()))
    # one position per window: pcad_forward_at's hidden_out
    one = own[:, :1].contiguous().to(DEV)
    want_at = eng.forward(ids, positions=one[:, 0], want_hidden=True, want_logits=False)[1]
    assert torch.equal(m.hidden_states_at(ids, layers=[NL], positions_per_window=one)[0], want_at)
    # three per window: the full last layer, whose rows pcad_forward (all positions) writes
    whole = eng.forward(ids, want_hidden=True, want_logits=False)[1].cpu()
    got3 = m.hidden_states_at(ids, layers=[NL], positions_per_window=own.to(DEV))
    assert torch.equal(got3[0].cpu(), gather(whole, own))
    assert torch.equal(m.hidden_states_at(ids, layers=[NL], positions_per_window=own.to(DEV), average=True)[0].cpu(),
                       averaged(gather(whole, own)))
    if dtype == torch.bfloat16 and D == 256:
        # the fold really engaged in this call's walk: the unfolded walk (any level below the last) rounds elsewhere
        unfolded = m.hidden_states_at(ids, layers=[0, NL], positions=pos)[1]
        assert not torch.equal(unfolded, got[0])
    m.check_status()


# ---- the oracle ----------------------------------------------------------------------------------------------------------------
def test_levels_against_the_oracle():
    """fp32, d_model 128, 3 layers: every level at the evaluated positions against the literal-RCPS torch oracle's hidden_states
    tuple, with tests/test_gpu_model.py's bar for pcad_forward_all_hidden against that oracle: 1e-4 of the level's largest value."""
    D, L, B = 128, 64, 3
    cfg = make_config("tiny", d_model=D, n_layer=NL)
    sd = synthetic_state_dict(cfg, seed=11)
    m = mlm(D, torch.float32)
    ids = rand_ids(B, L, 21)
    ref = O.forward_literal(ids, O.params_from_state_dict(sd, cfg), output_hidden_states=True)["all_hidden"]
    assert len(ref) == NL + 1
    pos, own = shared_positions(L), window_positions(B, L)
    got_s = m.hidden_states_at(ids.to(DEV), positions=pos).cpu()
    got_w = m.hidden_states_at(ids.to(DEV), positions_per_window=own.to(DEV)).cpu()
    avg = m.hidden_states_at(ids.to(DEV), positions=pos, average=True).cpu()
    for k, want in enumerate(ref):
        scale = want.abs().max()
        errs = (((got_s[k] - want[:, pos]).abs().max() / scale).item(), ((got_w[k] - gather(want, own)).abs().max() / scale).item(),
                ((avg[k] - averaged(want[:, pos])).abs().max() / scale).item())
        print(f"level {k}: shared {errs[0]:.3e} per-window {errs[1]:.3e} averaged {errs[2]:.3e} of max |h| {scale.item():.3f}")
        assert max(errs) < 1e-4, (k, errs)
    m.check_status()


# ---- chunking, the workspace, the batch ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_chunk_and_poison_independence(dtype):
    """"chunk_seqs" 1, 4 and the default are bit-identical (B = 9: nine chunks, three uneven ones, one), and "poison_workspace" 1 - every
    workspace byte 0xFF before the call - leaves no NaN and the same bits: the last level's assembled rows and the column copy of the
    per-window list are written before they are read."""
    D, L, B = 192, 96, 9
    m = mlm(D, dtype)
    eng = m._engine()
    ids = rand_ids(B, L, 5).to(DEV)
    pos, own = shared_positions(L), window_positions(B, L).to(DEV)

    def run():
        return [m.hidden_states_at(ids, positions=pos).cpu(), m.hidden_states_at(ids, positions_per_window=own).cpu(),
                m.hidden_states_at(ids, layers=[1, 2], positions_per_window=own, average=True).cpu(),
                m.hidden_states_at(ids, layers=[NL], positions=pos).cpu(), m.hidden_states_at(ids, layers=[NL], positions_per_window=own).cpu()]

    base = run()
    for opts in (dict(chunk_seqs=1), dict(chunk_seqs=4), dict(chunk_seqs=4, poison_workspace=1), dict(chunk_seqs=0, poison_workspace=1)):
        for k, v in opts.items():
            eng.set_option(k, v)
        for a, b in zip(run(), base):
            assert torch.isfinite(a.float()).all(), opts
            assert torch.equal(a, b), opts
    m.check_status()


@pytest.mark.parametrize("dtype", DTYPES)
def test_batch_independence(dtype):
    """"scan_segments" 0: a window's rows are bit-identical alone and inside a batch of 9."""
    D, L, B = 128, 64, 9
    m = mlm(D, dtype, scan_segments=0)
    ids = rand_ids(B, L, 8).to(DEV)
    pos, own = shared_positions(L), window_positions(B, L).to(DEV)
    for kw_all, kw_one in ((dict(positions=pos), dict(positions=pos)),
                           (dict(positions_per_window=own), dict(positions_per_window=own[5:6]))):
        for layers in (None, [NL]):
            batch = m.hidden_states_at(ids, layers=layers, **kw_all)
            alone = m.hidden_states_at(ids[5:6], layers=layers, **kw_one)
            assert torch.equal(alone[:, 0], batch[:, 5]), (dtype, list(kw_all), layers)
    m.check_status()


# ---- validation ----------------------------------------------------------------------------------------------------------------
def test_out_of_range_positions():
    """A per-window position of L + 3: PCAD_STATUS_BAD_POSITION and the rows of L - 1, at an intermediate level alone (the row kernel's
    check) and at every level; a shared position outside the window: PCAD_ERR_INVALID, nothing launched."""
    D, L, B = 128, 64, 3
    m = mlm(D, torch.float32)
    ids = rand_ids(B, L, 9).to(DEV)
    good = window_positions(B, L)
    bad = good.clone()
    bad[1, good[1].tolist().index(L - 1)] = L + 3
    for layers in ([1], None, [NL]):
        want = m.hidden_states_at(ids, layers=layers, positions_per_window=good.to(DEV)).cpu()
        m.check_status()
        got = m.hidden_states_at(ids, layers=layers, positions_per_window=bad.to(DEV)).cpu()
        assert m.status_bits() == engine.STATUS_BAD_POSITION, layers
        with pytest.raises(IndexError, match="position"):
            m.check_status()
        assert torch.equal(got, want), layers
    for shared in ([1, L], [-1]):
        with pytest.raises(RuntimeError, match=r"\(-1\).*out of range"):
            m.hidden_states_at(ids, layers=[1], positions=shared)
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, layers=[2, 1], positions=[1])
    with pytest.raises(ValueError):
        m.hidden_states_at(ids, positions=[1], positions_per_window=good.to(DEV))
    # a token id outside the vocabulary is reported as pcad_forward reports it, whichever levels are asked for
    ids2 = ids.clone()
    ids2[2, 7] = 9
    m.hidden_states_at(ids2, layers=[0, 1], positions=[3])
    assert m.status_bits() == engine.STATUS_BAD_TOKEN
    with pytest.raises(IndexError):
        m.check_status()
    m.hidden_states_at(ids, layers=[0, 1], positions=[3])
    m.check_status()


# ---- embeddings ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", DTYPES)
def test_extract_embeddings_last_layer_equals_default(dtype):
    """extract_embeddings(..., layer=-1) runs hidden_states_at(average=True) on pcad_forward's walk: bit-equal to layer=None, whose
    torch arithmetic the averaged form restates; an int and a list agree; level 0 is the averaged embedding-table rows."""
    m = mlm(128, dtype)
    tok = CaduceusTokenizer()
    rng = np.random.default_rng(3)
    seqs = ["".join(rng.choice(list("ACGTN"), size=64, p=[.24, .24, .24, .24, .04])) for _ in range(5)]
    base = embeddings.extract_embeddings(m, seqs, DEV, 31, tok)
    last = embeddings.extract_embeddings(m, seqs, DEV, 31, tok, layer=-1)
    assert last.dtype == np.float32 and last.shape == (5, 128)
    assert last.tobytes() == base.tobytes()
    both = embeddings.extract_embeddings(m, seqs, DEV, 31, tok, layer=[0, NL])
    assert both.shape == (5, 2, 128)
    # (with level 0 in the request the walk is the unfolded one; at this size - 640 token-rows - the fold does not engage either way)
    assert both[:, 1].tobytes() == base.tobytes()
    ids = torch.from_numpy(tok.encode_batch(seqs, mask_index=None)).long()
    comp = torch.tensor(m.config.complement_list())
    emb = m.get_input_embeddings().weight.detach().cpu()
    want0 = (emb[ids[:, 31]].float() + emb[comp[ids[:, 31]]].float()) / 2
    assert torch.equal(torch.from_numpy(both[:, 0]), want0)
