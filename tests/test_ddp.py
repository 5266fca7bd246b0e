"""CPU checks behind tests/test_gpu_grads_gather.py and tests/test_gpu_ddp.py: pcad_grads_flat_plan's layout is the
stated formula and it refuses what pcad_optim_plan refuses, without a device; the share rule - the ranks' micro-batches interleaved by
j mod W are the single process's with accumulation A W, and every rank's mask generator ends where the single process's does;
ddp.GradReducer over gloo on CPU tensors at worlds 2 and 4; ddp.init_from_env's device choice and refusals."""
import ctypes as C
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import optim_ref as OR
from plantcaduceus_amd import ddp, engine, ops

INV = -1                               # include/pcad.h PCAD_ERR_INVALID
F32, BF16 = 0, 1
P = 0x10000


@pytest.fixture(scope="module")
def lib():
    if not os.path.exists(engine.LIB_PATH) or not os.path.exists(engine.BWD_LIB_PATH):
        engine.build_library()
    return engine.load_bwd_library()


def rec(param=P, grad=P, master=None, m=P, v=P, n=5, pdt=F32, gdt=F32, flags=0):
    return (param, grad, master, m, v, n, pdt, gdt, flags)


def flat_plan(lib, records, offsets=True, total=True):
    """-> (status, offsets, total) of the C entry itself"""
    Record = ops._optim_record_type()
    tab = (Record * max(1, len(records)))()
    for r, x in zip(tab, records):
        r.param, r.grad, r.master, r.exp_avg, r.exp_avg_sq, r.n, r.param_dtype, r.grad_dtype, r.flags = x
    off = (C.c_int64 * max(1, len(records)))(*([-7] * max(1, len(records))))
    tot = C.c_int64(-7)
    rc = lib.pcad_grads_flat_plan(C.addressof(tab), len(records), C.addressof(off) if offsets else None, C.byref(tot) if total else None)
    return rc, list(off)[:len(records)], tot.value


def formula(sizes):
    up = [(n + 3) // 4 * 4 for n in sizes]
    return [sum(up[:i]) for i in range(len(sizes))], sum(up)


def test_flat_plan_is_the_formula(lib):
    """offset_i = sum_{j < i} round_up_4(n_j), total = sum_j round_up_4(n_j); sizes only, pointers are never dereferenced"""
    Ck = OR.CHUNK
    big = [(1 << 31) + 5, 1 << 31, 77, (1 << 30) + Ck - 1]                                  # more than 2^32 elements in all
    for sizes in ([0], [1], [3], [4], [5], [Ck], [Ck + 1], [0, 1, 3, 4, 5, Ck, Ck + 1], [5, 0, 0, 7, 0, 1], list(range(1, 51)) * 6, big):
        for gdt in (F32, BF16):
            rc, off, tot = flat_plan(lib, [rec(n=n, gdt=gdt) for n in sizes])
            assert rc == 0 and (off, tot) == formula(sizes), (sizes, gdt)
            assert all(o % 4 == 0 for o in off) and tot % 4 == 0
    assert formula([0, 1, 3, 4, 5, Ck, Ck + 1]) == ([0, 0, 4, 8, 12, 20, 20 + Ck], 24 + 2 * Ck)
    assert formula(big)[1] > 1 << 32 and formula(big)[0][3] == (1 << 31) + 8 + (1 << 31) + 80
    assert flat_plan(lib, [])[::2] == (0, 0)
    assert ops.grads_flat_plan([rec(n=n) for n in (5, 0, 2 * Ck + 1, Ck)]) == formula([5, 0, 2 * Ck + 1, Ck])


def test_flat_plan_refuses_what_optim_plan_refuses(lib):
    last = engine.load_library().pcad_last_error
    ok = rec()
    for field in ("param", "grad", "m", "v"):
        word = {"m": b"exp_avg", "v": b"exp_avg_sq"}.get(field, field.encode())
        rc, _, _ = flat_plan(lib, [ok, rec(**{field: P + 8})])
        assert rc == INV and b"pcad_grads_flat_plan" in last() and word in last() and b"table[1]" in last() and b"aligned" in last(), field
        rc, _, _ = flat_plan(lib, [rec(**{field: None})])
        assert rc == INV and word in last() and b"null" in last(), field
    assert flat_plan(lib, [rec(master=P + 4)])[0] == INV and b"master" in last() and b"aligned" in last()
    assert flat_plan(lib, [ok, ok, rec(n=-1)])[0] == INV and b"table[2].n" in last()
    assert flat_plan(lib, [rec(pdt=7)])[0] == INV and b"param_dtype" in last()
    assert flat_plan(lib, [rec(gdt=2)])[0] == INV and b"grad_dtype" in last()
    assert flat_plan(lib, [rec(pdt=BF16)])[0] == INV and b"master" in last()               # a bf16 param without master
    assert flat_plan(lib, [rec(pdt=BF16, master=P, gdt=BF16)])[0] == 0
    assert flat_plan(lib, [rec(flags=2)])[0] == INV and b"flags" in last()
    assert flat_plan(lib, [rec(n=0, param=None, grad=None, m=None, v=None, pdt=BF16)]) == (0, [0], 0)     # n == 0: pointers are not looked at
    assert flat_plan(lib, [rec(n=(1 << 24) * OR.CHUNK)])[0] == INV and b"2^24" in last()    # one chunk more than PCAD_OPTIM_MAX_CHUNKS
    assert flat_plan(lib, [rec(n=((1 << 24) - 1) * OR.CHUNK)])[::2] == (0, ((1 << 24) - 1) * OR.CHUNK)
    assert flat_plan(lib, [ok], offsets=False)[0] == INV and b"offsets_out" in last()
    assert flat_plan(lib, [ok], total=False)[0] == INV and b"total_out" in last()
    assert lib.pcad_grads_flat_plan(None, 2, None, None) == INV and b"table" in last()
    assert lib.pcad_grads_flat_plan(None, -1, None, None) == INV and b"count" in last()


def test_gather_entry_refuses_bad_arguments_without_a_device(lib):
    last = engine.load_library().pcad_last_error
    g = lambda table=P, cmap=P, count=3, chunks=5, offsets=P, flat=P, elems=100: lib.pcad_grads_gather(table, cmap, count, chunks, offsets, flat,
                                                                                                      elems, None)
    assert g(table=None) == INV and b"pcad_grads_gather" in last() and b"table" in last()
    assert g(table=P + 8) == INV and b"table" in last()
    assert g(cmap=None) == INV and b"chunk_map" in last()
    assert g(offsets=None) == INV and b"offsets" in last()
    assert g(offsets=P + 4) == INV and b"offsets" in last()
    assert g(flat=None) == INV and b"flat" in last()
    assert g(flat=P + 8) == INV and b"flat" in last()
    assert g(elems=-1) == INV and b"flat_elems" in last()
    assert g(chunks=-1) == INV and g(count=-1) == INV and g(chunks=1 << 24) == INV and b"2^24" in last()


# ---- the share rule -------------------------------------------------------------------------------------------------------------
L = 23


def _source(n, batch, accumulation, seed=11):
    from plantcaduceus_amd import mlm_eval, pretrain
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    g = np.random.default_rng(4)
    tok = CaduceusTokenizer()
    ids, special, w = mlm_eval.tokenize_windows(tok, ["".join(g.choice(list("ACGTacgt"), size=L)) for _ in range(n)], 0.5)
    return pretrain.BatchSource(ids, special, w, mlm_eval.make_collator(tok, 0.15), batch, accumulation, seed)


# n < batch A W (9 < 16: ranks with an empty share); a short last micro-batch (10 = 4 + 4 + 2); two steps per epoch, walked over the
# epoch boundary (24 windows, 3 steps)
@pytest.mark.parametrize("n,batch,A,W,steps", [(9, 4, 2, 2, 2), (3, 2, 1, 4, 2), (10, 4, 1, 3, 2), (10, 4, 3, 1, 2), (24, 3, 2, 2, 3), (24, 2, 1, 4, 4)])
def test_the_ranks_shares_are_the_single_process_batches(n, batch, A, W, steps):
    single = _source(n, batch, A * W)
    ranks = [_source(n, batch, A * W) for _ in range(W)]
    assert all(r.steps_per_epoch == single.steps_per_epoch for r in ranks)
    for step in range(steps):
        ref = single.step_batches(step)
        drawn = [r.step_batches(step) for r in ranks]                       # every rank draws all of them
        shares = [ddp.share(d, r, W) for r, d in enumerate(drawn)]
        assert sum(len(s) for s in shares) == len(ref) <= A * W
        assert len({1.0 / len(d) for d in drawn}) == 1 and len(drawn[0]) == len(ref)        # grad_scale is the same on every rank
        if n < batch * A * W and W > 1:
            assert any(len(s) == 0 for s in shares) or len(ref) >= W
        for j, want in enumerate(ref):
            got = shares[j % W][j // W]
            assert all(torch.equal(a, b) for a, b in zip(got, want)), (step, j)
        for r in ranks:
            assert torch.equal(r.mask_generator.get_state(), single.mask_generator.get_state())
    assert single.windows(steps - 1)[0].shape[0] <= batch


def test_labelled_batches_share_the_same_way():
    from plantcaduceus_amd import lora_predict
    ids, labels = np.arange(7 * 5, dtype=np.int64).reshape(7, 5), np.arange(7, dtype=np.int64)
    single = lora_predict.LabelledBatches(ids, labels, 2, 4, 3)
    assert [len(b[0]) for b in single.step_batches(0)] == [2, 2, 2, 1]      # a short last micro-batch
    for W in (2, 4):
        ref = single.step_batches(0)
        for j, want in enumerate(ref):
            got = ddp.share(lora_predict.LabelledBatches(ids, labels, 2, 4, 3).step_batches(0), j % W, W)[j // W]
            assert torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])


# ---- GradReducer over gloo on CPU tensors -----------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


TOTAL = 1000


def _rank_values(rank):
    g = torch.Generator().manual_seed(100 + rank)
    return torch.randn(TOTAL, generator=g), float(rank + 1) * 0.25


def _reducer_worker(rank, ws, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.set_num_threads(1)
        r = ddp.GradReducer(dist.group.WORLD, "cpu")
        flat = r.allocate(TOTAL)
        assert flat.shape == (TOTAL + ddp.TAIL,) and r.world == ws and r.backend == "gloo" and r.host is None and r.allocate(TOTAL) is flat
        grads, loss = _rank_values(rank)
        r.grads.copy_(grads)
        r.loss.fill_(loss)
        r.all_reduce()
        first = r.flat.clone()
        r.grads.copy_(grads)                                                # a second step: one rank's inf reaches every rank
        if rank == 1:
            r.grads[17] = float("inf")
        r.loss.fill_(loss)
        r.all_reduce()
        sums = [ddp.check_in_step([first], 3)]
        raised = ""
        try:
            ddp.check_in_step([first + (1.0 if rank == ws - 1 else 0.0)], 5)
        except RuntimeError as ex:
            raised = str(ex)
        torch.save({"first": first, "second": r.flat.clone(), "sum": sums[0], "raised": raised}, os.path.join(outdir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 4])
def test_grad_reducer_over_gloo(tmp_path, ws):
    mp.spawn(_reducer_worker, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt") for r in range(ws)]
    vals = [_rank_values(r) for r in range(ws)]
    ref = torch.stack([v[0].double() for v in vals]).sum(0)
    for g in got:
        assert torch.equal(g["first"], got[0]["first"]) and torch.equal(g["second"], got[0]["second"])     # every rank ends with the same bits
        assert g["sum"] == got[0]["sum"]
        assert "step 5" in g["raised"] and "rank 0" in g["raised"]          # a mismatch raises on every rank and names the step
    first = got[0]["first"]
    # a sum of ws fp32 terms: within (ws - 1) roundings of the float64 sum of the same values; two terms: exactly the fp32 sum
    assert float((first[:TOTAL].double() - ref).abs().max()) <= (ws - 1) * 2.0 ** -24 * float(torch.stack([v[0].abs() for v in vals]).sum(0).max())
    if ws == 2:
        assert torch.equal(first[:TOTAL], vals[0][0] + vals[1][0])
    assert float(first[TOTAL]) == sum(v[1] for v in vals) and bool((first[TOTAL + 1:] == 0).all())          # the loss slot holds the sum
    second = got[0]["second"]
    assert bool(torch.isinf(second[17])) and bool(torch.isfinite(second[:17]).all()) and not np.isfinite(float(second[:TOTAL].double().pow(2).sum()))


def test_grad_reducer_without_a_group_is_a_world_of_one():
    r = ddp.GradReducer(None, "cpu")
    flat = r.allocate(8)
    flat.copy_(torch.arange(12.0))
    r.all_reduce()
    assert r.world == 1 and torch.equal(flat, torch.arange(12.0)) and torch.equal(r.grads, torch.arange(8.0)) and float(r.loss) == 8.0
    assert r.allocate(16) is not flat and r.flat.shape == (20,) and not bool(r.flat.any())
    assert int(ddp.checksum([torch.tensor([1.0, -1.0])])) == 0x3F800000 + (0xBF800000 - (1 << 32))


# ---- init_from_env ------------------------------------------------------------------------------------------------------------------
def test_init_from_env_device_choice(monkeypatch):
    for k in ("WORLD_SIZE", "RANK", "LOCAL_RANK"):
        monkeypatch.delenv(k, raising=False)
    assert ddp.init_from_env("cuda:3", "gloo", device_count=1) == ("cuda:3", 0, 1) and not dist.is_initialized()      # plain python: no group
    assert ddp.rank_device("nccl", 0, 1) == "cuda:0" and ddp.rank_device("nccl", 5, 8) == "cuda:5"
    assert [ddp.rank_device("gloo", r, 1) for r in range(4)] == ["cuda:0"] * 4
    assert [ddp.rank_device("gloo", r, 2) for r in range(4)] == ["cuda:0", "cuda:1", "cuda:0", "cuda:1"]
    with pytest.raises(SystemExit, match="one device per rank"):
        ddp.rank_device("nccl", 1, 1)
    with pytest.raises(SystemExit, match="one of nccl, gloo"):
        ddp.rank_device("mpi", 0, 1)
    # under a launcher's environment the refusal comes before any group is made
    monkeypatch.setenv("WORLD_SIZE", "2")
    monkeypatch.setenv("RANK", "1")
    monkeypatch.setenv("LOCAL_RANK", "1")
    with pytest.raises(SystemExit, match="LOCAL_RANK 1 has no device of its own"):
        ddp.init_from_env("cuda:0", None, device_count=1)                   # nccl is the default
    assert not dist.is_initialized()
    made = []
    monkeypatch.setattr(dist, "init_process_group", lambda **kw: made.append(kw))
    monkeypatch.setattr(dist, "get_rank", lambda *a: 1)
    monkeypatch.setattr(dist, "get_world_size", lambda *a: 2)
    monkeypatch.setattr(torch.cuda, "set_device", lambda d: None)
    assert ddp.init_from_env("cuda:0", "gloo", device_count=1) == ("cuda:0", 1, 2) and made == [{"backend": "gloo"}]
    assert ddp.init_from_env("cuda:0", "nccl", device_count=2)[0] == "cuda:1" and made[1]["backend"] == "nccl"
    monkeypatch.setattr(ddp, "_OWN_GROUP", False)


def test_backend_from_flag_and_environment():
    assert ddp.backend_from(None, {}) is None and ddp.backend_from("gloo", {"PCAD_DDP_BACKEND": "nccl"}) == "gloo"      # the flag wins
    assert ddp.backend_from(None, {"PCAD_DDP_BACKEND": "gloo"}) == "gloo"
    with pytest.raises(SystemExit):
        ddp.backend_from(None, {"PCAD_DDP_BACKEND": "mpi"})
    from plantcaduceus_amd import pretrain
    base = ["--dataset_name", "d", "--output_dir", "o"]
    assert pretrain.build_parser().parse_args(base).ddp_backend is None
    assert pretrain.build_parser().parse_args(base + ["--ddp_backend", "gloo"]).ddp_backend == "gloo"
