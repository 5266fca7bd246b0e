"""-m gpu: fp32 main gradients in bf16 training: ops.linear_fn + pcad_linear_wgrad under training.TrainableCaduceusForMaskedLM,
optim.AdamW(fp32_grad_accumulation=True), `pretrain --fp32_grad_accumulation` and its data-parallel form.

Geometry: §4n's toy - d_model 64, d_inner 128, n_layer 2, B = 2, L = 69, bf16.  dt_rank 8 puts all four projections on the kernel
(in_proj 256 x 64, out_proj 64 x 128, x_proj 40 x 128, dt_proj 128 x 8): a counting wrapper around ops.linear_wgrad sees 7 calls per layer
and backward (in_proj once - its output feeds both directions -, x_proj, dt_proj and the tied out_proj once per direction) onto the
4 projections of each layer (6 weight tensors: x_proj and dt_proj exist per direction).  dt_rank 4 (x_proj 36 x 128, dt_proj 128 x 4) is
the addmm fallback: 3 calls per layer.

  (a) one micro-batch   the loss is torch.equal to the default model's (the forward is the same calls); every main_grad against the default
                        path's .grad.float() within the bf16-stored bar 2^-7 by scan_bwd_ref.metric; no parameter keeps a .grad
  (b) A = 16            G64 = the float64 sum of the default path's bf16 .grad taken one micro-batch at a time (the parent's code);
                        E_default = metric(the default path's bf16-accumulated .grad, G64), E_main = metric(main_grad, G64):
                        E_main < E_default for every projection weight and for their set as a whole.  The ratios are printed, not asserted
  (c) recompute         gradient checkpointing on against off: every main_grad torch.equal after one micro-batch and after two
  (d) optimizer         accumulation 1: the masters after one step torch.equal to ops.adamw_step fed the same gradients through the existing
                        (bf16 param, fp32 grad) flat table; zero_grad() leaves every slice and the padding +0 and the reducer's tail alone;
                        with reducer=GradReducer(None, dev) the same masters and no ops.grads_gather call
  (e) command           pretrain --dtype bfloat16 --fp32_grad_accumulation --gradient_accumulation_steps 4, 6 steps: finite parameters =
                        the rounded masters, no skipped step, the output loads into CaduceusForMaskedLM; rerun from checkpoint-3:
                        model.safetensors equal
  (f) data parallel     one gloo world-2 step at accumulation 1 against the single process at accumulation 2: the reduced flat buffer per
                        tensor within §4r's accumulation bar 2 (2 n_layer + 1) 3e-5 of max |g| (only the order of an fp32 sum differs);
                        both ranks' checksums equal; no gather launch
Every case prints its figures before it asserts.

Observed on an MI355X: (a) worst main_grad against .grad 4.1e-3 (dt_rank 8) / 5.2e-3 (4) [7.8e-3], 32 / 30 of 36 tensors bit-equal after
rounding; (b) E_default 3.8e-3 .. 1.4e-2, E_main 8.2e-4 .. 1.6e-3, ratios 2.9 .. 16.4 per tensor and 6.2 over the set; (c), (d) and the
resume of (e) bit-equal; (f) 8.0e-8 of max |g| [3e-4], equal checksums."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import _ddp_worker as W
import scan_bwd_ref as SB
import scan_ref as R
from plantcaduceus_amd import ops
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
WORKER = os.path.join(ROOT, "tests", "_main_grad_worker.py")
DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
B, L, SEED, N_LAYER = 2, 69, 42, 2
PROJECTIONS = ("in_proj", "x_proj", "dt_proj", "out_proj")


def toy_config(dt_rank):
    return make_config("toy", d_model=64, n_layer=N_LAYER, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=dt_rank, bias=False, conv_bias=True))


def batch(seed):
    """ids, labels (about 15 % of both windows), loss_weights"""
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(3, 7, (B, L), generator=g)
    keep = torch.rand(B, L, generator=g) < 0.15
    keep[:, 3] = True
    labels = torch.where(keep, torch.randint(3, 7, (B, L), generator=g), torch.full((B, L), -100)).to(torch.int32)
    return ids.to(DEV), labels.to(DEV), torch.ones(B, L, device=DEV)


def model_of(dt_rank, recompute=False, main=False, **opt_kw):
    """-> (model, optimizer or None): the bf16 toy model from the seeded state dict; main: with fp32 main gradients attached"""
    from plantcaduceus_amd.optim import AdamW
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    cfg = toy_config(dt_rank)
    m = TrainableCaduceusForMaskedLM(cfg, dtype=BF, device=DEV, gradient_checkpointing=recompute)
    m.load_state_dict(synthetic_state_dict(cfg, seed=SEED, stress=False))
    return m, (AdamW(m.named_parameters(), lr=1e-3, weight_decay=0.1, fp32_grad_accumulation=True, **opt_kw) if main else None)


def named(model):
    """each Parameter once, under its first name (tied weights appear once)"""
    seen, out = set(), {}
    for k, p in model.named_parameters():
        if id(p) not in seen:
            seen.add(id(p))
            out[k] = p
    return out


def is_projection(name):
    return name.endswith(".weight") and name.split(".")[-2] in PROJECTIONS


def backward(model, seed):
    out = model(*batch(seed))
    out.loss.backward()
    return out.loss.detach()


class Counting:
    """a wrapper that counts the calls of a function of plantcaduceus_amd.ops and keeps what identifies each"""

    def __init__(self, monkeypatch, name, key=lambda *a, **k: None):
        self.calls, inner = [], getattr(ops, name)

        def wrapper(*a, **k):
            self.calls.append(key(*a, **k))
            return inner(*a, **k)
        for attr in ("guards_ok", "last_outputs"):
            if hasattr(inner, attr):
                setattr(wrapper, attr, getattr(inner, attr))
        monkeypatch.setattr(ops, name, wrapper)


@pytest.mark.parametrize("dt_rank", [8, 4])
def test_one_micro_batch_against_the_default_path(dt_rank, monkeypatch):
    ref, _ = model_of(dt_rank)
    model, opt = model_of(dt_rank, main=True)
    count = Counting(monkeypatch, "linear_wgrad", key=lambda dy, x, out=None, **k: out.data_ptr())
    loss_ref, loss = backward(ref, 17), backward(model, 17)
    torch.cuda.synchronize()
    params, refs = named(model), named(ref)
    owner = {p.main_grad.data_ptr(): k for k, p in params.items()}
    on_kernel = [owner[ptr] for ptr in count.calls]
    pairs = {(k.split(".layers.")[1].split(".")[0], k.split(".")[-2]) for k in on_kernel}
    per_layer = 7 if dt_rank == 8 else 3
    print(f"dt_rank {dt_rank}: loss {loss.item():.7f} / {loss_ref.item():.7f}; {len(count.calls)} linear_wgrad calls onto {len(set(on_kernel))} weight "
          f"tensors = {len(pairs)} (layer, projection) pairs")
    assert torch.equal(loss, loss_ref)
    assert len(count.calls) == per_layer * N_LAYER and all(is_projection(k) for k in on_kernel)
    if dt_rank == 8:
        assert len(pairs) == 4 * N_LAYER and len(set(on_kernel)) == 6 * N_LAYER
        assert sum(is_projection(k) for k in params) == 6 * N_LAYER
    else:
        assert {pr for _, pr in pairs} == {"in_proj", "out_proj"}
    worst, equal = 0.0, 0
    for k, p in params.items():
        g = refs[k].grad
        assert p.grad is None and g is not None and p.main_grad.dtype == F32 and p.main_grad.shape == p.shape, k
        e = SB.metric(p.main_grad, g.float())
        worst = max(worst, e)
        equal += int(torch.equal(p.main_grad.to(BF), g))
        assert e <= R.BAR_SCAN[True], (k, e)
        if not is_projection(k):
            assert torch.equal(p.main_grad, g.float()), k                       # the hook adds the very gradient the default path has
    print(f"dt_rank {dt_rank}: worst main_grad vs .grad.float() {worst:.2e} [bar {R.BAR_SCAN[True]:.2e}]; {equal} of {len(params)} tensors bit-equal "
          f"after rounding main_grad to bf16")
    assert opt.flat.numel() >= sum(p.numel() for p in params.values())


def test_sixteen_micro_batches_are_summed_better_than_in_bf16():
    A = 16
    ref, _ = model_of(8)
    names = [k for k in named(ref) if is_projection(k)]
    refs = named(ref)
    g64 = {k: torch.zeros(refs[k].shape, dtype=torch.float64, device=DEV) for k in names}
    for j in range(A):                                          # one micro-batch at a time: the reference
        for p in ref.parameters():
            p.grad = None
        backward(ref, 100 + j)
        for k in names:
            g64[k] += refs[k].grad.double()
    for p in ref.parameters():
        p.grad = None
    for j in range(A):                                          # the default path: .grad accumulates in bf16
        backward(ref, 100 + j)
    model, _ = model_of(8, main=True)
    for j in range(A):
        backward(model, 100 + j)
    torch.cuda.synchronize()
    params = named(model)
    e_def = {k: SB.metric(refs[k].grad, g64[k]) for k in names}
    e_main = {k: SB.metric(params[k].main_grad, g64[k]) for k in names}
    for k in names:
        print(f"A = {A} {k}: E_default {e_def[k]:.3e} E_main {e_main[k]:.3e} ratio {e_def[k] / e_main[k]:.1f}")
    cat = lambda ts: torch.cat([t.reshape(-1).double() for t in ts])
    whole = cat([g64[k] for k in names])
    all_def = SB.metric(cat([refs[k].grad for k in names]), whole)
    all_main = SB.metric(cat([params[k].main_grad for k in names]), whole)
    print(f"A = {A} all projection weights: E_default {all_def:.3e} E_main {all_main:.3e} ratio {all_def / all_main:.1f}")
    assert len(names) == 6 * N_LAYER and refs[names[0]].grad.dtype == BF
    assert all(e_main[k] < e_def[k] for k in names), [k for k in names if not e_main[k] < e_def[k]]
    assert all_main < all_def


def test_recompute_gives_the_same_main_gradients():
    on, _ = model_of(8, recompute=True, main=True)
    off, _ = model_of(8, recompute=False, main=True)
    assert on.is_gradient_checkpointing and not off.is_gradient_checkpointing
    for step, seed in enumerate((17, 18)):
        la, lb = backward(on, seed), backward(off, seed)
        differ = [k for (k, p), q in zip(named(on).items(), named(off).values()) if not torch.equal(p.main_grad, q.main_grad)]
        print(f"recompute on / off after micro-batch {step + 1}: loss {la.item():.7f} / {lb.item():.7f}; main gradients that differ: {differ}")
        assert torch.equal(la, lb) and not differ
        assert all(p.grad is None for p in on.parameters()) and any(bool((p.main_grad != 0).any()) for p in on.parameters())


def test_optimizer_steps_on_the_main_gradients(monkeypatch):
    from plantcaduceus_amd.ddp import GradReducer
    gathers = Counting(monkeypatch, "grads_gather")
    hp = dict(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1, step=1, max_norm=1.0, grad_scale=1.0)
    masters = {}
    for tag, kw in (("plain", {}), ("reducer", {"reducer": GradReducer(None, DEV)})):
        model, opt = model_of(8, main=True, **kw)
        backward(model, 17)
        if tag == "plain":
            # the same gradients through the existing (bf16 param, fp32 grad) flat table
            params = [p.detach().clone() for p in opt.params]
            base = ops.OptimTable(params, [torch.zeros_like(p) for p in params], [m.clone() for m in opt.master],
                                  [torch.zeros_like(m) for m in opt.master], [torch.zeros_like(m) for m in opt.master], opt.decay)
            assert base.flat_plan()[1] == opt.flat.numel()
            flat = base.on_flat(opt.flat.clone())
            ops.adamw_step(flat, **hp)
            masters["table"] = flat.masters
        else:
            assert opt.flat.data_ptr() == kw["reducer"].grads.data_ptr()       # the reducer's own buffer
            kw["reducer"].loss.fill_(3.0)
        opt.step()
        st = opt.state()
        masters[tag] = opt.master
        assert st["finite"] == 1 and st["skipped"] == 0 and st["norm"] > 0 and bool((opt.flat != 0).any())
        assert all(torch.equal(p, m.to(BF)) for p, m in zip(opt.params, opt.master))
        opt.zero_grad()
        whole = opt.flat if tag == "plain" else kw["reducer"].flat[:-4]
        assert bool((whole.view(torch.int32) == 0).all())                       # every slice and the padding: +0
        assert all(bool((p.main_grad.view(torch.int32) == 0).all()) and p.grad is None for p in opt.params)
        if tag == "reducer":
            assert kw["reducer"].loss.item() == 3.0 and kw["reducer"].flat.numel() == opt.flat.numel() + 4
    same = lambda a, b: all(torch.equal(x, y) for x, y in zip(a, b))
    print(f"masters after one step: table {same(masters['plain'], masters['table'])}, reducer {same(masters['plain'], masters['reducer'])}; "
          f"grads_gather calls {len(gathers.calls)}")
    assert same(masters["plain"], masters["table"]) and same(masters["plain"], masters["reducer"])
    assert not gathers.calls


def command(data, cfg, out, *extra):
    from plantcaduceus_amd import pretrain
    return pretrain.main(["--config_name", cfg, "--dataset_name", data, "--do_train", "--output_dir", str(out), "--per_device_train_batch_size",
                          str(W.BATCH), "--gradient_accumulation_steps", "4", "--learning_rate", str(W.LR), "--lr_scheduler_type", "constant",
                          "--max_steps", "6", "--logging_steps", "1", "--save_steps", "3", "--seed", str(W.SEED), "--device", DEV,
                          "--dtype", "bfloat16", "--fp32_grad_accumulation", *extra])


def test_command_runs_resumes_and_its_output_loads(tmp_path):
    from safetensors.torch import load_file
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    data, cfg = W.write_inputs(tmp_path)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    res = command(data, cfg, a)
    sd = load_file(str(a / "checkpoint-6" / "model.safetensors"))
    opt = torch.load(str(a / "checkpoint-6" / "optimizer.pt"), weights_only=False)
    with open(a / "trainer_state.json") as f:
        hist = json.load(f)["log_history"]
    print(f"losses {[round(e['loss'], 5) for e in hist]}; grad norms {[round(e['grad_norm'], 4) for e in hist]}")
    assert opt["step"] == 6 and opt["skipped"] == 0 and res["train"]["skipped_steps"] == 0 and len(opt["names"]) == len(sd)
    assert sorted(opt) == ["exp_avg", "exp_avg_sq", "master", "names", "skipped", "step"]          # nothing new is saved
    for name, master in zip(opt["names"], opt["master"]):
        assert sd[name].dtype == BF and master.dtype == F32 and bool(torch.isfinite(master).all()), name
        assert torch.equal(sd[name], master.to(BF)), name
    assert all(np.isfinite(e["loss"]) and e["skipped_steps"] == 0 for e in hist) and hist[-1]["loss"] < hist[0]["loss"]
    eng = CaduceusForMaskedLM.from_pretrained(str(a)).to(BF).to(DEV).eval()
    with torch.no_grad():
        lg = eng(input_ids=batch(5)[0]).logits
    assert bool(torch.isfinite(lg.float()).all())
    command(data, cfg, b, "--resume_from_checkpoint", str(a / "checkpoint-3"))
    wa, wb = load_file(str(a / "model.safetensors")), load_file(str(b / "model.safetensors"))
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)


def _free_port():
    import socket
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def run_worker(world, out, accumulation):
    import _main_grad_worker as MW
    os.makedirs(out, exist_ok=True)
    args = [str(out), str(accumulation), "--backend", "gloo"]
    if world == 0:                                              # one process, no group: in this one
        MW.main(args)
        return [torch.load(os.path.join(out, "r0.pt"), weights_only=False)]
    env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0", PYTHONPATH=ROOT + os.pathsep + os.environ.get("PYTHONPATH", ""))
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", f"--nproc-per-node={world}", "--master-addr", "127.0.0.1",
           "--master-port", str(_free_port()), WORKER] + args
    r = subprocess.run(cmd, cwd=ROOT, env=env, capture_output=True, text=True, timeout=240)
    assert r.returncode == 0, r.stdout[-2000:] + r.stderr[-4000:]
    return [torch.load(os.path.join(out, f"r{k}.pt"), weights_only=False) for k in range(world)]


def test_world2_gloo_against_accumulation_2(tmp_path):
    one = run_worker(0, tmp_path / "one", 2)[0]
    ranks = run_worker(2, tmp_path / "two", 1)
    gbar = 2 * (2 * N_LAYER + 1) * R.BAR_SCAN[False]
    assert abs(gbar - 3e-4) < 1e-12
    first = ranks[0]
    assert [r["rank"] for r in ranks] == [0, 1] and all(r["world"] == 2 and r["scale"] == 0.5 == one["scale"] for r in ranks)
    assert torch.equal(ranks[1]["flat"], first["flat"]) and ranks[1]["checksum"] == first["checksum"] and ranks[1]["state"] == first["state"]
    assert first["offsets"] == one["offsets"] and first["names"] == one["names"] and first["total"] == one["total"] == first["flat"].numel()
    worst = 0.0
    for name, o, n in zip(first["names"], first["offsets"], first["sizes"]):
        ga, gb = one["flat"][o:o + n].double(), first["flat"][o:o + n].double()
        top = ga.abs().max().item()
        d = (ga - gb).abs().max().item()
        worst = max(worst, d / top)
        assert top > 0 and d <= gbar * top, (name, d, top)
    print(f"world 2 vs accumulation 2: worst |d flat| / max |g| over the tensors {worst:.2e} [bar {gbar:.1e}]; checksums "
          f"{[r['checksum'] for r in ranks]}; norms {first['state']['norm']:.7f} / {one['state']['norm']:.7f}; loss {first['loss']:.6f} / {one['loss']:.6f}")
    for r in ranks + [one]:
        assert r["state"]["finite"] == 1 and r["changed"] and r["rounded"] and r["gathers"] == 0 and r["grads_left"] == 0
        assert bool((r["flat_after"].view(torch.int32) == 0).all())             # zero_grad left +0
