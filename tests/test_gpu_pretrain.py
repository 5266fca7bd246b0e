"""-m gpu: the training loop of plantcaduceus_amd.pretrain on optim.AdamW, on the tiny geometry of
tests/test_gpu_training_model.py (n_layer 2, d_model 64, d_inner 128, dt_rank 4): 8 windows of L = 69, batch 4, fp32, lr 1e-3, no
warm-up, weights from checkpoint.synthetic_state_dict(stress=False) - the initialisation `--config_name` alone gives.

  trajectory    20 step losses under optim.AdamW against the same loop under torch.optim.AdamW(foreach=False) + clip_grad_norm_ on the
                GPU (same model, masks, order): max relative difference within 10 x the largest difference between torch's own
                foreach=False and foreach=True trajectories (two implementations of the reference: their distance is the noise),
                floored at 1e-6; and the last loss is below the first
  accumulation  accumulation 2 at batch 2 against accumulation 1 at batch 4, micro-batches of equal label-weight sums: master, m, v after
                the first step through Trainer.train_step: scale x accumulated gradients = the batch-4 gradients per tensor within
                2 (2 n_layer + 1) 3e-5 of max |g|, the norms agree, coef halves, and each run's update sits at the operator bar of
                tests/test_gpu_optim.py against the float64 restatement of its own gradients
  resume        the command to --max_steps 6, rerun from checkpoint-3: model.safetensors bit-equal, log histories equal from step 4 on
  output loads  CaduceusForMaskedLM.from_pretrained(output_dir) under mlm_eval.evaluate_split, called directly and through the command's
                --do_eval: eval_loss_token_mean equals the trainable model's loss on the same masks within test_gpu_training_model's
                forward bar 2 x 1e-4 x max |logit|.  The masks are evaluate_split's own (it seeds and draws them itself and takes none),
                drawn again the same way for the trainable model - not the final training step's, which cannot be handed to it
  bf16          --dtype bfloat16, 6 steps: finite parameters, fp32 optimizer state, parameters = rounded masters, last loss below first
Every case prints its figures before it asserts.  Observed on an MI355X: DESIGN.md §4o."""
import json
import os

import numpy as np
import pytest
import torch

import optim_ref as OR
from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
BF, F32 = torch.bfloat16, torch.float32
N_WIN, L, BATCH, LR, SEED = 8, 69, 4, 1e-3, 42


def toy_config():
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def sequences():
    g = np.random.default_rng(9)
    return ["".join(g.choice(list("ACGTacgt"), size=L)) for _ in range(N_WIN)]


def fresh_model(dtype=F32):
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    cfg = toy_config()
    m = TrainableCaduceusForMaskedLM(cfg, dtype=dtype, device=DEV)
    m.load_state_dict(synthetic_state_dict(cfg, seed=SEED, stress=False))
    return m


def args(tmp, *extra):
    from plantcaduceus_amd import pretrain
    return pretrain.build_parser().parse_args(["--dataset_name", str(tmp), "--output_dir", str(tmp), "--per_device_train_batch_size", str(BATCH),
                                               "--learning_rate", str(LR), "--lr_scheduler_type", "constant", "--logging_steps", "1",
                                               "--save_steps", "0", "--seed", str(SEED), "--device", DEV, *extra])


def batch_source(batch=BATCH, accumulation=1):
    from plantcaduceus_amd import mlm_eval, pretrain
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    tok = CaduceusTokenizer()
    ids, special, w = mlm_eval.tokenize_windows(tok, sequences(), 1.0)
    return pretrain.BatchSource(ids, special, w, mlm_eval.make_collator(tok, 0.15), batch, accumulation, SEED), tok


class TorchOptimizer:
    """clip_grad_norm_ + torch.optim.AdamW behind optim.AdamW's interface, with its decay rule"""

    def __init__(self, model, foreach, lr, max_norm=1.0):
        from plantcaduceus_amd import optim
        named = list(model.named_parameters())
        self.params = [p for _, p in named]
        self.opt = OR.torch_adamw(self.params, [optim.applies_weight_decay(k, p) for k, p in named], lr, 0.9, 0.999, 1e-8, 0.0, foreach=foreach)
        self.foreach, self.max_norm, self.grad_scale, self.norm = foreach, max_norm, 1.0, None

    def step(self, lr):
        for g in self.opt.param_groups:
            g["lr"] = lr
        if self.grad_scale != 1.0:
            for p in self.params:
                p.grad.mul_(self.grad_scale)
        self.norm = torch.nn.utils.clip_grad_norm_(self.params, self.max_norm, foreach=self.foreach)
        self.opt.step()

    def zero_grad(self):
        self.opt.zero_grad(set_to_none=False)

    def state(self):
        return {"norm": float(self.norm), "coef": float("nan"), "finite": 1, "skipped": 0}


def run_loop(tmp, which, steps=20):
    from plantcaduceus_amd import optim, pretrain
    model = fresh_model()
    src, tok = batch_source()
    opt = optim.AdamW(model.named_parameters(), lr=LR) if which == "fused" else TorchOptimizer(model, which == "foreach", LR)
    tr = pretrain.Trainer(model, opt, src, tok, args(tmp), steps, 0)
    tr.run()
    return np.array([e["loss"] for e in tr.log_history], dtype=np.float64), tr.log_history


def test_loss_trajectory_against_torch_adamw(tmp_path):
    fused, hist = run_loop(tmp_path, "fused")
    single, hist_t = run_loop(tmp_path, "single")
    foreach, _ = run_loop(tmp_path, "foreach")
    assert len(fused) == len(single) == len(foreach) == 20 and np.isfinite(fused).all()
    noise = float(np.max(np.abs(single - foreach) / np.abs(single)))
    diff = float(np.max(np.abs(fused - single) / np.abs(single)))
    bar = max(10 * noise, 1e-6)
    print("fused   " + " ".join(f"{v:.6f}" for v in fused))
    print("torch   " + " ".join(f"{v:.6f}" for v in single))
    print(f"max relative difference fused vs torch foreach=False {diff:.3e} [bar {bar:.3e}; torch foreach=False vs foreach=True {noise:.3e}]")
    print(f"grad norms fused {hist[0]['grad_norm']:.6f} .. {hist[-1]['grad_norm']:.6f}; torch {hist_t[0]['grad_norm']:.6f} .. {hist_t[-1]['grad_norm']:.6f}")
    assert diff <= bar
    assert fused[-1] < fused[0]
    assert all(e["skipped_steps"] == 0 for e in hist) and [e["step"] for e in hist] == list(range(1, 21))


class FixedBatches:
    """a batch source that hands Trainer.train_step the given micro-batches"""

    def __init__(self, batches):
        self.batches, self.steps_per_epoch = batches, 1

    def step_batches(self, step):
        return self.batches


def test_accumulation_two_at_batch_two_is_batch_four():
    """Trainer.train_step over one micro-batch of 4 windows and over two of 2, labels chosen so that both micro-batches carry the same
    label-weight sum (6 labelled positions of weight 1 per window), since the loss is a ratio per micro-batch.  Three things are held:
      the gradients   grad_scale (the loop's own) x the accumulated gradients against the batch-4 gradients, per tensor, within
                      2 (2 n_layer + 1) 3e-5 of the tensor's max |g|: tests/test_gpu_training_model.py holds every fp32 parameter
                      gradient of this geometry to (2 n_layer + 1) 3e-5 of its maximum from the float64 graph (R.BAR_SCAN per summed
                      direction and layer, and the head), so two ways of summing the same gradient differ by at most twice that.  The bar
                      is fixed by the batch-4 run alone.  Observed: 8.8e-7 of max |g| at worst
      the norms       the two steps' device norms, within the norm such a gradient difference can make (sqrt(sum n_t (bar max |g_t|)^2))
                      plus optim_ref.norm_bar of each; and coef of the second = half the first's, to the same relative bound
      the update      each run's master, m, v against the float64 restatement of ITS OWN gradients at the operator bar of
                      tests/test_gpu_optim.py unchanged (4 x torch's fp32 CPU AdamW's distance on those gradients, floored at 2 ulp of max |p|)
    The two runs' p are not compared with each other directly: below eps the first step's update is lr g / eps, so an element of layer
    1's in_proj.weight whose gradient (stock F.linear's backward) is 6.23e-9 summed at once and 5.95e-9 summed as two micro-batches - in a
    tensor whose gradients reach 8.8e-2 - moves p by 2.5e-6 under any optimizer; the gradient bar above is where that difference is held."""
    import scan_ref as R
    from plantcaduceus_amd import optim, pretrain
    src, tok = batch_source()
    g = torch.Generator().manual_seed(5)
    ids = torch.from_numpy(src.ids[:4]).to(torch.int32)
    labels = torch.full((4, L), -100, dtype=torch.int32)
    for b in range(4):
        at = torch.randperm(L, generator=g)[:6]
        labels[b, at] = ids[b, at]
    masked = ids.clone()
    masked[labels != -100] = tok.mask_token_id
    weights = torch.ones(4, L)
    hp = dict(lr=LR, beta1=0.9, beta2=0.999, eps=1e-8, weight_decay=0.1)
    init = [p.detach().cpu().clone() for _, p in fresh_model().named_parameters()]
    dist = lambda got, ref: max((a.double() - b.double()).abs().max().item() for a, b in zip(got, ref))
    runs = {}
    for name, micro in (("batch 4", [slice(0, 4)]), ("2 x batch 2", [slice(0, 2), slice(2, 4)])):
        model = fresh_model()
        opt = optim.AdamW(model.named_parameters(), lr=LR, weight_decay=0.1)
        kept = []
        opt.zero_grad = lambda opt=opt, kept=kept: kept.extend(p.grad.detach().cpu().clone() for p in opt.params)     # keep what the step saw
        tr = pretrain.Trainer(model, opt, FixedBatches([(masked[sl], labels[sl], weights[sl]) for sl in micro]), tok, args("."), 1, 0)
        tr.train_step()
        torch.cuda.synchronize()
        r = runs[name] = dict(p=[p.detach().cpu() for p in opt.params], m=[t.cpu() for t in opt.exp_avg], v=[t.cpu() for t in opt.exp_avg_sq],
                              state=opt.state(), grads=kept, scale=opt.grad_scale, names=opt.names, chunks=opt.table().chunks)
        assert r["scale"] == 1.0 / len(micro) and len(kept) == len(init)
        # the update, against the float64 restatement and torch's fp32 CPU AdamW on this run's own gradients
        p64, m64, v64 = [t.double() for t in init], [torch.zeros_like(t, dtype=torch.float64) for t in init], [torch.zeros_like(t, dtype=torch.float64) for t in init]
        norm64, coef64, _ = OR.adamw_step(p64, kept, m64, v64, opt.decay, step=1, max_norm=1.0, grad_scale=r["scale"], **hp)
        tp = [torch.nn.Parameter(t.clone()) for t in init]
        topt = OR.torch_adamw(tp, opt.decay, foreach=False, **hp)
        for p, gr in zip(tp, kept):
            p.grad = gr * r["scale"]
        torch.nn.utils.clip_grad_norm_(tp, 1.0, foreach=False)
        topt.step()
        ulp = float(np.spacing(np.float32(max(p.abs().max().item() for p in p64))))
        tor = {"p": dist([p.detach() for p in tp], p64), "m": dist([topt.state[p]["exp_avg"] for p in tp], m64),
               "v": dist([topt.state[p]["exp_avg_sq"] for p in tp], v64)}
        for q, ref in (("p", p64), ("m", m64), ("v", v64)):
            d, bar = dist(r[q], ref), max(4 * tor[q], 2 * ulp)
            print(f"{name}: {q} {d:.3e} [bar {bar:.3e}; torch fp32 {tor[q]:.3e}, ulp {ulp:.2e}]")
            assert d <= bar, (name, q)
        nbar = OR.norm_bar(r["chunks"])
        print(f"{name}: norm {r['state']['norm']:.7f} float64 {norm64:.7f} [relative bar {nbar:.2e}]; coef {r['state']['coef']:.8f} float64 {coef64:.8f}")
        assert abs(r["state"]["norm"] - norm64) <= nbar * norm64 and r["state"]["norm"] > 1.0        # clipping is active: coef = scale / norm
        assert any(not torch.equal(x, y) for x, y in zip(r["p"], init))
    one, two = runs["batch 4"], runs["2 x batch 2"]
    gbar = 2 * (2 * toy_config().n_layer + 1) * R.BAR_SCAN[False]
    worst, norm_room = 0.0, 0.0
    for k, ga, gb in zip(one["names"], one["grads"], two["grads"]):
        top = ga.abs().max().item()
        d = (gb.double() * two["scale"] - ga.double()).abs().max().item()
        worst = max(worst, d / top)
        norm_room += ga.numel() * (gbar * top) ** 2
        assert top > 0 and d <= gbar * top, (k, d, top)
    norm_room = norm_room ** 0.5
    na, nb = one["state"]["norm"], two["state"]["norm"]
    nbar = OR.norm_bar(one["chunks"])
    print(f"gradients: worst |scale x accumulated - batch 4| / max |g| over the tensors {worst:.2e} [bar {gbar:.1e}]; norms {na:.7f} / {nb:.7f} "
          f"[room {norm_room + nbar * (na + nb):.2e}]; coef {one['state']['coef']:.8f} / {two['state']['coef']:.8f}")
    assert abs(na - nb) <= norm_room + nbar * (na + nb)
    rel = (norm_room + nbar * (na + nb)) / na + 4 * 2.0 ** -24
    assert abs(two["state"]["coef"] - 0.5 * one["state"]["coef"]) <= rel * 0.5 * one["state"]["coef"]


def write_inputs(tmp):
    from plantcaduceus_amd.checkpoint import save_checkpoint
    data = tmp / "data"
    data.mkdir()
    for split in ("train", "validation"):                           # --do_eval reads the same windows back
        with open(data / f"{split}.tsv", "w") as f:
            f.write("seq\n" + "\n".join(sequences()) + "\n")
    cfgdir = tmp / "cfg"
    save_checkpoint(str(cfgdir), toy_config(), synthetic_state_dict(toy_config(), seed=SEED, stress=False), with_tokenizer=False)
    return str(data), str(cfgdir / "config.json")


def command(data, cfg, out, *extra):
    from plantcaduceus_amd import pretrain
    return pretrain.main(["--config_name", cfg, "--dataset_name", data, "--do_train", "--output_dir", str(out), "--per_device_train_batch_size",
                          str(BATCH), "--learning_rate", str(LR), "--lr_scheduler_type", "constant", "--max_steps", "6", "--logging_steps", "1",
                          "--save_steps", "3", "--seed", str(SEED), "--device", DEV, *extra])


def history(out):
    with open(os.path.join(out, "trainer_state.json")) as f:
        return json.load(f)["log_history"]


def test_resume_from_checkpoint_is_bit_equal_and_the_output_loads(tmp_path):
    from safetensors.torch import load_file
    from transformers import set_seed
    from plantcaduceus_amd import mlm_eval
    from plantcaduceus_amd.modeling_caduceus import CaduceusForMaskedLM
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    data, cfg = write_inputs(tmp_path)
    a, b = tmp_path / "straight", tmp_path / "resumed"
    res = command(data, cfg, a, "--do_eval")
    assert os.path.isdir(a / "checkpoint-3") and os.path.isdir(a / "checkpoint-6")
    for f in ("optimizer.pt", "rng_state.pt", "trainer_state.json", "model.safetensors", "config.json"):
        assert os.path.exists(a / "checkpoint-3" / f), f
    command(data, cfg, b, "--resume_from_checkpoint", str(a / "checkpoint-3"))
    wa, wb = load_file(str(a / "model.safetensors")), load_file(str(b / "model.safetensors"))
    worst = max((wa[k].double() - wb[k].double()).abs().max().item() for k in wa)
    ha, hb = history(a), history(b)
    print(f"resume: max |d parameter| {worst:.3e}; losses straight {[round(e['loss'], 6) for e in ha]} resumed {[round(e['loss'], 6) for e in hb[3:]]}")
    assert set(wa) == set(wb) and all(torch.equal(wa[k], wb[k]) for k in wa)
    assert [e["step"] for e in ha] == [1, 2, 3, 4, 5, 6] and ha[3:] == hb[3:] and hb[:3] == ha[:3]
    with open(a / "train_results.json") as f:
        tr = json.load(f)
    assert tr["train_samples"] == N_WIN and tr["epoch"] == 3.0 and tr["skipped_steps"] == 0 and abs(tr["train_loss"] - np.mean([e["loss"] for e in ha])) < 1e-5
    assert res["train"]["train_loss"] == tr["train_loss"]
    # the output loads: the inference class on the snapshot under evaluate_split, against the trainable model's loss on the same masks.
    # evaluate_split draws its own masks from set_seed(seed) - the final training step's cannot be handed to it - so they are drawn
    # again here the way it draws them (one loss batch of all 8 windows) for the trainable model: once called directly (seed 7), once
    # as the command's own --do_eval wrote it (eval_results.json: --seed 42, the fp32 parity configuration of mlm_eval)
    seqs, tok = sequences(), CaduceusTokenizer()
    eng = CaduceusForMaskedLM.from_pretrained(str(a)).to(F32).to(DEV).eval()
    model = TrainableCaduceusForMaskedLM.from_pretrained(str(a), dtype=F32, device=DEV)
    ids, special, w = mlm_eval.tokenize_windows(tok, seqs, 1.0)
    up = lambda x: torch.from_numpy(np.ascontiguousarray(x)).to(DEV)
    with open(a / "eval_results.json") as f:
        from_command = json.load(f)
    assert res["eval"] == from_command and os.path.exists(a / "all_results.json")
    for tag, seed, ev in (("evaluate_split", 7, mlm_eval.evaluate_split(eng, tok, seqs, "eval", 1.0, 0.15, N_WIN, 7, None, DEV)),
                          ("--do_eval", SEED, from_command)):
        set_seed(seed)
        masked, labels = mlm_eval.mask_windows(mlm_eval.make_collator(tok, 0.15), ids, special, N_WIN)
        with torch.no_grad():
            loss = model(up(masked), up(labels), up(w)).loss.item()
            top = eng(input_ids=up(masked), labels=up(labels), loss_weights=up(w)).logits.abs().max().item()
        bar = 2 * 1e-4 * top
        print(f"output loads ({tag}): eval_loss_token_mean {ev['eval_loss_token_mean']:.7f} trainable loss {loss:.7f} [bar {bar:.3e}, max |logit| {top:.3f}]; "
              f"eval_samples {ev['eval_samples']}")
        assert ev["eval_samples"] == N_WIN and abs(ev["eval_loss_token_mean"] - loss) <= bar and np.isfinite(ev["eval_loss"])


def test_bf16_run(tmp_path):
    from safetensors.torch import load_file
    data, cfg = write_inputs(tmp_path)
    out = tmp_path / "bf16"
    command(data, cfg, out, "--dtype", "bfloat16")
    sd = load_file(str(out / "checkpoint-6" / "model.safetensors"))
    opt = torch.load(str(out / "checkpoint-6" / "optimizer.pt"), weights_only=False)
    hist = history(out)
    print(f"bf16 losses {[round(e['loss'], 5) for e in hist]}")
    assert opt["step"] == 6 and opt["skipped"] == 0 and len(opt["names"]) == len(sd)
    for name, master, m, v in zip(opt["names"], opt["master"], opt["exp_avg"], opt["exp_avg_sq"]):
        assert sd[name].dtype == BF and master.dtype == m.dtype == v.dtype == F32, name
        assert bool(torch.isfinite(master).all()) and bool(torch.isfinite(m).all()) and bool(torch.isfinite(v).all()), name
        assert torch.equal(sd[name], master.to(BF)), name
    assert all(np.isfinite(e["loss"]) for e in hist) and hist[-1]["loss"] < hist[0]["loss"]
