"""Child process of tests/test_gpu_ddp.py, and the toy inputs it shares with it (DESIGN.md §4o's toy geometry: n_layer 2, d_model 64,
d_inner 128, dt_rank 4; 8 windows of L = 69).

    python tests/_ddp_worker.py OUT ACCUMULATION [--backend gloo|nccl] [--dtype float32|bfloat16] [--inf_rank R]
    python -m torch.distributed.run --nproc-per-node W tests/_ddp_worker.py OUT ACCUMULATION ...

One `pretrain.Trainer.train_step` on a fresh toy model through `optim.AdamW(reducer=ddp.GradReducer(...))`, batch 2 and
ACCUMULATION x world micro-batches, then OUT/r<rank>.pt: the reduced `flat` buffer as the step saw it, the optimizer's state block, this
rank's checksum of the master weights, whether any parameter changed, and the flat plan.  --inf_rank R: rank R writes one inf into its
first gradient after its backward.  Plain `python`: world 1, no group (GradReducer(None, ...))."""
import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_WIN, L, BATCH, LR, SEED = 8, 69, 2, 1e-3, 42


def toy_config():
    from plantcaduceus_amd.checkpoint import make_config
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def sequences():
    g = np.random.default_rng(9)
    return ["".join(g.choice(list("ACGTacgt"), size=L)) for _ in range(N_WIN)]


def write_inputs(tmp):
    """-> (dataset directory with train.tsv / validation.tsv, config.json) under tmp"""
    from plantcaduceus_amd.checkpoint import save_checkpoint, synthetic_state_dict
    data = tmp / "data"
    data.mkdir()
    for split in ("train", "validation"):
        with open(data / f"{split}.tsv", "w") as f:
            f.write("seq\n" + "\n".join(sequences()) + "\n")
    save_checkpoint(str(tmp / "cfg"), toy_config(), synthetic_state_dict(toy_config(), seed=SEED, stress=False), with_tokenizer=False)
    return str(data), str(tmp / "cfg" / "config.json")


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("accumulation", type=int)
    p.add_argument("--backend", default="gloo")
    p.add_argument("--dtype", default="float32")
    p.add_argument("--inf_rank", type=int, default=-1)
    w = p.parse_args(argv)
    import torch.distributed as dist
    from plantcaduceus_amd import ddp, mlm_eval, optim, pretrain
    from plantcaduceus_amd.checkpoint import synthetic_state_dict
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    device, rank, world = ddp.init_from_env("cuda:0", w.backend)
    dtype = {"float32": torch.float32, "bfloat16": torch.bfloat16}[w.dtype]
    cfg = toy_config()
    model = TrainableCaduceusForMaskedLM(cfg, dtype=dtype, device=device)
    model.load_state_dict(synthetic_state_dict(cfg, seed=SEED, stress=False))
    tok = CaduceusTokenizer()
    ids, special, weights = mlm_eval.tokenize_windows(tok, sequences(), 1.0)
    source = pretrain.BatchSource(ids, special, weights, mlm_eval.make_collator(tok, 0.15), BATCH, w.accumulation * world, SEED)
    reducer = ddp.GradReducer(dist.group.WORLD if ddp.active() else None, device)
    opt = optim.AdamW(model.named_parameters(), lr=LR, weight_decay=0.1, reducer=reducer)
    a = pretrain.build_parser().parse_args(["--dataset_name", "-", "--output_dir", w.out, "--learning_rate", str(LR), "--lr_scheduler_type",
                                            "constant", "--device", device])
    tr = pretrain.Trainer(model, opt, source, tok, a, 1, 0, rank, world)
    if rank == w.inf_rank:
        micro = tr.micro_step

        def poisoned(*args):
            loss = micro(*args)
            opt.params[0].grad.view(-1)[0] = float("inf")
            return loss
        tr.micro_step = poisoned
    before = [p.detach().clone() for p in opt.params]
    tr.train_step()
    torch.cuda.synchronize(device)
    offsets, total = opt.table().flat_plan()
    torch.save({"rank": rank, "world": world, "flat": reducer.grads.cpu(), "loss": float(reducer.loss), "state": opt.state(),
                "checksum": int(ddp.checksum(tr.masters())), "changed": any(not torch.equal(x, y) for x, y in zip(opt.params, before)),
                "offsets": offsets, "total": total, "chunks": opt.table().chunks, "names": opt.names, "sizes": [p.numel() for p in opt.params], "scale": opt.grad_scale,
                "rounded": all(m is None or torch.equal(p, m.to(p.dtype)) for p, m in zip(opt.params, opt.master))},
               os.path.join(w.out, f"r{rank}.pt"))
    ddp.shutdown()


if __name__ == "__main__":
    main()
