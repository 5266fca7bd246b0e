"""Child process of tests/test_gpu_main_grad.py, beside tests/_ddp_worker.py whose toy inputs it shares.

    python tests/_main_grad_worker.py OUT ACCUMULATION [--backend gloo|nccl]
    python -m torch.distributed.run --nproc-per-node W tests/_main_grad_worker.py OUT ACCUMULATION ...

One `pretrain.Trainer.train_step` on a fresh bf16 toy model through `optim.AdamW(reducer=..., fp32_grad_accumulation=True)`, batch 2 and
ACCUMULATION x world micro-batches, then OUT/r<rank>.pt: the reducer's flat buffer as the step saw it (taken just before zero_grad, which
zeroes it), the optimizer's state block, this rank's checksum of the master weights and the layout.  Plain `python`: world 1, no group."""
import argparse
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for path in (ROOT, os.path.join(ROOT, "tests")):
    if path not in sys.path:
        sys.path.insert(0, path)

import _ddp_worker as W  # noqa: E402


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("accumulation", type=int)
    p.add_argument("--backend", default="gloo")
    w = p.parse_args(argv)
    import torch.distributed as dist
    from plantcaduceus_amd import ddp, mlm_eval, ops, optim, pretrain
    from plantcaduceus_amd.checkpoint import synthetic_state_dict
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    device, rank, world = ddp.init_from_env("cuda:0", w.backend)
    cfg = W.toy_config()
    model = TrainableCaduceusForMaskedLM(cfg, dtype=torch.bfloat16, device=device)
    model.load_state_dict(synthetic_state_dict(cfg, seed=W.SEED, stress=False))
    tok = CaduceusTokenizer()
    ids, special, weights = mlm_eval.tokenize_windows(tok, W.sequences(), 1.0)
    source = pretrain.BatchSource(ids, special, weights, mlm_eval.make_collator(tok, 0.15), W.BATCH, w.accumulation * world, W.SEED)
    reducer = ddp.GradReducer(dist.group.WORLD if ddp.active() else None, device)
    opt = optim.AdamW(model.named_parameters(), lr=W.LR, weight_decay=0.1, reducer=reducer, fp32_grad_accumulation=True)
    assert opt.flat.data_ptr() == reducer.grads.data_ptr()                     # the reducer's own buffer, no second one
    a = pretrain.build_parser().parse_args(["--dataset_name", "-", "--output_dir", w.out, "--learning_rate", str(W.LR), "--lr_scheduler_type",
                                            "constant", "--device", device])
    tr = pretrain.Trainer(model, opt, source, tok, a, 1, 0, rank, world)
    seen, gathers, zero = {}, [], opt.zero_grad

    def keep_then_zero():
        seen["flat"] = reducer.grads.detach().cpu().clone()
        zero()
    opt.zero_grad = keep_then_zero
    gather = ops.grads_gather
    ops.grads_gather = lambda *args, **kw: (gathers.append(1), gather(*args, **kw))[1]
    before = [p.detach().clone() for p in opt.params]
    try:
        tr.train_step()
    finally:
        ops.grads_gather = gather                                               # world 1 runs inside the test's own process
    torch.cuda.synchronize(device)
    offsets, total = ops.grads_flat_plan(opt.table().records)
    torch.save({"rank": rank, "world": world, "flat": seen["flat"], "flat_after": reducer.grads.cpu(), "loss": float(reducer.loss), "state": opt.state(),
                "checksum": int(ddp.checksum(tr.masters())), "changed": any(not torch.equal(x, y) for x, y in zip(opt.params, before)),
                "offsets": offsets, "total": total, "names": opt.names, "sizes": [p.numel() for p in opt.params], "scale": opt.grad_scale,
                "gathers": len(gathers), "grads_left": sum(p.grad is not None for p in opt.params),
                "rounded": all(torch.equal(p, m.to(p.dtype)) for p, m in zip(opt.params, opt.master))},
               os.path.join(w.out, f"r{rank}.pt"))
    ddp.shutdown()


if __name__ == "__main__":
    main()
