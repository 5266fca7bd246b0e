"""Child process of tests/test_gpu_lora_dropout_train.py (DESIGN.md §4u on §4r's toy geometry).

    python tests/_lora_dropout_ddp_worker.py OUT ACCUMULATION
    python -m torch.distributed.run --nproc-per-node W tests/_lora_dropout_ddp_worker.py OUT ACCUMULATION

One `lora_predict.FinetuneTrainer.train_step` - optimizer step number 2, so that the step enters the masks' streams - on the toy
fine-tuning model with lora_dropout 0.1 and lora_B = 0.05 N(0, 1), batch 2 and ACCUMULATION x world micro-batches over gloo, then
OUT/r<rank>.pt: the reduced `flat` gradient buffer as the step saw it, the loss, the optimizer's state block and the flat plan."""
import argparse
import os
import sys
from types import SimpleNamespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

N_WIN, L, BATCH, LR, SEED, P, STEP = 16, 69, 2, 1e-3, 42, 0.1, 2


def toy_config():
    from plantcaduceus_amd.checkpoint import make_config
    return make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))


def windows():
    g = np.random.default_rng(13)
    return g.integers(3, 7, size=(N_WIN, L)).astype(np.int32), g.integers(0, 2, size=N_WIN).astype(np.int64)


def main(argv=None):
    p = argparse.ArgumentParser()
    p.add_argument("out")
    p.add_argument("accumulation", type=int)
    w = p.parse_args(argv)
    import torch.distributed as dist
    from plantcaduceus_amd import ddp, lora_predict, optim
    from plantcaduceus_amd.checkpoint import synthetic_state_dict
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification
    device, rank, world = ddp.init_from_env("cuda:0", "gloo")
    cfg = toy_config()
    model = TrainableCaduceusForSequenceClassification(cfg, 2, "single_label_classification", device=device, seed=SEED, lora_dropout=P)
    model.load_trunk({k: v for k, v in synthetic_state_dict(cfg, seed=SEED, stress=False).items() if k.startswith("caduceus.")})
    model.dropout_seed = SEED
    g = torch.Generator().manual_seed(31)
    with torch.no_grad():
        for k, q in model.named_parameters():
            if ".lora_B." in k:
                q.copy_((torch.randn(q.shape, generator=g) * 0.05).to(device))
    ids, labels = windows()
    source = lora_predict.LabelledBatches(ids, labels, BATCH, w.accumulation * world, SEED)
    reducer = ddp.GradReducer(dist.group.WORLD if ddp.active() else None, device)
    opt = optim.AdamW(model.named_parameters(), lr=LR, weight_decay=0.01, reducer=reducer)
    a = SimpleNamespace(output_dir=w.out, model_name=None, task_type="classification", device=device, learning_rate=LR, lr_scheduler_type="constant",
                        warmup_steps=0, eval_batch_size=4, eval_strategy="no", eval_steps=0, save_strategy="no", save_steps=0, logging_steps=1)
    tr = lora_predict.FinetuneTrainer(model.train(), opt, source, a, STEP + 1, None, rank, world)
    tr.step = STEP
    tr.train_step()
    torch.cuda.synchronize(device)
    offsets, total = opt.table().flat_plan()
    torch.save({"rank": rank, "world": world, "flat": reducer.grads.cpu(), "loss": float(reducer.loss), "state": opt.state(), "offsets": offsets,
                "names": opt.names, "sizes": [q.numel() for q in opt.params], "scale": opt.grad_scale, "dropout_step": model.dropout_step},
               os.path.join(w.out, f"r{rank}.pt"))
    ddp.shutdown()


if __name__ == "__main__":
    main()
