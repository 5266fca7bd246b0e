"""Child process of tests/test_gpu_feature_train.py.

    python -m torch.distributed.run --nproc-per-node W tests/_feature_train_worker.py SIDE <lora_predict train arguments>

Runs `lora_predict.main(["train", ...])` as the rank it is started as - the parent sets PCAD_TRAIN_FEATURES, PCAD_TRAIN_FEATURE_BATCH and
PCAD_DDP_BACKEND in the environment - with counters around everything the command writes with, and leaves SIDE/r<rank>.json: how many
windows this rank sent through the engine, how many engines it built and how many files it wrote."""
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def counted(counts):
    """patch counters into the package -> a function that undoes them"""
    import torch
    from plantcaduceus_amd import engine, pretrain
    from plantcaduceus_amd.training import TrainableCaduceusForSequenceClassification as Model
    saved = (engine.Engine.__init__, engine.Engine.forward_pooled, pretrain._write_json, Model.save_adapter, torch.save)

    def init(self, *a, **k):
        counts["engines"] += 1
        return saved[0](self, *a, **k)

    def forward_pooled(self, input_ids, *a, **k):
        counts["windows"] += int(input_ids.shape[0])
        return saved[1](self, input_ids, *a, **k)

    def write_json(*a, **k):
        counts["writes"] += 1
        return saved[2](*a, **k)

    def save_adapter(self, *a, **k):
        counts["writes"] += 1
        return saved[3](self, *a, **k)

    def save(*a, **k):
        counts["writes"] += 1
        return saved[4](*a, **k)
    engine.Engine.__init__, engine.Engine.forward_pooled, pretrain._write_json, Model.save_adapter, torch.save = init, forward_pooled, write_json, save_adapter, save

    def undo():
        engine.Engine.__init__, engine.Engine.forward_pooled, pretrain._write_json, Model.save_adapter, torch.save = saved
    return undo


def main(argv=None):
    argv = list(sys.argv[1:] if argv is None else argv)
    side, args = argv[0], argv[1:]
    from plantcaduceus_amd import lora_predict
    counts = {"engines": 0, "windows": 0, "writes": 0}
    undo = counted(counts)
    try:
        lora_predict.main(["train"] + args)
    finally:
        undo()
    with open(os.path.join(side, f"r{int(os.environ.get('RANK', '0'))}.json"), "w") as f:
        json.dump(counts, f)


if __name__ == "__main__":
    main()
