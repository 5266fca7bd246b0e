"""CPU checks of evaluation during pretraining and of validation sharded over the ranks (the GPU half is
tests/test_gpu_train_eval.py): the new flags against the installed `transformers.TrainingArguments`, the reference README's pretraining
command line, the refusals; which steps evaluate and save; `pretrain.rotate_checkpoints` on fake checkpoint directories;
`pretrain.BestCheckpoint` and the loop's rule that only a saved step is offered; `sharding.batch_block` as a partition of the
single-process loss batches and `sharding.gather_batch_rows` over gloo at worlds 2 and 3; the validation masks of a private generator."""
import dataclasses
import json
import os
import socket

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

from plantcaduceus_amd import pretrain, sharding

BASE = ["--dataset_name", "d", "--output_dir", "o"]


def parse(*extra):
    return pretrain.build_parser().parse_args(BASE + list(extra))


# ---- the parser -------------------------------------------------------------------------------------------------------------------
def test_new_flags_keep_training_arguments_names_and_defaults():
    from transformers import TrainingArguments
    a = parse()
    want = dict(eval_strategy="no", eval_steps=None, save_strategy="steps", save_total_limit=None, load_best_model_at_end=False,
                metric_for_best_model=None, prediction_loss_only=False)
    ta = {f.name: f.default for f in dataclasses.fields(TrainingArguments)}
    for k, v in want.items():
        assert getattr(a, k) == v, k
        assert k in ta and str(getattr(ta[k], "value", ta[k])) == str(v), (k, ta.get(k))
    assert parse("--evaluation_strategy", "epoch").eval_strategy == parse("--eval_strategy", "epoch").eval_strategy == "epoch"
    assert not hasattr(a, "evaluation_strategy")
    assert parse("--eval_steps", "7").eval_steps == 7 and parse("--eval_steps", "7.0").eval_steps == 7
    for flag in ("--load_best_model_at_end", "--prediction_loss_only"):
        dest = flag[2:]
        assert getattr(parse("--eval_strategy", "steps", "--logging_steps", "500", flag), dest) is True
        assert getattr(parse("--eval_strategy", "steps", flag, "True"), dest) is True
        assert getattr(parse(flag, "False"), dest) is False
    assert all(getattr(a, k) is None for k in pretrain.IGNORED_FLAGS)


# the reference README's "Pre-training PlantCAD" command, as printed but for: --report_to wandb dropped, and the two soft-mask flags
# spelt as HF_pre_train.py itself spells them (weights, not weight)
README_COMMAND = """--do_train --prediction_loss_only True --remove_unused_columns False --dataset_name kuleshov-group/Angiosperm_16_genomes
    --soft_masked_loss_weights_train 0.1 --soft_masked_loss_weights_evaluation 0.0 --weight_decay 0.01 --optim adamw_torch
    --dataloader_num_workers 16 --preprocessing_num_workers 16 --seed 32 --save_strategy steps --save_steps 1000
    --evaluation_strategy steps --eval_steps 1000 --logging_steps 10 --max_steps 120000 --warmup_steps 1000 --save_total_limit 20
    --learning_rate 2E-4 --lr_scheduler_type constant_with_warmup --run_name test --overwrite_output_dir
    --output_dir PlantCaduceus_train_1 --per_device_train_batch_size 32 --per_device_eval_batch_size 32 --gradient_accumulation_steps 4
    --tokenizer_name kuleshov-group/PlantCaduceus_l20 --config_name kuleshov-group/PlantCaduceus_l20""".split()


def test_the_readme_command_line_parses():
    a = pretrain.build_parser().parse_args(README_COMMAND)
    assert a.do_train and a.prediction_loss_only is True and a.remove_unused_columns is False and a.overwrite_output_dir is True
    assert (a.eval_strategy, a.eval_steps, a.save_strategy, a.save_steps, a.save_total_limit) == ("steps", 1000, "steps", 1000, 20)
    assert (a.soft_masked_loss_weights_train, a.soft_masked_loss_weights_evaluation, a.seed, a.max_steps) == (0.1, 0.0, 32, 120000)
    assert (a.optim, a.run_name, a.dataloader_num_workers, a.preprocessing_num_workers, a.report_to) == ("adamw_torch", "test", 16, 16, None)
    assert a.output_dir == "PlantCaduceus_train_1" and a.per_device_eval_batch_size == 32 and a.learning_rate == 2e-4
    assert pretrain.eval_interval(a, 77) == 1000 and pretrain.save_interval(a, 77) == 1000


@pytest.mark.parametrize("argv,flags", [
    (["--report_to", "wandb"], ["--report_to"]),
    (["--optim", "adafactor"], ["--optim"]),
    (["--eval_steps", "0.1"], ["--eval_steps"]),
    (["--eval_steps", "0"], ["--eval_steps"]),
    (["--metric_for_best_model", "accuracy"], ["--metric_for_best_model"]),
    (["--load_best_model_at_end", "--eval_steps", "2", "--save_steps", "3"], ["--eval_steps", "--save_steps"]),
    (["--load_best_model_at_end", "--eval_strategy", "steps", "--eval_steps", "2", "--save_steps", "3"], ["--eval_steps", "--save_steps"]),
    (["--load_best_model_at_end", "--eval_strategy", "steps", "--eval_steps", "2", "--save_steps", "0"], ["--eval_steps", "--save_steps"]),
    (["--load_best_model_at_end", "--eval_steps", "2", "--save_steps", "4"], ["--load_best_model_at_end", "--eval_strategy"]),
    (["--load_best_model_at_end", "--eval_strategy", "epoch"], ["--eval_strategy", "--save_strategy"]),
    (["--load_best_model_at_end", "--eval_strategy", "steps", "--save_strategy", "no", "--logging_steps", "5"], ["--eval_strategy", "--save_strategy"]),
])
def test_refusals_name_their_flags(argv, flags):
    with pytest.raises(SystemExit) as ex:
        parse(*argv)
    for f in flags:
        assert f in str(ex.value), (f, str(ex.value))


def test_accepted_combinations():
    assert parse("--report_to", "none", "--optim", "adamw_torch", "--metric_for_best_model", "eval_loss").metric_for_best_model == "eval_loss"
    assert parse("--load_best_model_at_end", "--eval_strategy", "steps", "--eval_steps", "2", "--save_steps", "4").load_best_model_at_end
    assert parse("--load_best_model_at_end", "--eval_strategy", "epoch", "--save_strategy", "epoch").load_best_model_at_end
    assert parse("--load_best_model_at_end", "--eval_strategy", "steps").load_best_model_at_end      # 500 and 500: logging_steps is eval_steps


# ---- which steps are due ------------------------------------------------------------------------------------------------------------
def test_due_steps():
    per_epoch, last = 4, 12
    ev = lambda *extra: pretrain.due_steps(pretrain.eval_interval(parse(*extra), per_epoch), last)
    sv = lambda *extra: pretrain.due_steps(pretrain.save_interval(parse(*extra), per_epoch), last)
    assert ev("--eval_strategy", "steps", "--eval_steps", "3") == [3, 6, 9, 12]
    assert ev("--eval_strategy", "epoch") == ev("--eval_strategy", "epoch", "--eval_steps", "3") == [4, 8, 12]
    assert ev("--eval_strategy", "no", "--eval_steps", "3") == ev() == []
    assert ev("--eval_strategy", "steps", "--logging_steps", "5") == [5, 10]                 # eval_steps unset follows logging_steps
    assert ev("--eval_strategy", "steps", "--logging_steps", "5", "--eval_steps", "6") == [6, 12]
    assert sv("--save_steps", "6") == [6, 12] and sv("--save_steps", "0") == [] and sv("--save_strategy", "no", "--save_steps", "6") == []
    assert sv("--save_strategy", "epoch", "--save_steps", "6") == [4, 8, 12]
    with pytest.raises(SystemExit, match="--eval_strategy"):
        pretrain.interval("sometimes", 1, 1, "eval_strategy")


# ---- rotation ---------------------------------------------------------------------------------------------------------------------
def _checkpoints(tmp, steps):
    for s in steps:
        d = tmp / f"checkpoint-{s}"
        d.mkdir()
        (d / "model.safetensors").write_bytes(b"x")
    (tmp / "checkpoint-notes").mkdir()                                      # not a checkpoint: left alone
    (tmp / "trainer_state.json").write_text("{}")
    return str(tmp)


def _left(out):
    return sorted(int(os.path.basename(d).split("-")[1]) for d in pretrain.checkpoint_dirs(out))


@pytest.mark.parametrize("limit,best,left", [(2, None, [4, 6]), (2, 2, [2, 6]), (1, 2, [2, 6]), (1, 6, [6]), (None, None, [2, 4, 6]),
                                             (None, 2, [2, 4, 6]), (2, 4, [4, 6]), (3, 2, [2, 4, 6]), (1, None, [6]), (5, None, [2, 4, 6])])
def test_rotation(tmp_path, limit, best, left):
    out = _checkpoints(tmp_path, (2, 4, 6))
    gone = pretrain.rotate_checkpoints(out, limit, None if best is None else os.path.join(out, f"checkpoint-{best}"))
    assert _left(out) == left and sorted(int(g.rsplit("-", 1)[1]) for g in gone) == sorted({2, 4, 6} - set(left))
    assert os.path.isdir(tmp_path / "checkpoint-notes") and os.path.exists(tmp_path / "trainer_state.json")


def test_rotation_orders_by_step_not_by_name_and_ignores_a_best_elsewhere(tmp_path):
    out = _checkpoints(tmp_path, (8, 9, 10, 100))
    pretrain.rotate_checkpoints(out, 2, str(tmp_path / "elsewhere" / "checkpoint-8"))
    assert _left(out) == [10, 100]
    assert pretrain.rotate_checkpoints(str(tmp_path / "missing"), 2) == []


def test_lora_train_rotates_with_the_same_function(tmp_path, monkeypatch):
    """FinetuneTrainer.save_checkpoint keeps the newest SAVE_TOTAL_LIMIT through pretrain.rotate_checkpoints"""
    from types import SimpleNamespace
    from plantcaduceus_amd import lora_predict
    out = _checkpoints(tmp_path, (1, 2, 3, 4, 5, 6))
    calls = []
    real = pretrain.rotate_checkpoints
    monkeypatch.setattr(pretrain, "rotate_checkpoints", lambda *a, **k: calls.append(a) or real(*a, **k))
    monkeypatch.setattr(torch, "save", lambda obj, path: None)
    tr = lora_predict.FinetuneTrainer.__new__(lora_predict.FinetuneTrainer)
    tr.a = SimpleNamespace(output_dir=out, model_name="base")
    tr.step = 7
    tr.model = SimpleNamespace(save_adapter=lambda path, name: os.makedirs(path))
    tr.opt = SimpleNamespace(state_dict=lambda: {})
    tr.trainer_state = lambda: {}
    assert tr.save_checkpoint() == os.path.join(out, "checkpoint-7")
    assert calls == [(out, lora_predict.SAVE_TOTAL_LIMIT)] and _left(out) == [3, 4, 5, 6, 7]


# ---- the best checkpoint ------------------------------------------------------------------------------------------------------------
def test_best_checkpoint_bookkeeping():
    best = pretrain.BestCheckpoint()
    assert best.state() == {"best_metric": None, "best_global_step": 0, "best_model_checkpoint": None}
    taken = [best.offer(loss, step, f"o/checkpoint-{step}") for step, loss in enumerate((0.9, float("nan"), 0.7, 0.8), start=1)]
    assert taken == [True, False, True, False]
    assert best.state() == {"best_metric": 0.7, "best_global_step": 3, "best_model_checkpoint": "o/checkpoint-3"}
    assert not best.offer(0.7, 5, "o/checkpoint-5") and best.step == 3           # a tie keeps the earlier one
    again = pretrain.BestCheckpoint()
    again.load_state({"global_step": 4})                                         # a trainer_state.json from before: nothing yet
    assert again.state() == pretrain.BestCheckpoint().state()
    again.load_state(best.state())
    assert again.state() == best.state()
    only_nan = pretrain.BestCheckpoint()
    assert not only_nan.offer(float("nan"), 1, "p") and only_nan.path is None


class LoopOnly(pretrain.Trainer):
    """pretrain.Trainer.run with the device work replaced: the order of log, evaluate and save, and what is offered as the best"""

    def __init__(self, a, losses, max_steps):
        source = type("Source", (), {"steps_per_epoch": 4})()
        super().__init__(None, None, source, None, a, max_steps, 0, valid=object())
        self.losses, self.events = losses, []

    def train_step(self):
        self.step += 1
        return 0.0

    def log(self, lr):
        self.events.append(("log", self.step))

    def evaluate(self):
        self.events.append(("eval", self.step))
        self.log_history.append({"eval_loss": self.losses[self.step], "step": self.step})
        return {"eval_loss": self.losses[self.step]}

    def checkpoint(self):
        self.events.append(("save", self.step))
        self.saved = getattr(self, "saved", []) + [json.loads(json.dumps(self.trainer_state()))]     # as the file would hold it


def test_only_an_evaluation_at_a_saved_step_becomes_the_best():
    a = parse("--device", "cpu", "--logging_steps", "1", "--eval_strategy", "steps", "--eval_steps", "1", "--save_steps", "2")
    losses = {1: 0.1, 2: 0.9, 3: 0.05, 4: float("nan"), 5: 0.2, 6: 0.8}        # the lowest are at unsaved steps
    tr = LoopOnly(a, losses, 6)
    tr.run()
    assert tr.best.state() == {"best_metric": 0.8, "best_global_step": 6, "best_model_checkpoint": os.path.join("o", "checkpoint-6")}
    assert tr.events[:3] == [("log", 1), ("eval", 1), ("log", 2)] and tr.events[3:5] == [("eval", 2), ("save", 2)]      # log, evaluate, save
    # the checkpoint written at an evaluated step holds that evaluation and the best so far
    first, second = tr.saved[0], tr.saved[1]
    assert first["log_history"][-1] == {"eval_loss": 0.9, "step": 2} and first["best_global_step"] == 2 and first["best_metric"] == 0.9
    assert second["best_global_step"] == 2 and second["global_step"] == 4       # nan at step 4: never the best
    # without a validation set nothing is evaluated, whatever the flags say
    quiet = LoopOnly(a, losses, 4)
    quiet.valid = None
    quiet.run()
    assert [e for e in quiet.events if e[0] == "eval"] == [] and quiet.best.path is None


def test_load_best_model_puts_the_checkpoints_weights_back(tmp_path):
    """the model at "step 2" is saved, moves on, and load_best_model brings back exactly what the checkpoint holds; tied weights stay tied"""
    from safetensors.torch import load_file
    from plantcaduceus_amd.checkpoint import make_config, synthetic_state_dict
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    from plantcaduceus_amd.training import TrainableCaduceusForMaskedLM
    cfg = make_config("toy", d_model=64, n_layer=2, ssm_cfg=dict(d_state=16, d_conv=4, expand=2, dt_rank=4, bias=False, conv_bias=True))
    model = TrainableCaduceusForMaskedLM(cfg, device="cpu")
    model.load_state_dict(synthetic_state_dict(cfg, seed=3, stress=False))
    ckpt, out = str(tmp_path / "checkpoint-2"), str(tmp_path / "out")
    pretrain.save_snapshot(model, CaduceusTokenizer(), ckpt)
    with torch.no_grad():
        for p in model.parameters():
            p.add_(0.5)                                                          # the later steps
    best = pretrain.BestCheckpoint()
    assert not pretrain.load_best_model(model, best)                             # no evaluation at a saved step: the last model stays
    moved = {k: v.clone() for k, v in model.state_dict().items()}
    best.offer(0.7, 2, ckpt)
    assert pretrain.load_best_model(model, best)
    pretrain.save_snapshot(model, CaduceusTokenizer(), out)
    a, b = load_file(os.path.join(ckpt, "model.safetensors")), load_file(os.path.join(out, "model.safetensors"))
    assert set(a) == set(b) and all(torch.equal(a[k], b[k]) for k in a)
    assert any(not torch.equal(moved[k], v) for k, v in model.state_dict().items())
    emb = model.caduceus.backbone.embeddings.word_embeddings.embedding.weight
    assert model.lm_head.lm_head.weight is emb and all(p.requires_grad for p in model.parameters())


# ---- the batch-block rule -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [0, 1, 5, 7, 8])
@pytest.mark.parametrize("batch", [1, 2, 3])
@pytest.mark.parametrize("world", [1, 2, 3, 4])
def test_the_ranks_blocks_partition_the_single_process_batches(n, batch, world):
    single = [(b0, min(b0 + batch, n)) for b0 in range(0, n, batch)]
    dealt, per_rank = [], set()
    for r in range(world):
        lo, hi, per = sharding.batch_block(n, batch, r, world)
        per_rank.add(per)
        mine = [(b0, min(b0 + batch, hi)) for b0 in range(lo, hi, batch)]
        assert hi - lo <= per and (hi - lo == per or hi == n)                   # full, or the one that holds the end, or empty
        assert len(mine) <= -(-len(single) // world) if single else not mine
        dealt += mine
    assert dealt == single and len(per_rank) == 1
    assert per_rank.pop() == -(-len(single) // world) * batch


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


WIDTH = 4
CASES = [(n, batch) for n in (0, 1, 5, 7, 8) for batch in (1, 2, 3)]


def _rows(n):
    return torch.randn(n, WIDTH, generator=torch.Generator().manual_seed(50 + n))


def _stand_in(data, calls=None):
    """a forward that is a function of the rows it is given: every row's output depends on the whole batch it came in"""
    def run(lo, hi):
        if calls is not None:
            calls.append((lo, hi))
        x = data[lo:hi]
        return x * x.sum() + x.mean(0)
    return run


def _gather_worker(rank, ws, port, outdir):
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port))
    dist.init_process_group("gloo", rank=rank, world_size=ws)
    try:
        torch.set_num_threads(1)
        out = {}
        for n, batch in CASES:
            calls = []
            got = sharding.gather_batch_rows(n, batch, _stand_in(_rows(n), calls), WIDTH, "cpu")
            out[(n, batch)] = (got, calls)
        torch.save(out, os.path.join(outdir, f"r{rank}.pt"))
    finally:
        dist.destroy_process_group()


@pytest.mark.parametrize("ws", [2, 3])
def test_gathered_rows_equal_the_one_process_array(tmp_path, ws):
    assert not dist.is_initialized()
    mp.spawn(_gather_worker, args=(ws, _free_port(), str(tmp_path)), nprocs=ws, join=True)
    got = [torch.load(tmp_path / f"r{r}.pt") for r in range(ws)]
    empty = 0
    for n, batch in CASES:
        one = sharding.gather_batch_rows(n, batch, _stand_in(_rows(n)), WIDTH, "cpu")       # no group here: every batch
        assert one.shape == (n, WIDTH) and one.dtype == torch.float32
        calls = []
        for r in range(ws):
            rows, mine = got[r][(n, batch)]
            assert rows.shape == one.shape and torch.equal(rows, one), (n, batch, r)       # exactly, on every rank
            empty += not mine
            calls += mine
        assert calls == [(b0, min(b0 + batch, n)) for b0 in range(0, n, batch)]             # every forward saw a single-process batch
    assert empty > 0                                                                        # ranks without a batch took part


# ---- the validation masks -------------------------------------------------------------------------------------------------------------
def _toy_sequences(n=8, L=69):
    g = np.random.default_rng(9)                                                            # tests/test_gpu_pretrain.py's windows
    return ["".join(g.choice(list("ACGTacgt"), size=L)) for _ in range(n)]


@pytest.mark.parametrize("batch", [2, 3, 8])
def test_private_generator_masks_are_evaluate_splits_and_touch_nothing_global(batch):
    from transformers import set_seed
    from plantcaduceus_amd import mlm_eval
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    tok, seqs, seed = CaduceusTokenizer(), _toy_sequences(), 42
    torch.manual_seed(1234)
    before = torch.get_rng_state()
    valid = pretrain.ValidationSet.build(tok, seqs, 0.25, 0.15, batch, seed)
    again = pretrain.ValidationSet.build(tok, seqs, 0.25, 0.15, batch, seed)
    assert torch.equal(torch.get_rng_state(), before)
    # evaluate_split's own draw: set_seed(seed), then mask_windows on the global generator
    ids, special, w = mlm_eval.tokenize_windows(tok, seqs, 0.25)
    set_seed(seed)
    masked, labels = mlm_eval.mask_windows(mlm_eval.make_collator(tok, 0.15), ids, special, batch)
    assert np.array_equal(valid.ids, masked) and np.array_equal(valid.labels, labels) and np.array_equal(valid.weights, w)
    assert np.array_equal(again.ids, valid.ids) and np.array_equal(again.labels, valid.labels)
    assert valid.n == 8 and valid.batch_size == batch and valid.ids.dtype == np.int32 and valid.labels.dtype == np.int32
    assert ((valid.labels != -100).sum(1) > 0).all() and not np.array_equal(valid.ids, ids)
    other = pretrain.ValidationSet.build(tok, seqs, 0.25, 0.15, batch, seed + 1)
    assert not np.array_equal(other.labels, valid.labels)
    assert pretrain.ValidationSet.build(tok, seqs, 1.0, 0.15, batch, seed, max_samples=5).n == 5


def test_a_missing_validation_split_names_the_flag_and_the_split(tmp_path):
    from plantcaduceus_amd.tokenization_caduceus import CaduceusTokenizer
    (tmp_path / "train.tsv").write_text("seq\nACGT\n")
    a = pretrain.build_parser().parse_args(["--dataset_name", str(tmp_path), "--output_dir", "o", "--eval_strategy", "steps"])
    with pytest.raises(SystemExit) as ex:
        pretrain.load_validation(a, CaduceusTokenizer())
    assert "--eval_strategy" in str(ex.value) and "validation" in str(ex.value)
