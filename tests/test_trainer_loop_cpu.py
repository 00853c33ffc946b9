"""The trainers' shared loop (iris_amd/utils/trainer.py: Trainer) on the CPU: a two-parameter model under torch's SGD over three fixed batches per epoch,
so every number below is deterministic.  What is pinned is the loop's contract: which steps are logged and with which epoch and learning rate, the
non-finite check, the checkpoint per epoch written by rename, resume as a straight run, and the two checkpoint hooks."""
import argparse
import json
import os

import pytest
import torch

from iris_amd._lib import IrisError
from iris_amd.utils import trainer
from iris_amd.utils.stage import read_checkpoint

BATCHES = torch.tensor([[1.0, -2.0, 0.5], [0.25, 3.0, -1.0], [-0.5, 0.75, 2.0]])
P0, W0, LR = [0.5, -1.0, 2.0], [[0.3, -0.2]], 0.01


class Batches:
    """what the loop asks of a pixel set"""

    def __init__(self):
        self.resamples = 0

    def resample(self):
        self.resamples += 1

    def __len__(self):
        return len(BATCHES)

    def __getitem__(self, i):
        return BATCHES[i]


def loss_of(p, w, batch):
    return ((p * batch).sum() - w.sum()) ** 2 + 0.1 * (w * w).sum()


class PlainToy(trainer.Trainer):
    """the base class's hooks: nothing added to the checkpoint"""
    prefix, logged = "toy", ("loss", "twice")

    def __init__(self, hparams, nan_at=None):
        super().__init__(Batches(), hparams, trainer.PROGRAM_DEFAULTS)
        self.material, self.model_crf = torch.nn.Module(), torch.nn.Module()
        self.material.mlp = torch.nn.Module()
        self.material.mlp.params = torch.nn.Parameter(torch.tensor(P0))
        self.model_crf.weight = torch.nn.Parameter(torch.tensor(W0))
        self.seen = torch.zeros(1)                                              # the steps taken: what Toy adds to the checkpoint
        self.nan_at = nan_at
        self._start([self.material.mlp.params, self.model_crf.weight], networks=[])

    def training_step(self, batch, global_step):
        loss = loss_of(self.material.mlp.params, self.model_crf.weight, batch)
        if global_step == self.nan_at:
            loss = loss * float("nan")
        self.seen = self.seen + 1
        return {"loss": loss, "twice": 2 * loss.detach(), "unlogged": loss.detach()}


class Toy(PlainToy):
    def _extra_state(self):
        return {"seen": self.seen}

    def _load_extra(self, ck, path):
        if "seen" not in ck["emitter"]:
            raise IrisError(f"{path}: no 'emitter.seen'")
        self.seen = ck["emitter"]["seen"].clone()


def hparams(tmp_path, name="exp", **changes):
    return trainer.default_hparams(trainer.PROGRAM_DEFAULTS, experiment_name=name, checkpoint_path=str(tmp_path / "ckpt"), log_path=str(tmp_path / "log"),
                                   optimizer="SGD", learning_rate=LR, milestones=[1], scheduler_rate=0.5, log_every=2, **changes)


def replay(n_epochs):
    """the same six steps by hand: -> [(step, epoch, lr, loss)] of every step, and the final parameters"""
    p, w = torch.tensor(P0, requires_grad=True), torch.tensor(W0, requires_grad=True)
    rows = []
    for epoch in range(n_epochs):
        lr = LR * (0.5 if epoch >= 1 else 1.0)
        for i in range(len(BATCHES)):
            loss = loss_of(p, w, BATCHES[i])
            gp, gw = torch.autograd.grad(loss, (p, w))
            rows.append((len(rows), epoch, lr, float(loss)))
            with torch.no_grad():
                p.add_(gp, alpha=-lr)                                           # (torch's SGD: the product in the precision of add_'s alpha)
                w.add_(gw, alpha=-lr)
    return rows, p.detach(), w.detach()


@pytest.fixture(scope="module")
def straight(tmp_path_factory):
    """fit(2) in one go, with os.replace watched: (trainer, hparams, [(source, target, the epoch the source file holds)])"""
    tmp_path = tmp_path_factory.mktemp("straight")
    renames, replace = [], os.replace

    def watched(src, dst):
        if str(dst).endswith(".ckpt"):
            renames.append((str(src), str(dst), torch.load(src, weights_only=False)["epoch"]))
        replace(src, dst)
    hp = hparams(tmp_path)
    with pytest.MonkeyPatch.context() as mp:
        mp.setattr(os, "replace", watched)
        tr = Toy(hp).fit(2)
    return tr, hp, renames


def test_the_logged_steps_their_epoch_and_learning_rate(straight):
    tr, hp, _ = straight
    rows, p, w = replay(2)
    assert tr.epoch == 2 and tr.global_step == 6 and tr.ps.resamples == 2
    assert torch.equal(tr.material.mlp.params.detach(), p) and torch.equal(tr.model_crf.weight.detach(), w)
    assert [e["step"] for e in tr.history] == [1, 3, 5]                         # log_every 2: the steps after which global_step is 2, 4, 6
    for e in tr.history:
        step, epoch, lr, loss = rows[e["step"]]
        assert set(e) == {"step", "epoch", "lr", "toy/loss", "toy/twice"}
        assert (e["epoch"], e["lr"]) == (epoch, lr) and e["toy/loss"] == pytest.approx(loss, rel=1e-6) and e["toy/twice"] == pytest.approx(2 * loss, rel=1e-6)
    assert [e["epoch"] for e in tr.history] == [0, 1, 1] and [e["lr"] for e in tr.history] == [LR, LR / 2, LR / 2]
    assert all(g["lr"] == LR / 2 for g in tr.optimizer.param_groups)            # the second epoch's rate, in the optimizer's groups
    assert tr.learning_rate(0) == LR and tr.learning_rate(1) == LR / 2 == trainer.multistep_lr(LR, [1], 0.5, 1)
    assert tr.log_file == os.path.join(hp["log_path"], "exp", "metrics.jsonl")
    with open(tr.log_file) as fh:
        assert [json.loads(line) for line in fh] == tr.history


def test_a_non_finite_loss_raises_with_its_step_and_is_not_logged(tmp_path):
    tr = Toy(hparams(tmp_path), nan_at=3)
    with pytest.raises(FloatingPointError, match=r"the loss of step 3 \(epoch 1\) is nan"):
        tr.fit(2)
    assert [e["step"] for e in tr.history] == [1]
    with open(tr.log_file) as fh:
        assert [json.loads(line)["step"] for line in fh] == [1]


def test_the_checkpoint_is_written_per_epoch_by_rename(straight):
    tr, hp, renames = straight
    assert tr.ckpt_file == os.path.join(hp["checkpoint_path"], "exp", "last.ckpt")
    assert renames == [(tr.ckpt_file + ".tmp", tr.ckpt_file, 1), (tr.ckpt_file + ".tmp", tr.ckpt_file, 2)]
    assert os.listdir(os.path.dirname(tr.ckpt_file)) == ["last.ckpt"]
    ck = read_checkpoint(tr.ckpt_file)
    assert ck["epoch"] == 2 and ck["global_step"] == 6 and ck["hyper_parameters"] == hp
    assert set(ck["state_dict"]) == {"material.mlp.params", "model_crf.weight", "emitter.seen"}
    assert torch.equal(ck["material"]["mlp.params"], tr.material.mlp.params.detach()) and torch.equal(ck["emitter"]["seen"], torch.tensor([6.0]))
    assert ck["optimizer_states"] == [tr.optimizer.state_dict()]


def test_resume_continues_as_a_straight_run(straight, tmp_path):
    ref = straight[0]
    hp = hparams(tmp_path)
    first = Toy(hp).fit(1)
    saved = read_checkpoint(first.ckpt_file)
    tr = Toy(dict(hp, resume=True))
    assert tr.epoch == 1 and tr.global_step == 3 and tr.history == []
    assert torch.equal(tr.material.mlp.params, first.material.mlp.params) and torch.equal(tr.model_crf.weight, first.model_crf.weight)
    assert tr.optimizer.state_dict() == saved["optimizer_states"][0] and tr.optimizer.param_groups[0]["lr"] == LR
    assert torch.equal(tr.seen, torch.tensor([3.0]))                            # the subclass's entry, through _extra_state and _load_extra
    tr.fit(2)
    assert tr.epoch == 2 and tr.global_step == 6 and tr.ps.resamples == 1
    assert torch.equal(tr.material.mlp.params, ref.material.mlp.params) and torch.equal(tr.model_crf.weight, ref.model_crf.weight)       # bit for bit
    assert tr.history == ref.history[1:] and torch.equal(tr.seen, ref.seen)
    with open(tr.log_file) as fh:
        assert [json.loads(line) for line in fh] == ref.history
    assert Toy(dict(hp, resume=True)).fit(2).history == []                      # nothing is left to run


def test_resume_without_a_file_and_with_a_file_of_another_stage(tmp_path):
    tr = Toy(hparams(tmp_path, resume=True))
    assert tr.epoch == 0 and tr.global_step == 0 and not os.path.exists(tr.ckpt_file)
    plain = PlainToy(hparams(tmp_path)).fit(1)                                  # the base hooks: no 'emitter.' key is written, none is asked for
    assert set(read_checkpoint(plain.ckpt_file)["state_dict"]) == {"material.mlp.params", "model_crf.weight"}
    assert PlainToy(hparams(tmp_path, resume=True)).epoch == 1
    with pytest.raises(IrisError, match="emitter.seen"):
        Toy(hparams(tmp_path, resume=True))


def test_hyper_parameters_merge_and_unknown_names(tmp_path):
    from iris_amd import train_brdf_crf, train_emitter
    ns = argparse.Namespace(**dict(hparams(tmp_path), emor_path="x", cache_dir="y"))        # a command line's Namespace: what is no hyper-parameter is dropped
    tr = Toy(ns)
    assert tr.hparams == hparams(tmp_path) and set(tr.hparams) == set(trainer.DEFAULT_OPTIONS) | set(trainer.PROGRAM_DEFAULTS)
    assert Toy(trainer.default_hparams(trainer.PROGRAM_DEFAULTS, optimizer="SGD")).ckpt_file is None            # no experiment name: no files
    with pytest.raises(KeyError, match="bogus"):
        trainer.default_hparams(trainer.PROGRAM_DEFAULTS, bogus=1)
    for mod in (train_brdf_crf, train_emitter):
        with pytest.raises(KeyError, match="bogus"):
            mod.default_hparams(bogus=1)
    assert set(train_brdf_crf.default_hparams()) - set(train_emitter.default_hparams()) == {"cache_dir"}
    assert set(train_emitter.default_hparams()) == set(trainer.DEFAULT_OPTIONS) | set(trainer.PROGRAM_DEFAULTS)
    milestones = train_emitter.default_hparams()["milestones"]
    milestones.append(3)                                                        # a copy, not the table's own list
    assert trainer.DEFAULT_OPTIONS["milestones"]["default"] == [1000]
