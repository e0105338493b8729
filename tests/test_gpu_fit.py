"""-m gpu: fit() end to end (fastegnn_amd/checkpoint.py) -- training N epochs in one go, and training k epochs, saving, loading into
fresh objects and training N - k more, give the same bits.

On the wide path (hidden_nf = 128) with ``deterministic = True`` every sum of a training step is ordered, the loss included
(fastegnn_loss_mse_mmd_ordered), so two runs of one seed agree bit for bit -- the promise of the mode -- and so does a resumed run:
parameters, moments, step counts, the sampler's counter, the stream's state and the logged losses.  On the fused path (hidden_nf = 64)
the virtual pools still sum with atomics, so there only the restored state is compared, and the next batch and sample drawn."""
import json

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import data as D
from fastegnn_amd.checkpoint import load_checkpoint
from fastegnn_amd.train import FusedAdam, MMDSampler
from tests.packed_ref import make_frame

pytestmark = pytest.mark.gpu

SIGMA, WEIGHT, NUM_SAMPLE, EPOCHS = 1.0, 0.01, 3, 4


@pytest.fixture(scope="module")
def packed():
    """8 complete graphs of 5 nodes (20 edges)"""
    gen = torch.Generator().manual_seed(5)
    ij = torch.tensor([(i, j) for i in range(5) for j in range(5) if i != j], dtype=torch.int64).t().contiguous()
    frames = []
    for _ in range(8):
        f = make_frame(5, 20, 3, 1, gen)
        f.edge_index = ij
        f.edge_attr = (f.loc_0[ij[0]] - f.loc_0[ij[1]]).norm(dim=1, keepdim=True)
        frames.append(f)
    return D.PackedDataset(frames, device="cuda")


class _Run:
    """fresh objects of one run: the model from `model_seed` (a resumed run takes ANOTHER seed: everything must come from the file)"""

    def __init__(self, packed, hidden_nf, model_seed=11, other=False):
        torch.manual_seed(model_seed)
        self.model = fastegnn_amd.FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2, hidden_nf=hidden_nf, virtual_channels=3,
                                           device="cuda", n_layers=2)
        self.model.deterministic = True
        self.opt = FusedAdam(self.model.parameters(), lr=9e-1 if other else 5e-4, weight_decay=1e-12, capturable=True)
        self.sampler = MMDSampler(77 if other else 3)
        graphs = None if hidden_nf > 64 else self.model.deterministic_for       # the wide path takes the edge list
        self.train = D.PackedStream(packed, 4, shuffle=True, seed=50 if other else 1, graphs=graphs)
        self.valid = D.PackedLoader(packed, batch_size=4, graphs=graphs)
        self.test = D.PackedLoader(packed, batch_size=3, graphs=graphs)

    def fit(self, max_epochs, **kw):
        return fastegnn_amd.fit(self.model, self.opt, self.train, self.valid, self.test, SIGMA, WEIGHT, max_epochs=max_epochs,
                                sampler=self.sampler, num_sample=NUM_SAMPLE, test_interval=2, **kw)

    def state(self):
        return dict(params=[p.detach().clone() for p in self.model.parameters()], m=[t.clone() for t in self.opt.exp_avg],
                    v=[t.clone() for t in self.opt.exp_avg_sq], steps=self.opt.steps, sampler=self.sampler.state_dict(),
                    stream=self.train.state_dict(), lr=self.opt.lr)


def _assert_same_state(a, b):
    for key in ("params", "m", "v"):
        assert len(a[key]) == len(b[key]) and all(torch.equal(x, y) for x, y in zip(a[key], b[key])), key
    assert a["steps"] == b["steps"] and a["sampler"] == b["sampler"] and a["stream"] == b["stream"] and a["lr"] == b["lr"]


def _strip(best):
    return {k: v for k, v in best.items() if k != "time_cost"}


def test_two_runs_of_one_seed_and_a_resumed_run_give_the_same_bits(packed, tmp_path):
    a = _Run(packed, 128)
    best_a, log_a = a.fit(EPOCHS)
    assert log_a["epochs"] == [2, 4] and len(log_a["loss_train"]) == EPOCHS and best_a["epoch_index"] in (2, 4)
    assert all(x == x and x > 0 for x in log_a["loss_train"] + log_a["loss"])
    assert max(a.opt.steps) == 2 * EPOCHS and a.sampler.counter == 2 * EPOCHS      # two batches per epoch, one draw each
    # (1) the mode's promise: a second uninterrupted run is the same run
    a2 = _Run(packed, 128)
    best_a2, log_a2 = a2.fit(EPOCHS)
    _assert_same_state(a.state(), a2.state())
    assert log_a2 == log_a and _strip(best_a2) == _strip(best_a)
    # (2) two epochs, a checkpoint, fresh objects, two more
    ckpt, log_path = tmp_path / "ckpt.pt", tmp_path / "log.json"
    b = _Run(packed, 128)
    b.fit(2, checkpoint_path=ckpt, log_path=log_path)
    c = _Run(packed, 128, model_seed=99, other=True)
    assert not torch.equal(next(c.model.parameters()), next(b.model.parameters()))
    best_c, log_c = c.fit(EPOCHS, checkpoint_path=ckpt, log_path=log_path, resume=True)
    _assert_same_state(c.state(), a.state())
    assert log_c == log_a and _strip(best_c) == _strip(best_a)
    assert json.loads(log_path.read_text())[1] == log_a
    assert torch.load(ckpt, weights_only=True)["extra"]["epoch_index"] == EPOCHS


def test_fused_path_restores_every_state_and_draws_the_same_next_batch(packed, tmp_path):
    ckpt = tmp_path / "ckpt.pt"
    b = _Run(packed, 64)
    best_b, log_b = b.fit(2, checkpoint_path=ckpt)
    assert max(b.opt.steps) == 4
    c = _Run(packed, 64, model_seed=99, other=True)
    extra = load_checkpoint(ckpt, c.model, c.opt, sampler=c.sampler, loaders=(c.train, c.valid, c.test))
    assert extra["epoch_index"] == 2 and extra["log_dict"] == log_b and _strip(extra["best_log_dict"]) == _strip(best_b)
    _assert_same_state(c.state(), b.state())
    assert c.model._range.wide == b.model._range.wide
    # a resume that has nothing left to do loads the same state and returns the logs
    d = _Run(packed, 64, model_seed=98, other=True)
    best_d, log_d = d.fit(2, checkpoint_path=ckpt, resume=True)
    _assert_same_state(d.state(), b.state())
    assert log_d == log_b and _strip(best_d) == _strip(best_b)
    # the next batch and the next sample are the ones the uninterrupted run draws
    nb, nc = b.train.next(), c.train.next()
    assert torch.equal(b.train.ids, c.train.ids)
    for key in ("loc_0", "vel_0", "loc_t", "edge_index"):
        assert torch.equal(nb[key], nc[key]), key
    (sb, cb), (sc, cc) = b.sampler.draw(nb["ptr"], NUM_SAMPLE), c.sampler.draw(nc["ptr"], NUM_SAMPLE)
    assert torch.equal(sb, sc) and torch.equal(cb, cc)
