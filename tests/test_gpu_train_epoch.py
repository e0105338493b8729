"""train_epoch (fastegnn_amd/train.py): the reference's training epoch with its loss summed on the device, against a hand-written
``train_step`` loop that reads every batch's loss back.  Two models from one seed, each with its own optimizer and its own sampler of
one seed, see the same batches: the two runs differ only by the arrival order of the kernels' atomic sums, which DESIGN.md section 6
measures at the 1e-7 level per tensor -- hence 1e-5 relative on the epoch's two numbers."""
import math

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import data as D
from fastegnn_amd.train import FusedAdam, MMDSampler, train_epoch, train_step
from tests.packed_ref import make_frame

pytestmark = pytest.mark.gpu

SIGMA, WEIGHT, NUM_SAMPLE, REL = 1.0, 0.01, 3, 1e-5


def _frames():
    """10 complete graphs of 5 nodes (20 edges); the targets of the last two are three times as far away, so that the last batch of a
    loader of 4 + 4 + 2 has a loss of its own and a wrong weighting shows"""
    gen = torch.Generator().manual_seed(5)
    ij = torch.tensor([(i, j) for i in range(5) for j in range(5) if i != j], dtype=torch.int64).t().contiguous()
    frames = []
    for i in range(10):
        f = make_frame(5, 20, 3, 1, gen)
        f.edge_index = ij
        f.edge_attr = (f.loc_0[ij[0]] - f.loc_0[ij[1]]).norm(dim=1, keepdim=True)
        if i >= 8:
            f.loc_t = f.loc_t * 3
        frames.append(f)
    return frames


@pytest.fixture(scope="module")
def packed():
    return D.PackedDataset(_frames(), device="cuda")


def _twin():
    torch.manual_seed(11)
    m = fastegnn_amd.FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2, hidden_nf=64, virtual_channels=3, device="cuda",
                              n_layers=2)
    return m, FusedAdam(m.parameters(), lr=5e-4, weight_decay=1e-12), MMDSampler(3)


def _by_hand(model, opt, smp, loader):
    """-> (graph-weighted mse, graph-weighted loss, unweighted mean of the per-batch mse, graphs)"""
    model.train()
    rows = []
    for data in loader:
        loss, mse = train_step(model, opt, data, None, SIGMA, WEIGHT, sampler=smp, num_sample=NUM_SAMPLE)
        rows.append((data["loc_mean"].size(0), loss.item(), mse.item()))
    graphs = sum(b for b, _, _ in rows)
    return (sum(b * m for b, _, m in rows) / graphs, sum(b * l for b, l, _ in rows) / graphs,
            sum(m for _, _, m in rows) / len(rows), graphs)


def _compare(make_loader, want_graphs, batch_sizes, weighting_shows=False):
    (ma, oa, sa), (mb, ob, sb) = _twin(), _twin()
    for pa, pb in zip(ma.parameters(), mb.parameters()):
        assert torch.equal(pa, pb)
    loader_a = make_loader(ma)
    assert [b["loc_mean"].size(0) for b in make_loader(ma)] == batch_sizes
    mse, loss, unweighted, graphs = _by_hand(ma, oa, sa, loader_a)
    if weighting_shows:   # FIRST: a mean over batches is not the mean over graphs here, or the comparison below could hide a wrong weighting
        assert abs(unweighted - mse) > 1e-3, (unweighted, mse)
    got = train_epoch(mb, ob, make_loader(mb), SIGMA, WEIGHT, sampler=sb, num_sample=NUM_SAMPLE)
    print(f"by hand: mse {mse!r} loss {loss!r} unweighted {unweighted!r}; train_epoch: {got!r}")
    assert graphs == want_graphs and got["graphs"] == want_graphs and isinstance(got["graphs"], int)
    assert math.isfinite(mse) and math.isfinite(loss)
    assert abs(got["mse"] - mse) <= REL * abs(mse), (got["mse"], mse)
    assert abs(got["loss"] - loss) <= REL * abs(loss), (got["loss"], loss)
    assert mb.training


def test_train_epoch_returns_the_graph_weighted_means_of_a_hand_written_loop(packed):
    """batches of 4, 4 and 2 graphs, the last one with a loss of its own"""
    _compare(lambda m: D.PackedLoader(packed, batch_size=4, drop_last=False), 10, [4, 4, 2], weighting_shows=True)


def test_train_epoch_over_a_packed_stream(packed):
    _compare(lambda m: D.PackedStream(packed, 4, shuffle=True, seed=1, graphs=m.deterministic_for), 8, [4, 4])


def test_train_epoch_over_an_empty_loader(packed):
    m, opt, smp = _twin()
    m.eval()
    got = train_epoch(m, opt, [], SIGMA, WEIGHT, sampler=smp, num_sample=NUM_SAMPLE)
    assert math.isnan(got["mse"]) and math.isnan(got["loss"]) and got["graphs"] == 0
    assert m.training
