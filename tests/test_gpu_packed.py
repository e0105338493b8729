"""PackedDataset.batch / PackedLoader on the device (csrc/collate.hip) against ``data.collate`` of the same frames on the same
device.  Copies and integer additions are exact: every comparison is ``torch.equal``, key order included; no tolerance anywhere."""
import numpy as np
import pytest
import torch

from fastegnn_amd import data as D
from tests.packed_ref import ZERO_EDGE_FRAMES, assert_batches_equal, make_frame, ragged_frames

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def packed():
    return D.PackedDataset(ragged_frames(C=3, seed=0), device="cuda")


def _check(packed, ids):
    want = D.collate([packed[int(i)] for i in ids])
    got = packed.batch(ids)
    assert_batches_equal(got, want)
    assert all(got[k].device == want[k].device for k in want.keys())
    return got


@pytest.mark.parametrize("ids", [list(range(23)), list(range(22, -1, -1)), [4, 9, 4, 0, 9, 9], [5], [ZERO_EDGE_FRAMES[0]]],
                         ids=["in order", "reversed", "repeated ids", "B=1", "B=1 without edges"])
def test_ragged_batches_equal_collate(packed, ids):
    assert packed.device.type == "cuda" and packed.tables["loc_mean"].shape[1:] == (3, 3)
    _check(packed, ids)


def test_a_batch_of_frames_without_edges(packed):
    """every edge table is empty: they take no part in the launch (an empty grid would be a launch error)"""
    got = _check(packed, list(ZERO_EDGE_FRAMES))
    assert got["edge_index"].shape == (2, 0) and got["edge_attr"].shape == (0, 1)
    assert got["ptr"].tolist() == [0, 3, 6] and got["batch"].tolist() == [0, 0, 0, 1, 1, 1]
    _check(packed, list(ZERO_EDGE_FRAMES) + [2])   # the empty segments in front of a full one


def test_more_frames_than_one_scan_round():
    """B = 300 in one batch: the plan kernel's offsets over 300 frames of 3..7 nodes, and 2 100 frames (three rounds of its scan)"""
    gen = torch.Generator().manual_seed(3)
    frames = [make_frame(int(n), int(e), 3, 1, gen) for n, e in zip(torch.randint(3, 8, (300,), generator=gen),
                                                                    torch.randint(0, 13, (300,), generator=gen))]
    p = D.PackedDataset(frames, device="cuda")
    got = _check(p, torch.randperm(300, generator=gen))
    assert got.num_graphs == 300
    _check(p, torch.randint(0, 300, (2100,), generator=gen))


def test_one_big_frame_between_two_single_nodes():
    gen = torch.Generator().manual_seed(7)
    frames = [make_frame(1, 1, 1, 2, gen), make_frame(3001, 20011, 1, 2, gen), make_frame(1, 2, 1, 2, gen)]
    p = D.PackedDataset(frames, device="cuda")
    got = _check(p, [0, 1, 2])
    assert got["edge_attr"].shape == (20014, 2) and got["loc_mean"].shape == (3, 3, 1)
    assert got["ptr"].tolist() == [0, 1, 3002, 3003]
    # the segment boundaries by themselves: first and last row of each frame, first and last edge
    for i, (a, b, ea, eb) in enumerate([(0, 1, 0, 1), (1, 3002, 1, 20012), (3002, 3003, 20012, 20014)]):
        f = frames[i].to("cuda")
        for k in ("loc_0", "loc_t", "vel_0", "node_feat", "node_attr"):
            assert torch.equal(got[k][a], f[k][0]) and torch.equal(got[k][b - 1], f[k][-1]), (i, k)
        assert torch.equal(got["edge_attr"][ea], f.edge_attr[0]) and torch.equal(got["edge_attr"][eb - 1], f.edge_attr[-1])
        assert torch.equal(got["edge_index"][:, ea], f.edge_index[:, 0] + a)
        assert torch.equal(got["edge_index"][:, eb - 1], f.edge_index[:, -1] + a)
        assert got["batch"][a].item() == i and got["batch"][b - 1].item() == i
    _check(p, [1, 0, 1])


def test_packed_loader_equals_data_loader(packed):
    old = D.DataLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(21))
    new = D.PackedLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(21))
    got, want = list(new), list(old)
    assert len(got) == len(want) == len(new) == len(old) == 6 and got[-1].num_graphs == 3
    for a, b in zip(got, want):
        assert_batches_equal(a, b)


def test_an_epoch_does_no_host_work_that_synchronises(packed):
    """the whole second epoch -- its order upload included -- under torch's synchronisation check: no copy from pageable memory,
    no read-back, nothing that waits for the device"""
    loader = D.PackedLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(2))
    want = list(D.DataLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(2)))
    first = list(loader)   # warm-up epoch
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(first) == len(second) == 6
    for a, b in zip(first, want):
        assert_batches_equal(a, b)
    ref = torch.Generator().manual_seed(2)
    torch.randperm(23, generator=ref)
    order = torch.randperm(23, generator=ref).tolist()   # the generator's second draw
    for i, b in enumerate(second):
        assert_batches_equal(b, D.collate([packed[j] for j in order[4 * i:4 * i + 4]]))


def test_a_packed_batch_trains():
    import fastegnn_amd
    from fastegnn_amd.train import FusedAdam, MMDSampler, train_step
    gen = torch.Generator().manual_seed(5)
    frames = []
    for n in (5, 7, 5, 6, 5, 8):   # complete graphs without self loops, as the N-body reader builds them
        ij = torch.tensor([(i, j) for i in range(n) for j in range(n) if i != j], dtype=torch.int64).t().contiguous()
        f = make_frame(n, ij.size(1), 3, 1, gen)
        f.edge_index = ij
        f.edge_attr = (f.loc_0[ij[0]] - f.loc_0[ij[1]]).norm(dim=1, keepdim=True)
        frames.append(f)
    loader = D.PackedLoader(D.PackedDataset(frames, device="cuda"), batch_size=4, shuffle=True,
                            generator=torch.Generator().manual_seed(1))
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, 3, device="cuda", n_layers=2)
    opt = FusedAdam(m.parameters(), lr=5e-4, weight_decay=1e-12)
    batch = next(iter(loader))
    assert batch.num_graphs == 4
    loss, _ = train_step(m, opt, batch, None, sigma=1.0, weight=0.01, sampler=MMDSampler(0), num_sample=3)
    assert np.isfinite(float(loss))
