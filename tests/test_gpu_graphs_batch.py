"""-m gpu: the batched graph build (graphs.radius_graph_batch / cutoff_edges_batch, data.water3d_batch,
Simulation(frames_per_call=k)) against oracle/graphs_ref.py applied per graph: the expected list is the concatenation of the
per-graph results with the node offset added; edge_index by integer equality, dist at rtol = 1e-6.  The last two tests compare
two builds of this tree with each other (batched against per-frame) and say so."""
import numpy as np
import pytest
import torch

from fastegnn_amd.graphs import cutoff_edges, cutoff_edges_batch, radius_graph, radius_graph_batch
from oracle import graphs_ref as G

pytestmark = pytest.mark.gpu


def _ptr(sizes):
    return np.concatenate([[0], np.cumsum(sizes)]).astype(np.int64)


def _oracle(loc, ptr, r, kdtree=False):
    """Per-graph oracle lists [(edge_index with global ids, dist)], an empty graph giving an empty list."""
    out = []
    for s, e in zip(ptr[:-1], ptr[1:]):
        if e - s < 2:
            out.append((np.zeros((2, 0), np.int64), np.zeros(0, np.float32)))
            continue
        ei, d = (G.radius_graph_kdtree if kdtree else G.radius_graph_bruteforce)(loc[s:e], r)
        out.append((ei + s, d))
    return out


def _check(got, per_graph):
    ei, d, edge_ptr = got
    want_ptr = _ptr([p[0].shape[1] for p in per_graph])
    assert edge_ptr.dtype == torch.int64 and edge_ptr.is_cuda and edge_ptr.tolist() == want_ptr.tolist()
    want_ei = np.concatenate([p[0] for p in per_graph], 1)
    assert ei.dtype == torch.int64 and tuple(ei.shape) == want_ei.shape
    assert np.array_equal(ei.cpu().numpy(), want_ei)
    assert d.dtype == torch.float32
    assert np.allclose(d.cpu().numpy(), np.concatenate([p[1] for p in per_graph]), rtol=1e-6, atol=0)


def _check_cutoff(got, full, per_graph, rate):
    """``full``: the batched radius graph the cutoff was given (already held to ``per_graph``, the oracle's lists).  The oracle's
    cutoff is applied per graph to what the cutoff received, edge ids and lengths: the order among ties and near-ties is then
    defined bit for bit (the device lengths may differ from the oracle's in the last place, which rtol = 1e-6 allows, and an
    order decided on other lengths is no reference for this one).  Against the oracle's own lists: counts and kept lengths."""
    ei, d, ep = (t.cpu().numpy() for t in full)
    cut = [G.cutoff_edges(ei[:, a:b], d[a:b], rate) for a, b in zip(ep[:-1], ep[1:])]
    assert [c[0].shape[1] for c in cut] == [int(p[0].shape[1] * (1 - rate)) for p in per_graph]
    _check(got, cut)
    assert np.array_equal(got[1].cpu().numpy(), np.concatenate([c[1] for c in cut]))
    want_d = np.concatenate([G.cutoff_edges(p[0], p[1], rate)[1] for p in per_graph])
    assert np.allclose(got[1].cpu().numpy(), want_d, rtol=1e-6, atol=0)
    d, ep = got[1], got[2].tolist()
    for a, b in zip(ep, ep[1:]):
        assert b - a < 2 or bool((d[a + 1:b] >= d[a:b - 1]).all())      # ascending inside every graph


def test_one_graph_equals_the_single_cloud_build():
    """B = 1: identical to radius_graph on the same cloud (a comparison of two builds of this tree)."""
    loc = torch.from_numpy((np.random.RandomState(300).rand(300, 3) - 0.3).astype(np.float32)).cuda()
    ei1, d1 = radius_graph(loc, 0.12)
    ei, d, ep = radius_graph_batch(loc, torch.tensor([0, 300]), 0.12)
    assert ei1.shape[1] > 0 and torch.equal(ei, ei1) and torch.equal(d, d1)
    assert ep.tolist() == [0, ei1.shape[1]]


RAGGED = [1, 2, 300, 0, 1500, 77]


@pytest.fixture(scope="module")
def ragged():
    """Six clouds in one region of space, so that a cell lookup that crossed a graph boundary would find points.  With the
    coincident pair the oracle counts 14 254 edges in graph 4 (14 252 without it)."""
    ptr = _ptr(RAGGED)
    loc = (np.random.RandomState(11).rand(ptr[-1], 3) * 1 - 0.3).astype(np.float32)
    loc[ptr[1] + 1] = loc[ptr[1]] + np.float32([0.05, 0, 0])
    loc[ptr[4] + 7] = loc[ptr[4] + 3]                    # coincident pair (distance 0)
    per_graph = _oracle(loc, ptr, 0.12)
    assert [p[0].shape[1] for p in per_graph] == [0, 2, 562, 0, 14254, 48]
    return loc, ptr, per_graph, radius_graph_batch(torch.from_numpy(loc).cuda(), torch.from_numpy(ptr), 0.12)


def test_ragged_batch_in_one_region_equals_per_graph_bruteforce(ragged):
    loc, ptr, per_graph, got = ragged
    _check(got, per_graph)
    ei, _, ep = got
    batch = torch.repeat_interleave(torch.arange(len(RAGGED)), torch.tensor(RAGGED)).cuda()
    assert torch.equal(batch[ei[0]], batch[ei[1]])       # no edge between two graphs
    assert ep[3] == ep[4]                                # the empty middle graph
    # ptr on the device or as a list gives the same result
    again = radius_graph_batch(torch.from_numpy(loc).cuda(), torch.from_numpy(ptr).cuda(), 0.12)
    assert all(torch.equal(a, b) for a, b in zip(got, again))


@pytest.mark.parametrize("rate", [0.0, 0.25, 0.5, 0.9, 1.0])
def test_cutoff_on_the_ragged_batch_equals_per_graph_cutoff(ragged, rate):
    _, _, per_graph, (ei, d, ep) = ragged
    before = (ei.clone(), d.clone(), ep.clone())
    got = cutoff_edges_batch(ei, d, ep, rate)
    _check_cutoff(got, (ei, d, ep), per_graph, rate)
    assert all(torch.equal(a, b) for a, b in zip((ei, d, ep), before))        # the inputs are left as they were
    # and equal to the single-cloud cutoff of every graph's own list (a build of this tree)
    single = [cutoff_edges(ei[:, a:b], d[a:b], rate) for a, b in zip(ep.tolist(), ep.tolist()[1:])]
    assert torch.equal(got[0], torch.cat([s[0] for s in single], 1)) and torch.equal(got[1], torch.cat([s[1] for s in single]))
    if rate == 0.25:
        assert torch.diff(got[2]).tolist() == [0, 1, 421, 0, 10690, 36]
    if rate == 1.0:
        assert got[0].shape == (2, 0) and got[1].numel() == 0 and got[2].tolist() == [0] * 7
    # the host copy of edge_ptr (no read-back inside the call) gives the same list
    again = cutoff_edges_batch(ei, d, ep, rate, edge_ptr_host=ep.tolist())
    assert all(torch.equal(a, b) for a, b in zip(got, again))


def test_many_small_clouds():
    """500 graphs of 5 to 40 points: per-graph grids of a single cell or a few, nothing sized by a cell table."""
    g = np.random.RandomState(5)
    sizes = g.randint(5, 41, 500)
    ptr = _ptr(sizes)
    loc = g.randn(ptr[-1], 3).astype(np.float32)
    per_graph = _oracle(loc, ptr, 1.0)
    assert ptr[-1] == 10887 and sum(p[0].shape[1] for p in per_graph) == 22596
    _check(radius_graph_batch(torch.from_numpy(loc).cuda(), ptr.tolist(), 1.0), per_graph)


def test_grids_that_differ_per_graph_in_both_orders():
    """One cloud at the 256-cell clamp (r < extent / 256) beside one of a few cells, at the same r."""
    g = np.random.RandomState(17)
    a = g.rand(20000, 3).astype(np.float32)
    a[0], a[1], a[2] = 0.0, 1.0, np.float32(1.0) - np.float32(0.001)       # pin the box; a pair in the last cell
    b = (g.rand(400, 3) * 0.01).astype(np.float32)
    r = 0.0039
    oa, ob = G.radius_graph_kdtree(a, r), G.radius_graph_kdtree(b, r)
    assert oa[0].shape[1] == 96 and 20000 < ob[0].shape[1] < 28000
    for first, second, of, os_ in ((a, b, oa, ob), (b, a, ob, oa)):
        n = len(first)
        got = radius_graph_batch(torch.from_numpy(np.concatenate([first, second])).cuda(), [0, n, n + len(second)], r)
        _check(got, [of, (os_[0] + n, os_[1])])


def test_contact_graph_shape_and_its_cutoff():
    """2 x 3 341 points in a 36 A cube offset by +50, r = 10: about 0.72 M edges per graph, a few hundred per centre."""
    g = np.random.RandomState(6)
    loc = (g.rand(2 * 3341, 3) * 36 + 50).astype(np.float32)
    ptr = _ptr([3341, 3341])
    per_graph = _oracle(loc, ptr, 10.0, kdtree=True)
    assert all(650000 < p[0].shape[1] < 790000 for p in per_graph)
    got = radius_graph_batch(torch.from_numpy(loc).cuda(), ptr, 10.0)
    _check(got, per_graph)
    _check_cutoff(cutoff_edges_batch(*got, 0.5), got, per_graph, 0.5)


def test_malformed_ptr_raises_and_the_next_call_works():
    """The status word of the count call: the kernels clamp every range to [0, N], so nothing is indexed outside loc."""
    loc = torch.from_numpy(np.random.RandomState(3).rand(300, 3).astype(np.float32)).cuda()
    for bad in ([0, 200, 100, 300], [0, 100, 250], [0, 100, 400], [5, 100, 300]):
        with pytest.raises(RuntimeError, match="ptr is not"):
            radius_graph_batch(loc, bad, 0.12)
    ptr = _ptr([100, 200])
    _check(radius_graph_batch(loc, ptr, 0.12), _oracle(loc.cpu().numpy(), ptr, 0.12))


def _clouds(sizes, seed):
    g = torch.Generator().manual_seed(seed)
    out = []
    for n in sizes:
        pos = (torch.rand(n, 3, generator=g) * 0.25).cuda()
        vel = (torch.randn(n, 3, generator=g) * 0.003).cuda()
        kind = torch.randint(1, 4, (n, 1), generator=g).float().cuda()
        out.append((pos, vel, pos + 15 * vel, kind))
    return out


@pytest.mark.parametrize("rotation", [None, "callable"])
def test_water3d_batch_equals_collated_frames_and_trains(rotation):
    """Batched against per-frame, both builds of this tree: every tensor of the Batch is torch.equal."""
    import fastegnn_amd
    from fastegnn_amd import data as D
    from fastegnn_amd.train import FusedAdam, train_step
    clouds = _clouds((1500, 2200), 3)

    def rotations():      # a fresh stream of per-graph rotations for each of the two builds
        g = torch.Generator().manual_seed(9)
        return (lambda: torch.linalg.qr(torch.randn(3, 3, generator=g))[0]) if rotation else None
    rot = rotations()
    want = D.collate([D.water3d_frame(p, v, t, k, virtual_channels=4, radius=0.035, cutoff_rate=0.5, rotation=rot)
                      for p, v, t, k in clouds])
    cat = [torch.cat([c[i] for c in clouds], 0) for i in range(4)]
    got = D.water3d_batch(*cat, [0, 1500, 3700], virtual_channels=4, radius=0.035, cutoff_rate=0.5, rotation=rotations())
    assert list(got.keys()) == list(want.keys())
    for k in want.keys():
        assert got[k].dtype == want[k].dtype and got[k].device == want[k].device and torch.equal(got[k], want[k]), k
    assert got["edge_index"].shape[1] > 10000
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, 4, device="cuda", n_layers=2, gravity=[0, -1, 0])
    opt = FusedAdam(m.parameters(), lr=5e-4, weight_decay=1e-12)
    g = torch.Generator().manual_seed(4)
    sample = torch.stack([torch.randperm(1500, generator=g)[:12], 1500 + torch.randperm(2200, generator=g)[:12]]).cuda()
    loss, _ = train_step(m, opt, got, sample_nodes=sample, sigma=1.0, weight=0.01)
    assert np.isfinite(float(loss))


def test_simulation_frames_per_call_gives_the_same_frames(tmp_path):
    """Simulation(frames_per_call=15) and (=4: ragged last call) against frames_per_call=1, all builds of this tree."""
    from dataclasses import fields
    from fastegnn_amd.data import Frame, Simulation
    g = np.random.RandomState(0)
    arrays = {}
    for t in range(3):
        pos = g.rand(1, 600, 3) * 0.25 + np.cumsum(g.randn(40, 600, 3) * 0.001, 0)
        arrays[f"traj{t}/position"] = pos.astype(np.float32)
        arrays[f"traj{t}/particle_type"] = g.randint(1, 4, 600)
    (tmp_path / "w3d").mkdir()
    np.savez(tmp_path / "w3d" / "train.npz", **arrays)
    kw = dict(dataset_name="w3d", data_dir=str(tmp_path), virtual_channels=3, delta_t=5, cutoff_rate=0.25, seed=1)
    one = Simulation(**kw)
    assert len(one) == 45 and min(f.edge_index.shape[1] for f in one.data) > 100
    for k in (15, 4):
        many = Simulation(frames_per_call=k, **kw)
        assert many.frames == one.frames and len(many) == len(one)
        for fa, fb in zip(many.data, one.data):
            for f in fields(Frame):
                a, b = getattr(fa, f.name), getattr(fb, f.name)
                assert a.dtype == b.dtype and a.shape == b.shape and torch.equal(a, b), f.name
