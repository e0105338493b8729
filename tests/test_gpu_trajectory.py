"""TrajectoryDataset.batch / TrajectoryLoader on the device (csrc/traj.hip) against ``data.water3d_batch`` of the same clouds sliced from
the raw arrays by torch, and ``ds[i]`` against ``Simulation``.  Copies, integers and the one subtraction per component of ``vel_0`` are
exact (``torch.equal``); ``node_feat[:,0]`` is bit-equal to numpy's float32 evaluation of ``sqrt((vx*vx + vy*vy) + vz*vz)`` (every
operation rounded, a correctly rounded root) and within one unit in the last place of the yardstick's; ``loc_mean`` is within
``2^-23 max|loc_0 of the graph|`` of the fp64 mean -- derived, not measured: the fp64 accumulation of at most 2^24 fp32 terms
contributes far less, the one rounding to fp32 at most half a unit at the data's scale.  No tolerance here was taken from a run."""
import os

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from fastegnn_amd.train import FusedAdam, MMDSampler, evaluate, train_epoch
from tests.packed_ref import make_frame
from tests.trajectory_ref import DELTA_T, FIRST, N_SAMPLES, RADIUS, make_trajectories, sliced, write_npz

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 67   # guard bands: sentinel value, elements on either side of every output (odd: the float outputs start unaligned)
NODE_OUT = ("loc_0", "loc_t", "vel_0", "node_feat", "node_attr")
BATCHES = {
    "one": [0],
    "B only": [FIRST["B"], FIRST["B"] + 1],
    "repeats, the large cloud first": [FIRST["D"], FIRST["A"] + 1, FIRST["A"] + 1, FIRST["C"] + 3, FIRST["B"]],
    "every sample, shuffled": torch.randperm(N_SAMPLES, generator=torch.Generator().manual_seed(11)).tolist(),
}


@pytest.fixture(scope="module")
def trajectories():
    return make_trajectories(0)


@pytest.fixture(scope="module")
def datasets(trajectories):
    """one dataset per (virtual_channels, cutoff_rate), made on first use"""
    made = {}

    def get(C, cutoff_rate):
        if (C, cutoff_rate) not in made:
            made[C, cutoff_rate] = D.TrajectoryDataset(trajectories, C, DELTA_T, RADIUS, cutoff_rate, device="cuda")
        return made[C, cutoff_rate]
    return get


def _banded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _direct(ds, ids_dev, N, samples=None):
    """the three device calls themselves, every output carved from a larger sentinel-filled buffer -> {name: (buffer, view)}"""
    B, C = ids_dev.numel(), ds.virtual_channels
    shapes = dict(loc_0=(N, 3), loc_t=(N, 3), vel_0=(N, 3), node_feat=(N, 2), node_attr=(N, 1), loc_mean=(B, 3, C))
    out = {k: _banded(s, torch.float32) for k, s in shapes.items()}
    out.update(batch=_banded((N,), torch.int64), ptr=_banded((B + 1,), torch.int64), slots=_banded((B, 4), torch.int64))
    v = {k: view for k, (_, view) in out.items()}
    ops = D.HipTrajOps
    ops.plan(ids_dev, ds.samples_dev if samples is None else samples, ds.row0, ds.n, ds.T, ds.kind0, ds.delta_t, v["ptr"], v["slots"])
    ops.gather(v["ptr"], v["slots"], N, ds.pos, ds.kind, ds.kind_scaled, *[v[k] for k in NODE_OUT], v["batch"])
    ops.mean(v["ptr"], v["slots"], ds.pos, v["loc_mean"])
    torch.cuda.synchronize()   # an error of the runtime would surface here
    return out


def _bands_intact(out):
    for k, (buf, view) in out.items():
        n = view.numel()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), k


# ---- 1. batch parity with water3d_batch, 4. the guard bands of the same cases ----
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cutoff_rate", [0.0, 0.25])
@pytest.mark.parametrize("name", list(BATCHES))
def test_batch_equals_water3d_batch(trajectories, datasets, name, cutoff_rate, C):
    ds, ids = datasets(C, cutoff_rate), BATCHES[name]
    assert len(ds) == N_SAMPLES and ds.pos.is_cuda
    got = ds.batch(ids)
    loc_0, vel_0, loc_t, kind, ptr = sliced(trajectories, ds.samples, ids, DELTA_T, device="cuda")
    want = D.water3d_batch(loc_0, vel_0, loc_t, kind, ptr, C, RADIUS, cutoff_rate)
    assert list(got.keys()) == list(want.keys()) == list(D.collate([make_frame(2, 1, C)]).keys())
    for k in want.keys():
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape and got[k].is_contiguous() and got[k].is_cuda, k
    for k in ("loc_0", "loc_t", "vel_0", "node_attr", "batch", "ptr", "edge_index", "edge_attr"):
        assert torch.equal(got[k], want[k]), k
    assert torch.equal(got["node_feat"][:, 1], want["node_feat"][:, 1])
    has_edges = any(b - a > 1 for a, b in zip(ptr, ptr[1:]))
    assert (got["edge_index"].size(1) > 0) == has_edges

    v = got["vel_0"].cpu().numpy()
    speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    assert speed.dtype == np.float32
    mine, theirs = got["node_feat"][:, 0].cpu().numpy(), want["node_feat"][:, 0].cpu().numpy()
    print(f"node_feat[:,0]: {int((mine != speed).sum())} of {mine.size} differ from numpy, "
          f"max |mine - yardstick| / ulp = {float((np.abs(mine - theirs) / np.spacing(np.abs(theirs))).max())}")
    assert np.array_equal(mine, speed)
    assert (np.abs(mine - theirs) <= np.spacing(np.abs(theirs))).all()

    again = ds.batch(ids)["loc_mean"]
    assert torch.equal(again, got["loc_mean"])                                      # two calls, identical bits
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        mean64, bound = loc_0[s:e].double().mean(0), 2.0 ** -23 * float(loc_0[s:e].abs().max())
        err = float((got["loc_mean"][b].double() - mean64[:, None]).abs().max())
        assert err <= bound, (b, err, bound)
        assert torch.equal(got["loc_mean"][b], got["loc_mean"][b, :, :1].expand(3, C))   # all C columns equal
        if e - s == 1:
            assert torch.equal(got["loc_mean"][b, :, 0], loc_0[s])                  # a one-point cloud: the mean is the point

    # the same batch with every output between guard bands: nothing outside is written, every element inside is
    out = _direct(ds, torch.tensor(ids, dtype=torch.int64, device="cuda"), ptr[-1])
    _bands_intact(out)
    for k in NODE_OUT + ("loc_mean", "batch", "ptr"):
        assert torch.equal(out[k][1], got[k]), k


def test_ids_may_live_on_either_side(datasets):
    ds, ids = datasets(3, 0.25), BATCHES["repeats, the large cloud first"]
    want = ds.batch(ids)
    for form in (np.asarray(ids), torch.tensor(ids), torch.tensor(ids, device="cuda")):
        got = ds.batch(form)
        assert all(torch.equal(got[k], want[k]) for k in want.keys())
    with pytest.raises(IndexError):
        ds.batch(torch.tensor([0, N_SAMPLES], device="cuda"))


# ---- 2. ds[i] against Simulation ----
def test_samples_and_frames_equal_simulation(trajectories, tmp_path):
    os.makedirs(tmp_path / "set")
    write_npz(tmp_path / "set" / "train.npz", trajectories)
    args = dict(partition="train", max_samples=50, delta_t=DELTA_T, cutoff_rate=0.25, device="cuda", seed=4, radius=RADIUS)
    ds = D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, **args)
    sim = D.Simulation("set", str(tmp_path), 3, **args)
    assert ds.frames == sim.frames and len(ds) == len(sim) == 50 and {k for k, _ in ds.frames} == {"A", "B", "C", "D"}
    for i in range(len(ds)):
        mine, theirs = ds[i], sim[i]
        for k in ("edge_index", "edge_attr", "loc_0", "loc_t", "vel_0", "node_feat", "node_attr", "loc_mean"):
            assert mine[k].dtype == theirs[k].dtype and torch.equal(mine[k], theirs[k]), (i, ds.frames[i], k)
    a, b = D.collate([ds[i] for i in (3, 0, 7)]), D.collate([sim[i] for i in (3, 0, 7)])   # collate keeps working on the dataset
    assert all(torch.equal(a[k], b[k]) for k in b.keys())


# ---- 3. no host work in the assembly ----
class _CountingLib:
    """the library handle with every fastegnn_* call counted"""

    def __init__(self, lib):
        self._lib, self.calls = lib, []

    def __getattr__(self, name):
        f = getattr(self._lib, name)
        if not name.startswith("fastegnn_"):
            return f

        def call(*args):
            self.calls.append(name)
            return f(*args)
        return call


def test_the_node_side_is_three_calls_and_no_synchronisation(datasets, monkeypatch):
    ds = datasets(3, 0.0)
    many = torch.randint(0, N_SAMPLES, (40,), generator=torch.Generator().manual_seed(2))
    cases = [(ids.to("cuda"), ids.numpy()) for ids in (torch.tensor([FIRST["C"] + 1]), many)]
    want = [ds.batch(host) for _, host in cases]   # warm-up of both shapes, and the results to compare with
    counting = _CountingLib(K.lib())
    monkeypatch.setitem(K._libs, K.LIB_PATH, counting)
    assert K.lib() is counting
    torch.cuda.synchronize()
    counts, got = [], []
    torch.cuda.set_sync_debug_mode("error")
    try:
        for ids_dev, ids_host in cases:
            del counting.calls[:]
            got.append(ds._assemble_nodes(ids_dev, ids_host))
            counts.append(list(counting.calls))
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert counts[0] == counts[1] == ["fastegnn_traj_plan", "fastegnn_traj_gather", "fastegnn_traj_mean"] and len(counts[0]) <= 3
    for g, w in zip(got, want):
        assert all(torch.equal(g[k], w[k]) for k in NODE_OUT + ("loc_mean", "batch", "ptr"))


# ---- 4. bounds: corrupted device arrays are clamped ----
@pytest.mark.parametrize("host_ids, dev_ids", [
    ([1, 4, 5, 0, 2], [-1, N_SAMPLES, 2 ** 40, 0, 2]),                       # the device's clouds are far larger than the host's N
    ([FIRST["D"]] * 3, [-1, FIRST["B"], 2 ** 40]),                           # and smaller: the tail of every output stays unwritten
], ids=["more nodes than the host counted", "fewer nodes than the host counted"])
def test_corrupted_sample_ids_are_clamped(datasets, host_ids, dev_ids):
    """sample ids of -1, len(ds) and 2^40 handed straight to the device calls, the output sizes from the host's (intact) ids: the plan
    clamps every id to [0, len(ds)), the gather writes nothing at or beyond the N it was given and skips what its slot does not cover.
    The batch may be wrong; the call returns, reads nothing outside the tables (by reading csrc/traj.hip: every index is a clamped id, an
    offset below B, or a row checked against the table's rows) and writes nothing outside the outputs."""
    ds = datasets(3, 0.0)
    N = int(ds._node_cnt[host_ids].sum())
    out = _direct(ds, torch.tensor(dev_ids, dtype=torch.int64, device="cuda"), N)
    _bands_intact(out)
    clamped = [min(max(i, 0), N_SAMPLES - 1) for i in dev_ids]
    n = ds._node_cnt[clamped]
    assert out["ptr"][1].tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
    written = min(N, int(n.sum()))
    want = ds.batch(clamped)
    for k in NODE_OUT + ("batch",):   # what lies inside both the host's N and the device's clouds is the clamped samples' data
        assert torch.equal(out[k][1][:written], want[k][:written]), k
        assert bool((out[k][1][written:] == SENT).all()), k
    assert torch.equal(out["loc_mean"][1], want["loc_mean"])


def test_a_corrupted_sample_table_is_clamped(datasets, trajectories):
    """a frame number beyond T, a negative one, trajectory numbers outside the set: frames are clamped to [0, T) one by one (f, f + 1,
    f + delta_t), trajectories to [0, n_traj)"""
    ds = datasets(3, 0.0)
    samples = ds.samples_dev.clone()
    samples[1] = torch.tensor([0, 99])     # A, T = 6: frames 5, 5, 5
    samples[2] = torch.tensor([0, -8])     # A: frames 0, 1, 2
    samples[3] = torch.tensor([77, 0])     # -> D
    samples[4] = torch.tensor([-3, 4])     # -> A, frames 4, 5, 5
    ids = [1, 2, 3, 4]
    N = 37 + 37 + 2049 + 37
    out = _direct(ds, torch.tensor(ids, dtype=torch.int64, device="cuda"), N, samples=samples)
    _bands_intact(out)
    A, Dd = (torch.from_numpy(trajectories[t][1]).cuda() for t in (0, 3))
    assert out["ptr"][1].tolist() == [0, 37, 74, 2123, 2160]
    loc_0, loc_t, vel_0 = (out[k][1] for k in ("loc_0", "loc_t", "vel_0"))
    assert torch.equal(loc_0[:37], A[5]) and torch.equal(loc_t[:37], A[5]) and not vel_0[:37].any()
    assert torch.equal(loc_0[37:74], A[0]) and torch.equal(loc_t[37:74], A[2]) and torch.equal(vel_0[37:74], A[1] - A[0])
    assert torch.equal(loc_0[74:2123], Dd[0]) and torch.equal(loc_t[74:2123], Dd[2])
    assert torch.equal(loc_0[2123:], A[4]) and torch.equal(loc_t[2123:], A[5]) and torch.equal(vel_0[2123:], A[5] - A[4])


# ---- 5. the loader ----
def _same_samples(a, b):
    return all(torch.equal(a[k], b[k]) for k in ("ptr", "batch", "loc_0", "loc_t", "vel_0", "node_attr"))


def test_loader_yields_the_samples_of_data_loader(datasets):
    ds = datasets(3, 0.25)
    new = D.TrajectoryLoader(ds, 4, shuffle=True, drop_last=False, generator=torch.Generator().manual_seed(21))
    old = D.DataLoader(ds, 4, shuffle=True, generator=torch.Generator().manual_seed(21))
    state = new.state_dict()
    got, want = list(new), list(old)
    assert len(got) == len(want) == len(new) == len(old) == 4 and got[-1].num_graphs == 2   # the last batch is short
    assert all(_same_samples(a, b) for a, b in zip(got, want))
    assert all(list(a.keys()) == list(b.keys()) for a, b in zip(got, want))
    second = list(new)
    assert not all(_same_samples(a, b) for a, b in zip(second, got))                        # the next epoch is another order
    new.load_state_dict(state)
    assert all(_same_samples(a, b) for a, b in zip(list(new), got))                         # restored: the same order again


@pytest.mark.parametrize("C", [1, 3])
def test_an_epoch_trains_and_evaluates(datasets, C):
    ds = datasets(C, 0.25)
    loader = D.TrajectoryLoader(ds, 4, shuffle=True, generator=torch.Generator().manual_seed(1))
    torch.manual_seed(0)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, C, device="cuda", n_layers=2)
    opt = FusedAdam(m.parameters(), lr=5e-4, weight_decay=1e-12)
    res = train_epoch(m, opt, loader, 1.0, 0.01, sampler=MMDSampler(0), num_sample=3 * C)
    assert res["graphs"] == len(ds) and np.isfinite(res["loss"]) and np.isfinite(res["mse"])
    res = evaluate(m, loader, 1.0, 0.01)
    assert res["graphs"] == len(ds) and np.isfinite(res["mse"])
