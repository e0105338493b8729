"""CPU: the host side of the trajectory loader (fastegnn_amd/data.py: TrajectoryDataset / TrajectoryLoader) -- sample enumeration and
validation, the orchestration of ``batch()`` through the torch mirror of the three device calls (tests/trajectory_ref.py) with brute-force
edges, and the ABI of the new exports.  Nothing here needs a GPU; the kernels themselves are tests/test_gpu_trajectory.py's."""
import os
import re

import numpy as np
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from oracle import graphs_ref
from tests.packed_ref import make_frame
from tests.trajectory_ref import DELTA_T, FIRST, N_SAMPLES, RADIUS, SHAPES, TorchTrajOps, make_trajectories, sliced, write_npz

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("fastegnn_traj_plan", "fastegnn_traj_gather", "fastegnn_traj_mean")


class MirrorOps(TorchTrajOps):
    """the mirror plus the edges the product path gets from the batched graph calls: per cloud the float32 brute force and the cutoff
    of oracle/graphs_ref.py, ids shifted by the cloud's first node"""

    @staticmethod
    def edges(loc_0, ptr, ptr_host, radius, cutoff_rate):
        assert ptr.tolist() == list(ptr_host)
        ei, dist = [], []
        for a, b in zip(ptr_host, ptr_host[1:]):
            e, d = graphs_ref.cutoff_edges(*graphs_ref.radius_graph_bruteforce(loc_0[a:b].numpy(), radius), cutoff_rate)
            ei.append(torch.from_numpy(e) + a)
            dist.append(torch.from_numpy(d))
        return torch.cat(ei, 1), torch.cat(dist, 0)


@pytest.fixture()
def mirror(monkeypatch):
    monkeypatch.setattr(D, "_TRAJ_OPS", MirrorOps)


@pytest.fixture(scope="module")
def trajectories():
    return make_trajectories(0)


# ---- sample enumeration ----
@pytest.mark.parametrize("delta_t", [0, 1, 2])
def test_all_enumerates_every_start_frame(trajectories, delta_t):
    ds = D.TrajectoryDataset(trajectories, 3, delta_t, RADIUS, device="cpu")
    want = [(t, f) for t, (_, T, _) in enumerate(SHAPES) for f in range(T) if f + max(1, delta_t) <= T - 1]
    assert ds.samples.dtype == np.int64 and ds.samples.tolist() == [list(p) for p in want] and len(ds) == len(want)
    assert ds.frames == [(SHAPES[t][0], f) for t, f in want]
    if delta_t == DELTA_T:
        assert len(ds) == N_SAMPLES and all(ds.samples[FIRST[k]].tolist() == [t, 0] for t, (k, _, _) in enumerate(SHAPES))


def test_device_state_is_positions_and_kinds_with_64_bit_offsets(trajectories):
    ds = D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, device="cpu")
    n, T = np.asarray([s[2] for s in SHAPES]), np.asarray([s[1] for s in SHAPES])
    assert ds.pos.shape == (int((n * T).sum()), 3) and ds.pos.dtype == torch.float32
    assert ds.kind.shape == ds.kind_scaled.shape == (int(n.sum()), 1)
    for host, dev, want in ((ds.row0_host, ds.row0, np.concatenate([[0], np.cumsum(n * T)[:-1]])), (ds.n_host, ds.n, n),
                            (ds.T_host, ds.T, T), (ds.kind0_host, ds.kind0, np.concatenate([[0], np.cumsum(n)[:-1]]))):
        assert host.dtype == np.int64 and dev.dtype == torch.int64 and host.tolist() == dev.tolist() == want.tolist()
    for t, (_, position, kind) in enumerate(trajectories):
        r0, k0 = int(ds.row0_host[t]), int(ds.kind0_host[t])
        assert torch.equal(ds.pos[r0:r0 + T[t] * n[t]], torch.from_numpy(position).reshape(-1, 3))
        k = torch.from_numpy(kind).reshape(-1, 1)
        assert torch.equal(ds.kind[k0:k0 + n[t]], k) and torch.equal(ds.kind_scaled[k0:k0 + n[t]], k / k.max())


def test_from_directory_draws_the_frames_of_the_rule(trajectories, tmp_path):
    """15 start frames per trajectory from [0, min(250, T - 1 - max(1, delta_t))], cut at max_samples, one permutation: restated with
    numpy's generator, in that order of calls"""
    os.makedirs(tmp_path / "set")
    write_npz(tmp_path / "set" / "valid.npz", trajectories)
    for max_samples, seed in ((1e8, 0), (50, 3), (15, 1)):
        ds = D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="valid", max_samples=max_samples, delta_t=DELTA_T,
                                                device="cpu", seed=seed, radius=RADIUS)
        rng, want = np.random.default_rng(seed), []
        for key, T, _ in SHAPES:
            count = min(15, int(max_samples) - len(want))
            want += [(key, int(f)) for f in rng.integers(0, min(250, T - 1 - DELTA_T) + 1, size=count)]
            if len(want) >= max_samples:
                break
        want = [want[i] for i in rng.permutation(len(want))]
        assert ds.frames == want and len(ds) == len(want) == min(60, int(max_samples))
        assert ds.radius == RADIUS and ds.delta_t == DELTA_T
    assert D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="valid", delta_t=1, device="cpu").radius == D.Simulation.RADIUS


def test_bad_samples_raise_value_error_naming_the_first(trajectories):
    T_a = SHAPES[0][1]
    with pytest.raises(ValueError, match=r"sample 1 = \(trajectory 0, start frame 4\)"):   # T - max(1, delta_t) = 6 - 2
        D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, samples=np.asarray([[0, 3], [0, T_a - DELTA_T], [9, 0]]), device="cpu")
    with pytest.raises(ValueError, match=r"sample 0 = \(trajectory 0, start frame 5\)"):   # delta_t = 0 still reads frame f + 1
        D.TrajectoryDataset(trajectories, 3, 0, RADIUS, samples=np.asarray([[0, T_a - 1]]), device="cpu")
    with pytest.raises(ValueError, match=r"sample 2 = \(trajectory -1, start frame 0\)"):
        D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, samples=np.asarray([[0, 0], [1, 1], [-1, 0]]), device="cpu")
    with pytest.raises(ValueError, match=r"sample 0 = \(trajectory 4, start frame 0\)"):
        D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, samples=np.asarray([[4, 0]]), device="cpu")
    with pytest.raises(ValueError, match=r"sample 0 = \(trajectory 2, start frame -1\)"):
        D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, samples=np.asarray([[2, -1]]), device="cpu")
    with pytest.raises(ValueError, match="empty cloud"):
        D.TrajectoryDataset(trajectories + [("E", np.zeros((5, 0, 3), np.float32), np.zeros(0, np.float32))], 3, DELTA_T, RADIUS,
                            device="cpu")
    with pytest.raises(ValueError, match="integer array"):
        D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, samples=np.asarray([[0.0, 1.0]]), device="cpu")
    with pytest.raises(ValueError, match="3 kinds for 37"):
        D.TrajectoryDataset([("A", trajectories[0][1], np.ones(3, np.float32))], 3, DELTA_T, RADIUS, device="cpu")


# ---- orchestration of batch() through the mirror ----
@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("cutoff_rate", [0.0, 0.25])
@pytest.mark.parametrize("ids", [[0], [4, 5], [FIRST["C"] + 3, 1, 1, FIRST["B"]], "tensor"], ids=["one", "B only", "repeats", "tensor ids"])
def test_batch_orchestration_against_direct_slicing(mirror, trajectories, ids, cutoff_rate, C):
    ds = D.TrajectoryDataset(trajectories, C, DELTA_T, RADIUS, cutoff_rate, device="cpu")
    if ids == "tensor":
        ids = torch.tensor([FIRST["A"] + 2, FIRST["C"], FIRST["B"] + 1, FIRST["A"]], dtype=torch.int64)
    got = ds.batch(ids)
    ids = [int(i) for i in ids]
    assert list(got.keys()) == list(D.collate([make_frame(2, 1, C)]).keys())
    loc_0, vel_0, loc_t, kind, ptr = sliced(trajectories, ds.samples, ids, DELTA_T)
    N, B = ptr[-1], len(ids)
    assert got["ptr"].tolist() == ptr and got["ptr"].dtype == torch.int64
    assert got["batch"].tolist() == [b for b in range(B) for _ in range(ptr[b + 1] - ptr[b])] and got["batch"].dtype == torch.int64
    assert torch.equal(got["loc_0"], loc_0) and torch.equal(got["loc_t"], loc_t) and torch.equal(got["vel_0"], vel_0)
    assert torch.equal(got["node_attr"], kind) and got["node_attr"].shape == (N, 1)
    v = vel_0.numpy()
    speed = np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2])
    assert got["node_feat"].shape == (N, 2) and np.array_equal(got["node_feat"][:, 0].numpy(), speed)
    scaled = torch.cat([kind[a:b] / kind[a:b].max() for a, b in zip(ptr, ptr[1:])], 0)
    assert torch.equal(got["node_feat"][:, 1:], scaled)
    assert got["loc_mean"].shape == (B, 3, C)
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        want = loc_0[s:e].double().mean(0)
        assert (got["loc_mean"][b].double() - want[:, None]).abs().max() <= 2.0 ** -23 * loc_0[s:e].abs().max()
    # the edges are the per-cloud brute force, in its order, with global ids; the attribute is their length
    E = got["edge_index"].size(1)
    assert got["edge_index"].dtype == torch.int64 and got["edge_attr"].shape == (E, 1)
    at = 0
    for s, e in zip(ptr, ptr[1:]):
        ei, d = graphs_ref.cutoff_edges(*graphs_ref.radius_graph_bruteforce(loc_0[s:e].numpy(), RADIUS), cutoff_rate)
        assert np.array_equal(got["edge_index"][:, at:at + d.size].numpy(), ei + s) and np.array_equal(got["edge_attr"][at:at + d.size, 0].numpy(), d)
        at += d.size
    assert at == E and (E > 0) == any(e - s > 1 for s, e in zip(ptr, ptr[1:]))


def test_batch_validates_ids_on_the_host_as_the_packed_dataset_does(mirror, trajectories):
    ds = D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, device="cpu")
    for bad in ([-1], [N_SAMPLES], [0, 2 ** 40]):
        with pytest.raises(IndexError):
            ds.batch(bad)
    for bad in ([], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            ds.batch(bad)
    with pytest.raises(IndexError):
        ds[N_SAMPLES]


def test_the_mirror_clamps_what_the_kernels_clamp(trajectories):
    """the plan's clamps restated: ids outside, a trajectory number outside, a frame beyond T -- every slot row stays inside pos"""
    ds = D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, device="cpu")
    samples = ds.samples_dev.clone()
    samples[2] = torch.tensor([0, 99])      # a frame beyond T
    samples[3] = torch.tensor([7, 0])       # a trajectory beyond the set
    ids = torch.tensor([-1, N_SAMPLES, 2 ** 40, 2, 3], dtype=torch.int64)
    ptr, slots = torch.empty(6, dtype=torch.int64), torch.empty(5, 4, dtype=torch.int64)
    TorchTrajOps.plan(ids, samples, ds.row0, ds.n, ds.T, ds.kind0, DELTA_T, ptr, slots)
    n = [37, 2049, 2049, 37, 2049]
    assert ptr.tolist() == np.concatenate([[0], np.cumsum(n)]).tolist()
    assert slots[3, :3].tolist() == [5 * 37] * 3 and slots[4].tolist() == slots[1].tolist()
    assert int((slots[:, :3] + torch.tensor(n)[:, None]).max()) <= ds.pos.size(0) and int(slots.min()) >= 0


def test_loader_follows_data_loader_and_restores_its_order(mirror, trajectories):
    ds = D.TrajectoryDataset(trajectories, 1, DELTA_T, RADIUS, device="cpu")
    seen, assemble = [], ds._assemble
    ds._assemble = lambda ids_dev, ids_host: seen.append((ids_dev.tolist(), ids_host.tolist())) or assemble(ids_dev, ids_host)

    def epoch(loader):
        del seen[:]
        sizes = [b.num_graphs for b in loader]
        assert sizes == [4, 4, 4, 2] and all(dev == host for dev, host in seen)   # the device slice and the host slice agree
        return [host for _, host in seen]

    loader = D.TrajectoryLoader(ds, 4, shuffle=True, generator=torch.Generator().manual_seed(5))
    state = loader.state_dict()
    first, second = epoch(loader), epoch(loader)
    ref = torch.Generator().manual_seed(5)
    for got in (first, second):   # DataLoader's order: one randperm per epoch from the loader's generator
        order = torch.randperm(N_SAMPLES, generator=ref).tolist()
        assert got == [order[i:i + 4] for i in range(0, N_SAMPLES, 4)]
    assert first != second
    loader.load_state_dict(state)
    assert epoch(loader) == first
    assert len(loader) == 4 and len(D.TrajectoryLoader(ds, 4, drop_last=True)) == 3
    assert [b.num_graphs for b in D.TrajectoryLoader(ds, 5)] == [5, 5, 4]


# ---- ABI ----
def test_header_declares_and_binding_lists_the_new_exports():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    assert "#define FASTEGNN_ABI_VERSION 108" in src and "#define FASTEGNN_TRAJ_SLOT_WORDS 4" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in K.EXPORTED
    assert K.ABI_VERSION == 108 and D._TRAJ_SLOT_WORDS == 4 and D._TRAJ_OPS is D.HipTrajOps


def test_every_product_library_exports_them_and_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            assert all(hasattr(L, n) for n in NEW_EXPORTS)
    L, one = K.lib(), C.c_void_p(64)   # (never dereferenced: every call below is refused on the host)
    assert L.fastegnn_traj_plan(one, -1, one, 1, one, one, one, one, 1, 2, one, one, None) == -1 and b"B < 0" in L.fastegnn_last_error()
    assert L.fastegnn_traj_plan(one, 1, one, 0, one, one, one, one, 1, 2, one, one, None) == -1
    assert L.fastegnn_traj_plan(one, 1, one, 1, one, one, one, one, 1, -1, one, one, None) == -1 and b"delta_t" in L.fastegnn_last_error()
    assert L.fastegnn_traj_plan(None, 1, one, 1, one, one, one, one, 1, 2, one, one, None) == -1 and b"null" in L.fastegnn_last_error()
    assert L.fastegnn_traj_gather(one, one, 1, -1, one, 1, one, one, 1, one, one, one, one, one, one, None) == -1
    assert L.fastegnn_traj_gather(one, one, 1, 5, None, 1, one, one, 1, one, one, one, one, one, one, None) == -1
    assert L.fastegnn_traj_gather(one, one, 1, 5, one, 1, one, one, 1, one, one, None, one, one, one, None) == -1
    assert L.fastegnn_traj_gather(one, one, 1, 5, one, 0, one, one, 1, one, one, one, one, one, one, None) == -1
    assert L.fastegnn_traj_gather(one, one, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None, None) == 0   # nothing to do
    assert L.fastegnn_traj_mean(one, one, 1, one, 1, 0, one, None) == -1 and b"C out of range" in L.fastegnn_last_error()
    assert L.fastegnn_traj_mean(one, one, 1, one, 1, 3, None, None) == -1
    assert L.fastegnn_traj_mean(one, None, 1, one, 1, 3, one, None) == -1
