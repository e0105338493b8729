"""CPU: the host side of rigid motions on the trajectory path (fastegnn_amd/data.py: ``apply_motion``, ``TrajectoryDataset(rotation=,
translation=, motion_seed=)``, ``batch(ids, motion=)``; fastegnn_amd/rollout.py) -- the motion table, its validation, and the
orchestration of ``batch()`` / ``Rollout`` through the torch restatement of the device calls (tests/motion_ref.py) with brute-force
edges.  Nothing here needs a GPU; the kernels themselves are tests/test_gpu_motion.py's."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from tests.motion_ref import MovedRolloutOps, MovedTrajOps, rule_numpy, split
from tests.rollout_ref import StandIn
from tests.trajectory_ref import DELTA_T, FIRST, RADIUS, make_trajectories, sliced, write_npz

R = importlib.import_module("fastegnn_amd.rollout")   # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("fastegnn_traj_gather_moved", "fastegnn_rollout_graph_moved")
IDS = [FIRST["A"], FIRST["C"], FIRST["B"] + 1, FIRST["A"]]   # ragged, a one-point cloud, a repeat


@pytest.fixture()
def mirror(monkeypatch):
    monkeypatch.setattr(D, "_TRAJ_OPS", MovedTrajOps)
    monkeypatch.setattr(R, "_ROLLOUT_OPS", MovedRolloutOps)
    monkeypatch.setattr(MovedTrajOps, "calls", [])
    monkeypatch.setattr(MovedRolloutOps, "calls", [])


@pytest.fixture(scope="module")
def trajectories():
    return make_trajectories(0)[:3]   # without the 2 049-point cloud: the brute-force edges are quadratic


def _ds(trajectories, **kw):
    return D.TrajectoryDataset(trajectories, 3, DELTA_T, RADIUS, 0.25, device="cpu", **kw)


def _bits(t):
    return t.contiguous().view(torch.int32)


# ---- the rule ----
def test_apply_motion_is_the_rule_operation_by_operation():
    assert fastegnn_amd.apply_motion is D.apply_motion and "apply_motion" in fastegnn_amd.__all__
    g = torch.Generator().manual_seed(0)
    x, Rm, t = torch.randn(500, 3, generator=g) * 3, torch.randn(3, 3, generator=g), torch.randn(3, generator=g) * 5
    assert np.array_equal(D.apply_motion(x, Rm, t).numpy(), rule_numpy(x.numpy(), Rm.numpy(), t.numpy()))
    assert np.array_equal(D.apply_motion(x, Rm).numpy(), rule_numpy(x.numpy(), Rm.numpy()))
    assert D.apply_motion(x, Rm.numpy(), t.numpy()).dtype == torch.float32           # arrays are taken as fp32
    # without t no addition runs: -0.0 stays -0.0; with t = 0 it becomes +0.0
    z = torch.full((1, 3), -0.0)
    assert bool(torch.signbit(D.apply_motion(z, torch.eye(3))).all())
    assert not bool(torch.signbit(D.apply_motion(z, torch.eye(3), torch.zeros(3))).any())


# ---- the constructor ----
def test_y_and_xyz_tables(trajectories):
    S = len(_ds(trajectories))
    ds = _ds(trajectories, rotation="y", motion_seed=3)
    assert ds.motion.shape == (S, 12) and ds.motion.dtype == torch.float32 and not ds._has_t and not ds.motion[:, 9:].any()
    deg = np.random.default_rng(3).integers(0, 361, size=S)
    c, s = np.cos(np.radians(deg.astype(np.float64))), np.sin(np.radians(deg.astype(np.float64)))
    for i in range(S):   # the reference's roty, built in fp64 and rounded once
        want = np.array([[c[i], 0, s[i]], [0, 1, 0], [-s[i], 0, c[i]]]).astype(np.float32)
        assert np.array_equal(ds.motion[i, :9].view(3, 3).numpy(), want), i
    ds = _ds(trajectories, rotation="xyz", translation=5.0, motion_seed=3)
    Rm = ds.motion[:, :9].view(S, 3, 3).double()
    assert float((Rm @ Rm.transpose(1, 2) - torch.eye(3, dtype=torch.float64)).abs().max()) <= 1e-6
    assert float((torch.linalg.det(Rm) - 1).abs().max()) <= 1e-6 and ds._has_t
    rng = np.random.default_rng(3)
    deg = rng.integers(0, 361, size=(S, 3))
    c, s = (np.stack([f(np.radians(deg[:, a].astype(np.float64))) for a in range(3)], 1)[0] for f in (np.cos, np.sin))
    rx = np.array([[1, 0, 0], [0, c[0], -s[0]], [0, s[0], c[0]]])
    ry = np.array([[c[1], 0, s[1]], [0, 1, 0], [-s[1], 0, c[1]]])
    rz = np.array([[c[2], -s[2], 0], [s[2], c[2], 0], [0, 0, 1]])
    assert np.array_equal(ds.motion[0, :9].view(3, 3).numpy(), (rx @ ry @ rz).astype(np.float32))   # rotx @ roty @ rotz
    assert np.array_equal(ds.motion[:, 9:].numpy(), (rng.standard_normal((S, 3)) * 5.0).astype(np.float32))   # drawn after the angles
    per_axis = _ds(trajectories, translation=(1.0, 0.0, 2.0), motion_seed=3)                          # a scale per axis, no rotation
    assert torch.equal(per_axis.motion[:, :9], torch.eye(3).reshape(1, 9).expand(S, 9)) and not per_axis.motion[:, 10].any()
    assert np.array_equal(per_axis.motion[:, 9:].numpy(),
                          (np.random.default_rng(3).standard_normal((S, 3)) * np.array([1.0, 0.0, 2.0])).astype(np.float32))


def test_seeds_and_explicit_tables(trajectories):
    S = len(_ds(trajectories))
    a, b, c = (_ds(trajectories, rotation="xyz", translation=2.0, motion_seed=s).motion for s in (7, 7, 8))
    assert torch.equal(a, b) and not torch.equal(a[:, :9], c[:, :9]) and not torch.equal(a[:, 9:], c[:, 9:])
    assert _ds(trajectories).motion is None and _ds(trajectories, motion_seed=5).motion is None
    g = torch.Generator().manual_seed(1)
    one, many = torch.randn(3, 3, generator=g), torch.randn(S, 3, 3, generator=g)
    t1, tS = torch.randn(3, generator=g), torch.randn(S, 3, generator=g)
    ds = _ds(trajectories, rotation=one, translation=t1)
    assert torch.equal(ds.motion[:, :9], one.reshape(1, 9).expand(S, 9)) and torch.equal(ds.motion[:, 9:], t1.expand(S, 3)) and ds._has_t
    ds = _ds(trajectories, rotation=many.numpy(), translation=tS.numpy())
    assert torch.equal(ds.motion[:, :9], many.reshape(S, 9)) and torch.equal(ds.motion[:, 9:], tS)
    ds = _ds(trajectories, rotation=many.double())   # fp64 input: rounded once
    assert torch.equal(ds.motion[:, :9], many.reshape(S, 9)) and not ds._has_t


def test_bad_motion_arguments_raise_value_error(trajectories):
    S = len(_ds(trajectories))
    nan = torch.eye(3).clone()
    nan[1, 1] = float("nan")
    for kw in (dict(rotation="z"), dict(rotation="reference"), dict(rotation=nan), dict(rotation=torch.full((3, 3), float("inf"))),
               dict(rotation=torch.eye(4)), dict(rotation=torch.zeros(S + 1, 3, 3)), dict(rotation=torch.zeros(9)),
               dict(translation=float("nan")), dict(translation=(1.0, 2.0)), dict(translation=torch.zeros(S + 1, 3)),
               dict(translation=torch.tensor([0.0, float("inf"), 0.0])), dict(translation=np.zeros((2, 2)))):
        with pytest.raises(ValueError):
            _ds(trajectories, **kw)


# ---- orchestration through the mirror ----
def test_an_unmoved_dataset_makes_the_calls_and_the_batches_it_made_before(mirror, trajectories):
    ds = _ds(trajectories)
    got = ds.batch(IDS)
    assert MovedTrajOps.calls == ["plan", "gather", "mean"]
    loc_0, vel_0, loc_t, kind, ptr = sliced(trajectories, ds.samples, IDS, DELTA_T)
    assert torch.equal(got["loc_0"], loc_0) and torch.equal(got["loc_t"], loc_t) and torch.equal(got["vel_0"], vel_0)
    assert torch.equal(got["node_attr"], kind) and got["ptr"].tolist() == ptr
    assert "motion" not in ds._assemble_nodes(torch.tensor(IDS), np.asarray(IDS))
    out = R.rollout(StandIn(), ds, IDS, 2)
    assert set(MovedRolloutOps.calls) == {"graph"} and out["counted"].tolist() == [4, 3]
    assert "gather_moved" not in MovedTrajOps.calls and "mean_of" not in MovedTrajOps.calls


@pytest.mark.parametrize("translation", [None, 5.0])
def test_a_moved_batch_is_the_rule_applied_to_the_slices(mirror, trajectories, translation):
    ds = _ds(trajectories, rotation="xyz", translation=translation, motion_seed=2)
    got = ds.batch(IDS)
    assert MovedTrajOps.calls == ["plan", "gather_moved", "mean_of"]     # + the index_select of the rows: four launches on the device
    loc_0, vel_0, loc_t, kind, ptr = sliced(trajectories, ds.samples, IDS, DELTA_T)
    plain = _ds(trajectories).batch(IDS)
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        Rm, t = split(ds.motion[IDS[b]], translation is not None)
        assert (t is None) == (translation is None)
        for k, src, tt in (("loc_0", loc_0, t), ("loc_t", loc_t, t), ("vel_0", vel_0, None)):
            want = rule_numpy(src[s:e].numpy(), Rm.numpy(), None if tt is None else tt.numpy())
            assert np.array_equal(got[k][s:e].numpy(), want), (b, k)
        v = got["vel_0"][s:e].numpy()
        assert np.array_equal(got["node_feat"][s:e, 0].numpy(), np.sqrt((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]))
        mean64 = got["loc_0"][s:e].double().mean(0)     # the mean of the MOVED cloud
        assert float((got["loc_mean"][b].double() - mean64[:, None]).abs().max()) <= 2.0 ** -23 * float(got["loc_0"][s:e].abs().max())
    for k in ("node_attr", "batch", "ptr"):
        assert torch.equal(got[k], plain[k]), k
    assert torch.equal(got["node_feat"][:, 1], plain["node_feat"][:, 1])
    assert list(got.keys()) == list(plain.keys())
    # the graph is built from the moved loc_0: the attribute is the moved pair's length
    row, col = got["edge_index"]
    d = (got["loc_0"][row].double() - got["loc_0"][col].double()).pow(2).sum(-1).sqrt()
    assert got["edge_index"].size(1) > 0 and float((got["edge_attr"][:, 0].double() - d).abs().max()) <= 1e-6 * max(1.0, float(got["loc_0"].abs().max()))


def test_an_explicit_motion_overrides_the_table(mirror, trajectories):
    ds, B = _ds(trajectories, rotation="y", motion_seed=1), len(IDS)
    g = torch.Generator().manual_seed(4)
    Rm, t = torch.linalg.qr(torch.randn(B, 3, 3, generator=g))[0].contiguous(), torch.randn(B, 3, generator=g)
    rows = torch.cat([Rm.reshape(B, 9), t], 1)
    got = ds.batch(IDS, motion=rows)
    pair = ds.batch(IDS, motion=(Rm, t))
    assert all(torch.equal(got[k], pair[k]) for k in got.keys())
    loc_0 = sliced(trajectories, ds.samples, IDS, DELTA_T)[0]
    ptr = got["ptr"].tolist()
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        assert np.array_equal(got["loc_0"][s:e].numpy(), rule_numpy(loc_0[s:e].numpy(), Rm[b].numpy(), t[b].numpy()))
    assert not torch.equal(got["loc_0"], ds.batch(IDS)["loc_0"])
    no_t = ds.batch(IDS, motion=(Rm.numpy(), None))                     # a pair without t: no translation is added
    assert np.array_equal(no_t["loc_0"][:ptr[1]].numpy(), rule_numpy(loc_0[:ptr[1]].numpy(), Rm[0].numpy()))
    moved_plain = _ds(trajectories).batch(IDS, motion=rows)            # a dataset without a table takes one per call
    assert all(torch.equal(got[k], moved_plain[k]) for k in got.keys())
    bad = rows.clone()
    bad[1, 4] = float("nan")
    for motion in (rows[:2], rows.double(), bad, (Rm[:1], t), (Rm, t[:, :2]), (Rm, t, t)):
        with pytest.raises(ValueError):
            ds.batch(IDS, motion=motion)


@pytest.mark.parametrize("translation", [None, (0.5, 5.0, 0.0)])
def test_getitem_sees_the_clouds_batch_sees(mirror, trajectories, translation, monkeypatch):
    """``ds[i]`` hands ``water3d_frame`` the moved slices and no ``rotation=`` (the frame's graph needs the device: the call is caught
    here, and tests/test_gpu_motion.py runs it)"""
    def caught(loc_0, vel_0, loc_t, node_type, virtual_channels, radius, cutoff_rate):
        return dict(loc_0=loc_0, vel_0=vel_0, loc_t=loc_t, node_attr=node_type, args=(virtual_channels, radius, cutoff_rate))
    monkeypatch.setattr(D, "water3d_frame", caught)
    ds = _ds(trajectories, rotation="xyz", translation=translation, motion_seed=6)
    for i in (FIRST["A"] + 1, FIRST["B"], FIRST["C"] + 2, -1):
        frame, batch = ds[i], ds.batch([i % len(ds)])
        for k in ("loc_0", "loc_t", "vel_0"):
            assert torch.equal(_bits(frame[k]), _bits(batch[k])), (i, k)
        assert torch.equal(frame["node_attr"], batch["node_attr"]) and frame["args"] == (3, RADIUS, 0.25)
    plain = _ds(trajectories)
    assert torch.equal(plain[0]["loc_0"], plain.batch([0])["loc_0"]) and not torch.equal(ds[0]["loc_0"], plain[0]["loc_0"])


def test_loader_batches_are_moved(mirror, trajectories):
    ds = _ds(trajectories, rotation="xyz", translation=1.0)
    gen = lambda: torch.Generator().manual_seed(5)  # noqa: E731
    order = torch.randperm(len(ds), generator=gen()).tolist()
    for i, got in enumerate(D.TrajectoryLoader(ds, 4, shuffle=True, generator=gen())):
        want = ds.batch(order[4 * i:4 * i + 4])
        assert all(torch.equal(got[k], want[k]) for k in want.keys())


def test_from_directory_reference_protocol(trajectories, tmp_path):
    os.makedirs(tmp_path / "set")
    for partition in ("train", "test"):
        write_npz(tmp_path / "set" / f"{partition}.npz", trajectories)
    args = dict(max_samples=20, delta_t=DELTA_T, device="cpu", seed=1, radius=RADIUS)
    test = D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="test", rotation="reference", motion_seed=9, **args)
    train = D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="train", rotation="reference", motion_seed=9, **args)
    assert train.motion is None and test.motion.shape == (20, 12) and test.frames == train.frames
    y = D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="train", rotation="y", translation=2.0, motion_seed=9, **args)
    assert torch.equal(y.motion[:, :9], test.motion[:, :9]) and y._has_t and bool(y.motion[:, 9:].any())
    m = test.motion[:, :9].view(-1, 3, 3)
    assert bool((m[:, 1, 1] == 1).all()) and not m[:, 0, 1].any() and not m[:, 1, 0].any() and torch.equal(m[:, 0, 2], -m[:, 2, 0])
    assert D.TrajectoryDataset.from_directory("set", str(tmp_path), 3, partition="test", **args).motion is None


# ---- rollouts ----
@pytest.mark.parametrize("translation", [None, 3.0])
def test_a_rollout_over_a_moved_dataset_scores_against_moved_truth(mirror, trajectories, translation):
    ds = _ds(trajectories, rotation="xyz", translation=translation, motion_seed=4)
    ids, steps = [FIRST["A"], FIRST["C"], FIRST["B"] + 1], 3
    ro = R.Rollout(StandIn(), ds, ids, steps=steps, record=True)
    want0 = ds.batch(ids)
    assert all(torch.equal(ro.batch[k], want0[k]) for k in ro.batch.keys())          # step 0 is the moved batch
    while ro.k < ro.steps:
        ro.step()
    out = ro.result()
    assert set(MovedRolloutOps.calls) == {"graph_moved"} and out["stopped"] is None and out["counted"].tolist() == [3, 2, 1]
    ptr = want0["ptr"].tolist()
    want = torch.full((steps, len(ids)), float("nan"), dtype=torch.float64)
    for b, i in enumerate(ids):
        t_, f = (int(v) for v in ds.samples[i])
        Rm, t = split(ds.motion[i], translation is not None)
        for k in range(steps):
            frame = f + (k + 1) * DELTA_T
            if frame < int(ds.T_host[t_]):
                truth = rule_numpy(trajectories[t_][1][frame], Rm.numpy(), None if t is None else t.numpy())
                d = out["pred"][k, ptr[b]:ptr[b + 1]].double() - torch.from_numpy(truth).double()
                want[k, b] = float((d ** 2).sum()) / (3 * (ptr[b + 1] - ptr[b]))
    have = ~torch.isnan(want)
    assert torch.equal(torch.isnan(out["per_graph"]), ~have)
    assert float(((out["per_graph"] - want)[have].abs() / want[have]).max()) <= 1e-12
    # against the unmoved truth the score is another number: the frame matters
    d = out["pred"][0, :ptr[1]].double() - torch.from_numpy(trajectories[0][1][DELTA_T]).double()
    assert abs(float((d ** 2).sum()) / (3 * ptr[1]) - float(out["per_graph"][0, 0])) > 1e-3 * float(out["per_graph"][0, 0])
    # from_state has no dataset and no motion
    b = want0
    free = R.Rollout.from_state(StandIn(), b["loc_0"], b["vel_0"], b["node_attr"], b["ptr"], virtual_channels=3, radius=RADIUS,
                                cutoff_rate=0.25, delta_t=DELTA_T, steps=1)
    free.step()
    assert free._motion is None and torch.isnan(free.result()["mse"]).all()


# ---- ABI ----
def test_header_declares_and_binding_lists_the_new_exports():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    assert "#define FASTEGNN_ABI_VERSION 108" in src and "rigid motions" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in K.EXPORTED
    assert K.ABI_VERSION == 108
    assert all(callable(getattr(D.HipTrajOps, n)) for n in ("gather_moved", "mean_of")) and callable(R.HipRolloutOps.graph_moved)


def test_every_product_library_exports_them_and_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            assert all(hasattr(L, n) for n in NEW_EXPORTS)
    L, one = K.lib(), C.c_void_p(64)   # (never dereferenced: every call below is refused on the host)
    gather = L.fastegnn_traj_gather_moved
    assert gather(one, one, 1, 5, one, 1, one, one, 1, one, one, one, one, one, one, None, 1, None) == -1 and b"null" in L.fastegnn_last_error()
    assert gather(one, one, 1, -1, one, 1, one, one, 1, one, one, one, one, one, one, one, 1, None) == -1
    assert gather(one, one, 1, 5, None, 1, one, one, 1, one, one, one, one, one, one, one, 1, None) == -1
    assert gather(one, one, 1, 5, one, 1, one, one, 1, one, one, None, one, one, one, one, 1, None) == -1
    assert gather(one, one, 1, 5, one, 0, one, one, 1, one, one, one, one, one, one, one, 1, None) == -1
    assert gather(one, one, 0, 0, None, 0, None, None, 0, None, None, None, None, None, None, None, 0, None) == 0   # nothing to do
    graph = L.fastegnn_rollout_graph_moved
    assert graph(one, 1, one, one, 5, one, 5, one, 3, one, one, None, 1, None) == -1 and b"motion" in L.fastegnn_last_error()
    assert graph(one, 1, one, one, 5, one, 5, one, 0, one, one, one, 1, None) == -1 and b"C out of range" in L.fastegnn_last_error()
    assert graph(one, -1, one, one, 5, one, 5, one, 3, one, one, one, 1, None) == -1
    assert graph(None, 1, one, one, 5, one, 5, one, 3, one, one, one, 1, None) == -1
    assert graph(one, 1, one, one, 5, one, 5, None, 3, one, one, one, 1, None) == -1    # a score without its truth rows
    assert graph(None, 0, None, None, 0, None, 0, None, 3, None, None, None, 0, None) == 0   # nothing to do
