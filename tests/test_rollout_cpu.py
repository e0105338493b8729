"""CPU: the host side of rollouts (fastegnn_amd/rollout.py: Rollout / rollout) driven through the torch restatement of the device calls
(tests/rollout_ref.py, tests/trajectory_ref.py) with brute-force edges and a small torch stand-in model, and the ABI of the new exports.
Nothing here needs a GPU; the kernels themselves are tests/test_gpu_rollout.py's."""
import importlib
import os
import re

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from tests.rollout_ref import MirrorTrajOps, StandIn, TorchRolloutOps, equal_with_nan
from tests.trajectory_ref import FIRST, RADIUS, make_trajectories

R = importlib.import_module("fastegnn_amd.rollout")   # (the package attribute of that name is the function)
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_EXPORTS = ("fastegnn_rollout_plan", "fastegnn_rollout_advance", "fastegnn_rollout_graph")
DT = 2
# A (T = 6, n = 37) from frame 0, C (T = 9, n = 130) from frame 0, B (T = 4, n = 1) from frame 1: ragged, and at stride 2 the truth
# frames run out after 2, 4 and 1 steps
IDS = [FIRST["A"], FIRST["C"], FIRST["B"] + 1]
STEPS = 4
COUNTED = [3, 2, 1, 1]


@pytest.fixture()
def mirror(monkeypatch):
    monkeypatch.setattr(D, "_TRAJ_OPS", MirrorTrajOps)
    monkeypatch.setattr(R, "_ROLLOUT_OPS", TorchRolloutOps)
    monkeypatch.setattr(MirrorTrajOps, "seen", [])


@pytest.fixture(scope="module")
def trajectories():
    return make_trajectories(0)[:3]   # without the 2 049-point cloud: the brute-force edges are quadratic


def _ds(trajectories, cutoff_rate=0.25, delta_t=DT, C=3):
    return D.TrajectoryDataset(trajectories, C, delta_t, RADIUS, cutoff_rate, device="cpu")


def test_public_names():
    assert fastegnn_amd.Rollout is R.Rollout and fastegnn_amd.rollout is R.rollout
    assert {"Rollout", "rollout"} <= set(fastegnn_amd.__all__) and R._ROLLOUT_OPS is R.HipRolloutOps
    assert all(callable(getattr(R.HipRolloutOps, n)) for n in ("plan", "advance", "graph"))


def test_step_0_is_the_loaders_batch(mirror, trajectories):
    ds = _ds(trajectories)
    ro = R.Rollout(StandIn(), ds, IDS, steps=STEPS)
    want = ds.batch(IDS)
    assert list(ro.batch.keys()) == [k for k in want.keys() if k != "loc_t"] and ro.k == 0 and ro.stopped is None
    for k in ro.batch.keys():
        assert ro.batch[k].dtype == want[k].dtype and torch.equal(ro.batch[k], want[k]), k


def test_a_hand_written_loop_over_the_same_ops_gives_the_same_numbers(mirror, trajectories):
    ds = _ds(trajectories)
    out = R.rollout(StandIn(), ds, IDS, STEPS, record=True)
    assert out["stopped"] is None and out["pred"].shape == (STEPS, 37 + 130 + 1, 3)

    ops, model, b = TorchRolloutOps, StandIn(), ds.batch(IDS)
    loc, vel, feat, mean = (b[k].clone() for k in ("loc_0", "vel_0", "node_feat", "loc_mean"))
    ptr, ptr_host, B = b["ptr"], b["ptr"].tolist(), len(IDS)
    ei, ea = b["edge_index"], b["edge_attr"]
    truth = torch.empty(STEPS, B, dtype=torch.int64)
    ops.plan(torch.tensor(IDS), ds.samples_dev, ds.row0, ds.n, ds.T, DT, truth)
    sse, flag = torch.full((STEPS, B), float("nan"), dtype=torch.float64), R.FlagWord("cpu")
    n = torch.tensor(np.diff(ptr_host), dtype=torch.float64)
    inv = np.float32(1.0) / np.float32(DT)
    for k in range(STEPS):
        x = model(node_loc=loc, node_vel=vel, node_attr=None, node_feat=feat, edge_index=ei, loc_mean=mean, data_batch=b["batch"],
                  edge_attr=ops.augment(ea, loc, ei))[0]
        assert torch.equal(out["pred"][k], x), k
        before = loc.clone()
        ops.advance(x, DT, loc, vel, feat, None, flag)
        ops.graph(ptr, loc, x, ds.pos, truth[k], mean, sse[k])
        # the rules themselves, restated once more with numpy
        assert torch.equal(loc, x) and np.array_equal(vel.numpy(), (x.numpy() - before.numpy()) * inv)
        for g, (s, e) in enumerate(zip(ptr_host, ptr_host[1:])):
            t, f = ds.samples[IDS[g]]
            frame = f + (k + 1) * DT
            if frame >= ds.T_host[t]:
                assert torch.isnan(sse[k, g]) and int(truth[k, g]) == -1
                continue
            want = ((x[s:e].double() - torch.from_numpy(trajectories[t][1][frame]).double()) ** 2).sum()
            assert abs(float(sse[k, g]) - float(want)) <= 1e-12 * float(want)
        ei, dist = MirrorTrajOps.edges(loc, ptr, ptr_host, RADIUS, 0.25)
        ea = dist.unsqueeze(-1)
    assert flag.get() == 0
    assert equal_with_nan(out["per_graph"], sse / (3.0 * n)[None, :])
    assert out["counted"].tolist() == COUNTED and out["mse"].dtype == torch.float64
    for k in range(STEPS):
        have = ~torch.isnan(sse[k])
        assert int(have.sum()) == COUNTED[k] and float(out["mse"][k]) == float((sse[k] / (3.0 * n))[have].sum() / COUNTED[k])


def test_counted_and_nan_rows_when_truth_runs_out(mirror, trajectories):
    out = R.rollout(StandIn(), _ds(trajectories), IDS, STEPS + 1)
    nan = torch.isnan(out["per_graph"])
    assert nan.tolist() == [[False, False, False], [False, False, True], [True, False, True], [True, False, True], [True, True, True]]
    assert out["counted"].tolist() == COUNTED + [0] and torch.isnan(out["mse"][4]) and not torch.isnan(out["mse"][:4]).any()
    assert out["pred"] is None and out["stopped"] is None


def test_a_non_finite_prediction_stops_the_rollout_and_never_reaches_the_graph_build(mirror, trajectories):
    ds = _ds(trajectories)
    ro = R.Rollout(StandIn(nan_at=1), ds, IDS, steps=STEPS, record=True)
    ro.step()
    before = {k: ro.batch[k].clone() for k in ("loc_0", "node_feat")}
    x = ro.step()
    assert torch.isnan(x[0, 1]) and torch.isinf(x[-1, 2])
    assert ro.stopped == ("non-finite", 1) and ro.k == 2 and ro.batch is None
    with pytest.raises(RuntimeError, match="has ended"):
        ro.step()
    assert len(MirrorTrajOps.seen) == 3 and all(bool(torch.isfinite(loc).all()) for loc in MirrorTrajOps.seen)
    state = ro._state
    assert state["loc_0"][0, 1] == before["loc_0"][0, 1] and state["loc_0"][-1, 2] == before["loc_0"][-1, 2]     # x_cur is kept,
    assert state["vel_0"][0, 1] == 0 and state["vel_0"][-1, 2] == 0 and bool(torch.isfinite(state["node_feat"]).all())   # with vel 0
    assert torch.equal(state["loc_0"][1:-1], x[1:-1])
    out = ro.result()
    assert out["stopped"] == ("non-finite", 1) and out["counted"].tolist() == [3, 2, 0, 0]
    assert equal_with_nan(out["pred"][1], x)                                         # the record keeps the raw value,
    assert torch.isnan(out["per_graph"][1, 0]) and not torch.isnan(out["per_graph"][1, 1])   # and so does the score of that cloud
    assert torch.isnan(out["per_graph"][2:]).all() and torch.isnan(out["pred"][2:]).all() and torch.isnan(out["mse"][1:]).all()
    # the driver stops as well, and a NaN on the last step is found by result()
    assert R.rollout(StandIn(nan_at=1), ds, IDS, STEPS)["stopped"] == ("non-finite", 1)
    assert R.rollout(StandIn(nan_at=1), ds, IDS, 2)["stopped"] == ("non-finite", 1)


def test_max_edges_stops_the_rollout_before_the_forward(mirror, trajectories):
    ds = _ds(trajectories)
    E0 = ds.batch(IDS)["edge_index"].size(1)
    model = StandIn()
    ro = R.Rollout(model, ds, IDS, steps=STEPS, max_edges=E0 - 1)
    assert ro.stopped == ("max_edges", 0) and ro.batch is None and model.calls == 0
    assert ro.result()["counted"].tolist() == [0] * STEPS
    # the stand-in pulls every node towards its neighbours and its cloud's centre: the second graph is denser than the first
    free = R.Rollout(StandIn(), ds, IDS, steps=STEPS)
    free.step()
    assert free.batch["edge_index"].size(1) > E0
    model = StandIn()
    out = R.rollout(model, ds, IDS, STEPS, max_edges=E0, record=True)   # exactly E0 edges are allowed
    assert out["stopped"] == ("max_edges", 1) and model.calls == 1 and out["counted"].tolist() == [3, 0, 0, 0]
    assert not torch.isnan(out["pred"][0]).any() and torch.isnan(out["pred"][1:]).all() and torch.isnan(out["per_graph"][1:]).all()


def test_bad_arguments_raise(mirror, trajectories):
    with pytest.raises(ValueError, match="delta_t"):
        R.Rollout(StandIn(), _ds(trajectories, delta_t=0), [0], steps=2)
    ds = _ds(trajectories)
    for bad in ([-1], [len(ds)], [0, 2 ** 40]):
        with pytest.raises(IndexError):
            R.Rollout(StandIn(), ds, bad, steps=2)
    for bad in ([], [[0, 1]], [0.5]):
        with pytest.raises(ValueError):
            R.Rollout(StandIn(), ds, bad, steps=2)
    for steps in (0, -1, 1.5):
        with pytest.raises(ValueError, match="steps"):
            R.Rollout(StandIn(), ds, [0], steps=steps)
    with pytest.raises(TypeError):
        R.Rollout(StandIn(), trajectories, [0], steps=2)


def test_the_model_mode_is_restored_and_no_graph_is_recorded(mirror, trajectories):
    ds, model = _ds(trajectories), StandIn()
    model.train()
    out = R.rollout(model, ds, IDS, 2, record=True)
    assert model.training and not out["pred"].requires_grad
    model.eval()
    R.rollout(model, ds, IDS, 1)
    assert not model.training


def test_from_state_steps_without_a_dataset_and_without_a_score(mirror, trajectories):
    ds = _ds(trajectories)
    b = ds.batch(IDS)
    args = dict(virtual_channels=3, radius=RADIUS, cutoff_rate=0.25, delta_t=DT, steps=3, record=True)
    ro = R.Rollout.from_state(StandIn(), b["loc_0"], b["vel_0"], b["node_attr"], b["ptr"], **args)
    first = ro.batch
    assert list(first.keys()) == [k for k in b.keys() if k != "loc_t"]
    for k in ("loc_0", "vel_0", "node_attr", "edge_index", "edge_attr", "batch", "ptr", "loc_mean"):
        assert torch.equal(first[k], b[k]), k
    ptr = b["ptr"].tolist()
    want = torch.cat([D._node_feat(b["vel_0"][s:e], b["node_attr"][s:e]) for s, e in zip(ptr, ptr[1:])], 0)   # water3d_batch's rule
    assert torch.equal(first["node_feat"], want) and torch.equal(first["node_feat"][:, 1], b["node_feat"][:, 1])
    assert first["loc_0"].data_ptr() != b["loc_0"].data_ptr()   # the caller's tensors are not the state
    # the same stepper: a hand-written loop over the ops from that first batch
    ops, model, flag = TorchRolloutOps, StandIn(), R.FlagWord("cpu")
    loc, vel, feat, mean = (first[k].clone() for k in ("loc_0", "vel_0", "node_feat", "loc_mean"))
    ei, ea, want = first["edge_index"], first["edge_attr"], []
    for k in range(3):
        x = model(node_loc=loc, node_vel=vel, node_attr=None, node_feat=feat, edge_index=ei, loc_mean=mean, data_batch=first["batch"],
                  edge_attr=ops.augment(ea, loc, ei))[0]
        want.append(x)
        ops.advance(x, DT, loc, vel, feat, None, flag)
        ops.graph(first["ptr"], loc, None, None, None, mean, None)
        ei, dist = MirrorTrajOps.edges(loc, first["ptr"], ptr, RADIUS, 0.25)
        ea = dist.unsqueeze(-1)
    while ro.k < ro.steps:
        ro.step()
    out = ro.result()
    assert torch.equal(out["pred"], torch.stack(want))
    assert torch.isnan(out["mse"]).all() and torch.isnan(out["per_graph"]).all() and out["counted"].tolist() == [0, 0, 0]
    assert out["stopped"] is None and b["loc_0"].equal(ds.batch(IDS)["loc_0"])
    with pytest.raises(ValueError, match="ptr"):
        R.Rollout.from_state(StandIn(), b["loc_0"], b["vel_0"], b["node_attr"], [0, 5], **args)
    with pytest.raises(ValueError, match="delta_t"):
        R.Rollout.from_state(StandIn(), b["loc_0"], b["vel_0"], b["node_attr"], b["ptr"], **dict(args, delta_t=0))


def test_the_plan_mirror_clamps_what_the_kernel_clamps(trajectories):
    ds = _ds(trajectories)
    samples = ds.samples_dev.clone()
    samples[2] = torch.tensor([0, 99])      # a frame beyond T: clamped to T - 1 = 5, every truth frame is beyond the end
    samples[3] = torch.tensor([7, 0])       # a trajectory beyond the set -> C
    ids = torch.tensor([-1, 2 ** 40, 2, 3], dtype=torch.int64)
    truth = torch.empty(3, 4, dtype=torch.int64)
    TorchRolloutOps.plan(ids, samples, ds.row0, ds.n, ds.T, DT, truth)
    last = ds.samples[-1]                   # (C, its last start frame 6): frame 8 at step 0, then beyond
    rC = int(ds.row0_host[2])
    assert truth[:, 0].tolist() == [2 * 37, 4 * 37, -1] and truth[:, 1].tolist() == [rC + (int(last[1]) + 2) * 130, -1, -1]
    assert truth[:, 2].tolist() == [-1, -1, -1] and truth[:, 3].tolist() == [rC + 2 * 130, rC + 4 * 130, rC + 6 * 130]


# ---- ABI ----
def test_header_declares_and_binding_lists_the_new_exports():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    assert "#define FASTEGNN_ABI_VERSION 108" in src
    code = re.sub(r"/\*.*?\*/", "", src, flags=re.S)
    for name in NEW_EXPORTS:
        assert re.search(r"\bint " + name + r"\s*\(", code), name
        assert name in K.EXPORTED
    assert K.ABI_VERSION == 108


def test_every_product_library_exports_them_and_refuses_bad_arguments_before_any_launch():
    import ctypes as C
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            assert all(hasattr(L, n) for n in NEW_EXPORTS)
    L, one = K.lib(), C.c_void_p(64)   # (never dereferenced: every call below is refused on the host)
    assert L.fastegnn_rollout_plan(one, -1, one, 1, one, one, one, 1, 2, 3, one, None) == -1 and b"B < 0" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_plan(one, 1, one, 1, one, one, one, 1, 2, 0, one, None) == -1 and b"steps" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_plan(one, 1, one, 1, one, one, one, 1, 0, 3, one, None) == -1 and b"delta_t" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_plan(one, 1, one, 0, one, one, one, 1, 2, 3, one, None) == -1
    assert L.fastegnn_rollout_plan(one, 1, one, 1, one, one, one, 1, 2, 3, None, None) == -1 and b"null" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_plan(None, 0, None, 1, None, None, None, 1, 2, 3, None, None) == 0   # nothing to do
    assert L.fastegnn_rollout_advance(one, -1, 1, one, one, one, None, one, None) == -1
    assert L.fastegnn_rollout_advance(one, 5, 0, one, one, one, None, one, None) == -1 and b"delta_t" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_advance(one, 5, 1, one, one, one, None, None, None) == -1 and b"flag" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_advance(None, 5, 1, one, one, one, None, one, None) == -1
    assert L.fastegnn_rollout_advance(one, 5, 1, one, None, one, None, one, None) == -1
    assert L.fastegnn_rollout_advance(None, 0, 1, None, None, None, None, one, None) == 0          # nothing to do
    assert L.fastegnn_rollout_graph(one, 1, one, one, 5, one, 5, one, 0, one, one, None) == -1 and b"C out of range" in L.fastegnn_last_error()
    assert L.fastegnn_rollout_graph(one, 1, one, one, 5, one, 5, one, (1 << 20) + 1, one, one, None) == -1
    assert L.fastegnn_rollout_graph(one, -1, one, one, 5, one, 5, one, 3, one, one, None) == -1
    assert L.fastegnn_rollout_graph(one, 1, one, one, -5, one, 5, one, 3, one, one, None) == -1
    assert L.fastegnn_rollout_graph(None, 1, one, one, 5, one, 5, one, 3, one, one, None) == -1
    assert L.fastegnn_rollout_graph(one, 1, one, one, 5, one, 5, one, 3, None, one, None) == -1
    assert L.fastegnn_rollout_graph(one, 1, one, one, 5, one, 5, None, 3, one, one, None) == -1    # a score without its truth rows
    assert L.fastegnn_rollout_graph(one, 1, one, None, 5, one, 5, one, 3, one, one, None) == -1
