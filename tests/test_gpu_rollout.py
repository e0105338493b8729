"""Rollouts on the device (csrc/rollout.hip, fastegnn_amd/rollout.py).  The three launches against their torch restatement
(tests/rollout_ref.py): ``vel``, ``node_feat[:,0]`` and the new ``loc`` are single correctly rounded fp32 operations and compare with
``torch.equal``; ``loc_mean`` has the bits ``fastegnn_traj_mean`` gives on the same rows; ``sse`` is a sum of n non-negative fp64 terms
and is held to a relative 1e-11 of torch's fp64 sum (n * 2^-53 < 2e-13 for the sizes here).  The end-to-end tests are teacher-forced:
before every step the model is called by hand on the rollout's own batch, so that neither rounding nor a pair at the radius boundary
can compound; the two calls use the same kernels and differ in the arrival order of the pool sums only (``OUT_TOL``).  No tolerance
here was taken from a run."""
import importlib

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import data as D
from fastegnn_amd import graphs
from fastegnn_amd.train import _predict, augment_edge_attr
from tests.helpers import OUT_TOL, rel_err
from tests.rollout_ref import TorchRolloutOps, equal_with_nan

R = importlib.import_module("fastegnn_amd.rollout")   # (the package attribute of that name is the function)

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 67        # guard bands: sentinel value, elements on either side of every output
SIZES = (1, 255, 256, 257, 1025)   # across the 256-thread workgroup and the 1 024-node tile
C_ = 3


def _banded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _bands_intact(out):
    for k, (buf, view) in out.items():
        n = view.numel()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), k


def _case(seed=0):
    """B = 5 graphs of SIZES back to back: the state, a prediction, a truth table in another order, graph 3 without a truth frame"""
    g = torch.Generator().manual_seed(seed)
    ptr = [0] + np.cumsum(SIZES).tolist()
    N = ptr[-1]
    loc, x_new = torch.rand(N, 3, generator=g), torch.rand(N, 3, generator=g)
    pos = torch.rand(N + 11, 3, generator=g)
    truth = torch.tensor([N + 11 - 1, 300, 900, -1, 1200 - 1025 + 11], dtype=torch.int64)   # each range lies inside pos
    assert all(t < 0 or t + n <= pos.size(0) for t, n in zip(truth.tolist(), SIZES))
    return ptr, N, loc, x_new, pos, truth


def _run_ops(ptr, N, loc, x_new, pos, truth, delta_t, record=True):
    """advance + graph on banded outputs -> ({name: (buffer, view)}, flag value)"""
    B = len(ptr) - 1
    out = dict(loc=_banded((N, 3), torch.float32), vel=_banded((N, 3), torch.float32), node_feat=_banded((N, 2), torch.float32),
               record=_banded((N, 3), torch.float32), loc_mean=_banded((B, 3, C_), torch.float32), sse=_banded((B,), torch.float64))
    v = {k: view for k, (_, view) in out.items()}
    v["loc"].copy_(loc)
    flag = R.FlagWord("cuda")
    ops, dev = R.HipRolloutOps, lambda t: t.cuda()
    ops.advance(dev(x_new), delta_t, v["loc"], v["vel"], v["node_feat"], v["record"] if record else None, flag)
    ops.graph(dev(torch.tensor(ptr)), v["loc"], dev(x_new), dev(pos), dev(truth), v["loc_mean"], v["sse"])
    torch.cuda.synchronize()   # an error of the runtime would surface here
    value = flag.get()
    flag.release()
    return out, value


# ---- 1. the ops against the restatement ----
@pytest.mark.parametrize("delta_t", [1, 3])   # 1/3 is no fp32 number: the multiplication rounds
def test_advance_and_graph_against_the_restatement(delta_t):
    ptr, N, loc, x_new, pos, truth = _case()
    out, flagged = _run_ops(ptr, N, loc, x_new, pos, truth, delta_t)
    _bands_intact(out)
    got = {k: view.cpu() for k, (_, view) in out.items()}
    B = len(SIZES)
    want = dict(loc=loc.clone(), vel=torch.empty(N, 3), node_feat=torch.full((N, 2), float(SENT)), loc_mean=torch.empty(B, 3, C_),
                sse=torch.empty(B, dtype=torch.float64), record=torch.empty(N, 3))
    ref_flag = R.FlagWord("cpu")
    TorchRolloutOps.advance(x_new, delta_t, want["loc"], want["vel"], want["node_feat"], want["record"], ref_flag)
    TorchRolloutOps.graph(torch.tensor(ptr), want["loc"], x_new, pos, truth, want["loc_mean"], want["sse"])
    assert flagged == 0 and ref_flag.get() == 0
    assert torch.equal(got["loc"], want["loc"]) and torch.equal(got["loc"], x_new)
    assert torch.equal(got["vel"], want["vel"]) and torch.equal(got["record"], x_new)
    assert torch.equal(got["node_feat"], want["node_feat"]) and bool((got["node_feat"][:, 1] == SENT).all())   # column 1 is not touched
    # loc_mean: the bits of fastegnn_traj_mean on the same rows (slot word 0 = the graph's first row)
    slots = torch.zeros(B, 4, dtype=torch.int64)
    slots[:, 0] = torch.tensor(ptr[:-1])
    mean = torch.empty(B, 3, C_, device="cuda")
    D.HipTrajOps.mean(torch.tensor(ptr).cuda(), slots.cuda(), out["loc"][1], mean)
    assert torch.equal(out["loc_mean"][1], mean)
    assert float((got["loc_mean"].double() - want["loc_mean"].double()).abs().max()) <= 2.0 ** -23   # the restatement: within the rounding
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        if int(truth[b]) < 0:
            assert torch.isnan(got["sse"][b]) and torch.isnan(want["sse"][b])
            continue
        r = int(truth[b])
        exact = ((x_new[s:e].double() - pos[r:r + e - s].double()) ** 2).sum()
        print(f"graph {b} (n = {e - s}): sse {float(got['sse'][b])!r}, torch fp64 {float(exact)!r}")
        assert abs(float(got["sse"][b]) - float(exact)) <= 1e-11 * float(exact)
        assert abs(float(want["sse"][b]) - float(exact)) <= 1e-11 * float(exact)
    # without a record the same state, and a truth range that leaves pos is NaN, not read
    truth_bad = truth.clone()
    truth_bad[4] = pos.size(0) - 1025 + 1
    again, _ = _run_ops(ptr, N, loc, x_new, pos, truth_bad, delta_t, record=False)
    _bands_intact(again)
    assert bool((again["record"][1] == SENT).all()) and torch.equal(again["vel"][1], out["vel"][1])
    assert torch.isnan(again["sse"][1][4]) and torch.equal(again["sse"][1][:3], out["sse"][1][:3])
    assert torch.equal(again["loc_mean"][1], out["loc_mean"][1])                     # two calls, identical bits


# ---- 2. the non-finite flag ----
def test_a_non_finite_component_sets_the_flag_and_keeps_the_state():
    ptr, N, loc, x_new, pos, truth = _case(1)
    x_bad = x_new.clone()
    x_bad[5, 1], x_bad[N - 1, 2] = float("nan"), float("inf")
    out, flagged = _run_ops(ptr, N, loc, x_bad, pos, truth, 2)
    _bands_intact(out)
    assert flagged == 1
    got = {k: view.cpu() for k, (_, view) in out.items()}
    want = dict(loc=loc.clone(), vel=torch.empty(N, 3), node_feat=torch.full((N, 2), float(SENT)))
    TorchRolloutOps.advance(x_bad, 2, want["loc"], want["vel"], want["node_feat"], None, R.FlagWord("cpu"))
    assert all(torch.equal(got[k], want[k]) for k in want)
    assert got["loc"][5, 1] == loc[5, 1] and got["loc"][N - 1, 2] == loc[N - 1, 2] and got["vel"][5, 1] == 0 and got["vel"][N - 1, 2] == 0
    assert got["loc"][5, 0] == x_bad[5, 0] and bool(torch.isfinite(got["loc"]).all()) and bool(torch.isfinite(got["node_feat"]).all())
    assert equal_with_nan(got["record"], x_bad)                                       # the record keeps the raw value,
    assert torch.isnan(got["sse"][1]) and torch.isinf(got["sse"][4])                  # and so does the score (graphs 1 and 4)
    assert bool(torch.isfinite(got["loc_mean"]).all())
    _, flagged = _run_ops(ptr, N, loc, x_new, pos, truth, 2)
    assert flagged == 0


# ---- 3. the plan ----
def _smooth_trajectories(shapes, seed=0):
    """points in the unit cube with a smooth small drift"""
    rng = np.random.default_rng(seed)
    out = []
    for key, T, n in shapes:
        p0, v, a = rng.random((n, 3)), 0.004 * rng.standard_normal((n, 3)), 0.0005 * rng.standard_normal((n, 3))
        t = np.arange(T, dtype=np.float64)[:, None, None]
        out.append((key, (p0[None] + v[None] * t + a[None] * t * t).astype(np.float32), rng.choice(np.asarray([1.0, 3.0], np.float32), size=n)))
    return out


E2E_SHAPES = (("P", 9, 37), ("Q", 9, 300))
E2E_SAMPLES = np.asarray([[0, 0], [1, 3], [1, 0]])
E2E_RADIUS, E2E_DT, E2E_STEPS = 0.185, 2, 4


@pytest.fixture(scope="module")
def ds():
    return D.TrajectoryDataset(_smooth_trajectories(E2E_SHAPES), C_, E2E_DT, E2E_RADIUS, 0.25, samples=E2E_SAMPLES, device="cuda")


@pytest.fixture(scope="module")
def model():
    torch.manual_seed(0)
    return fastegnn_amd.FastEGNN(2, 0, 2, 64, C_, device="cuda", n_layers=2)


def test_plan_against_the_restatement(ds):
    samples = ds.samples_dev.clone()
    samples[2] = torch.tensor([5, 99])      # a trajectory beyond the set, a frame beyond T
    for ids, table in (([0, 1, 2], ds.samples_dev), ([2, 2, 0, 1, 1], ds.samples_dev), ([-1, 3, 2 ** 40, 2], samples)):
        for steps in (1, 6):
            ids_dev = torch.tensor(ids, dtype=torch.int64, device="cuda")
            buf, got = _banded((steps, len(ids)), torch.int64)
            R.HipRolloutOps.plan(ids_dev, table, ds.row0, ds.n, ds.T, ds.delta_t, got)
            torch.cuda.synchronize()
            want = torch.empty(steps, len(ids), dtype=torch.int64)
            TorchRolloutOps.plan(ids_dev.cpu(), table.cpu(), ds.row0.cpu(), ds.n.cpu(), ds.T.cpu(), ds.delta_t, want)
            assert torch.equal(got.cpu(), want), (ids, steps)
            _bands_intact({"truth_rows": (buf, got)})
            assert int(got.max()) + 300 <= ds.pos.size(0) and int(got.min()) >= -1
    # the table by hand: sample (Q, 3) at stride 2 has frames 5 and 7, then none
    got = torch.empty(4, 3, dtype=torch.int64, device="cuda")
    R.HipRolloutOps.plan(torch.arange(3, device="cuda"), ds.samples_dev, ds.row0, ds.n, ds.T, 2, got)
    q0 = 9 * 37
    assert got.cpu().tolist() == [[2 * 37, q0 + 5 * 300, q0 + 2 * 300], [4 * 37, q0 + 7 * 300, q0 + 4 * 300], [6 * 37, -1, q0 + 6 * 300],
                                  [8 * 37, -1, q0 + 8 * 300]]


# ---- 4. end to end, teacher-forced ----
def _by_hand(model, batch):
    with torch.no_grad():
        return _predict(model, batch, augment_edge_attr(batch.get("edge_attr"), batch["loc_0"], batch["edge_index"]))[0].clone()


def _check_edges(batch, radius, cutoff_rate):
    ei, dist, edge_ptr = graphs.radius_graph_batch(batch["loc_0"], batch["ptr"], radius)
    ei, dist, _ = graphs.cutoff_edges_batch(ei, dist, edge_ptr, cutoff_rate)
    assert torch.equal(batch["edge_index"], ei) and torch.equal(batch["edge_attr"], dist.unsqueeze(-1))


def _per_graph_mse(ds, ids, pred, steps):
    """fp64 per-graph MSE of the recorded predictions against ds.pos, NaN where the trajectory has no such frame"""
    want = torch.full((steps, len(ids)), float("nan"), dtype=torch.float64)
    at = 0
    for b, i in enumerate(ids):
        t, f = (int(v) for v in ds.samples[i])
        n, r0 = int(ds.n_host[t]), int(ds.row0_host[t])
        for k in range(steps):
            frame = f + (k + 1) * ds.delta_t
            if frame < int(ds.T_host[t]):
                d = pred[k, at:at + n].double() - ds.pos[r0 + frame * n:r0 + (frame + 1) * n].double()
                want[k, b] = float((d ** 2).sum()) / (3 * n)
        at += n
    return want


def test_teacher_forced_rollout(ds, model):
    ids = [0, 1, 2]
    model.eval()
    ro = R.Rollout(model, ds, ids, steps=E2E_STEPS, record=True)
    inv = torch.tensor(1.0 / E2E_DT, dtype=torch.float32, device="cuda")
    prev = None
    for k in range(E2E_STEPS):
        batch = ro.batch
        if k >= 1:
            assert torch.equal(batch["loc_0"], prev)
            assert torch.equal(batch["vel_0"], (prev - before) * inv) and bool(torch.isfinite(batch["node_feat"]).all())
        _check_edges(batch, E2E_RADIUS, 0.25)
        assert batch["edge_index"].size(1) > 0
        hand, before = _by_hand(model, batch), batch["loc_0"].clone()
        prev = ro.step().clone()
        err = rel_err(prev, hand)
        print(f"step {k}: {batch['edge_index'].size(1)} edges, rel_err(step, by hand) = {err:.3e}")
        assert err <= OUT_TOL and ro.k == k + 1
    assert ro.batch is None and ro.stopped is None
    out = ro.result()
    assert out["stopped"] is None and out["counted"].tolist() == [3, 3, 2, 2] and torch.equal(out["pred"][-1], prev)
    want = _per_graph_mse(ds, ids, out["pred"], E2E_STEPS)
    assert torch.equal(torch.isnan(out["per_graph"]), torch.isnan(want))
    have = ~torch.isnan(want)
    assert float(((out["per_graph"] - want)[have].abs() / want[have]).max()) <= 1e-11
    for k in range(E2E_STEPS):
        assert abs(float(out["mse"][k]) - float(want[k][have[k]].mean())) <= 1e-11 * float(want[k][have[k]].mean())


# ---- 5. step 0 equals the loader ----
def test_step_0_equals_the_loader(ds, model):
    ids = [2, 0]
    out = fastegnn_amd.rollout(model, ds, ids, 1, record=True)
    batch = ds.batch(ids)
    first = R.Rollout(model, ds, ids, steps=1).batch
    assert all(torch.equal(first[k], batch[k]) for k in first.keys()) and list(first.keys()) == [k for k in batch.keys() if k != "loc_t"]
    model.eval()
    assert rel_err(out["pred"][0], _by_hand(model, batch)) <= OUT_TOL
    want = _per_graph_mse(ds, ids, out["pred"], 1)
    assert float(((out["per_graph"] - want).abs() / want).max()) <= 1e-11 and out["counted"].tolist() == [2]
    model.train()
    fastegnn_amd.rollout(model, ds, ids, 1)
    assert model.training                                                            # the mode is restored


# ---- 6. EGNN by its own signature ----
def test_egnn_dispatch(ds):
    torch.manual_seed(0)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
    m.eval()
    ro = R.Rollout(m, ds, [0], steps=2, record=True)
    batch = ro.batch
    _check_edges(batch, E2E_RADIUS, 0.25)
    hand = _by_hand(m, batch)
    assert rel_err(ro.step(), hand) <= OUT_TOL
    ro.step()
    out = ro.result()
    assert out["stopped"] is None and bool(torch.isfinite(out["pred"]).all()) and out["counted"].tolist() == [1, 1]
    assert bool(torch.isfinite(out["mse"]).all())
