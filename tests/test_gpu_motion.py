"""Rigid motions on the device (csrc/traj.hip: fastegnn_traj_gather_moved; csrc/rollout.hip: fastegnn_rollout_graph_moved; the rule is
include/fastegnn_hip.h "rigid motions").  The kernels against their torch restatement (tests/motion_ref.py, which applies
``data.apply_motion``): every moved value is a fixed sequence of single fp32 operations, so ``loc_0``, ``loc_t``, ``vel_0`` and
``node_feat`` compare bit for bit (on the int32 view, which also tells -0.0 from +0.0); ``loc_mean`` has the bits ``fastegnn_traj_mean``
gives on a table of the moved rows; ``sse`` is held to the relative 1e-11 of tests/test_gpu_rollout.py.  End to end on the lattice
fixture, whose pair distances keep 1 % of the radius between themselves and the radius, so that the moved and the unmoved batch have the
same edge set whatever the rounding.  No tolerance here was taken from a run.

``edge_attr`` moved against unmoved, 1e-5 relative: the moved coordinates are below 16 with the default ``motion_seed`` (largest |t|
11.6), where fp32 resolves 9.5e-7; a pair's difference carries up to one such unit per coordinate, so the worst case for the shortest
pairs (0.093) is 1.6e-5 and the bound is not guaranteed by that argument alone -- the CPU restatement of this fixture gives 8.6e-6."""
import importlib

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import data as D
from oracle import fastegnn_ref as REF
from tests.motion_ref import (LATTICE_DT, LATTICE_RADIUS, LATTICE_SAMPLES, MovedRolloutOps, MovedTrajOps, lattice_trajectories,
                              sorted_edges, split)
from tests.helpers import OUT_TOL, rel_err
from tests.trajectory_ref import DELTA_T, FIRST, RADIUS, make_trajectories

R = importlib.import_module("fastegnn_amd.rollout")   # (the package attribute of that name is the function)

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 67   # guard bands: sentinel value, elements on either side of every output (odd: the float outputs start unaligned)
NODE_OUT = ("loc_0", "loc_t", "vel_0", "node_feat", "node_attr")
C_ = 3
BATCHES = {
    # small clouds first: the first 1 024-node tile holds four slots and a part of the fifth, the others straddle or lie inside D
    "all four, mixed": [FIRST["A"], FIRST["B"], FIRST["C"], FIRST["D"], FIRST["A"] + 1, FIRST["D"]],
    # two whole tiles inside one slot and a tail of one node
    "the 2 049-node cloud alone": [FIRST["D"]],
}
ZERO_ROWS = {"A": 3, "D": 1030}   # nodes of frame 0 of A and D whose coordinates are all -0.0


@pytest.fixture(scope="module")
def trajectories():
    out = make_trajectories(0)
    for key, node in ZERO_ROWS.items():
        t = [k for k, _, _ in out].index(key)
        out[t][1][0, node, :] = -0.0
    return out


@pytest.fixture(scope="module")
def ds(trajectories):
    return D.TrajectoryDataset(trajectories, C_, DELTA_T, RADIUS, 0.0, device="cuda")


def _banded(shape, dtype):
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * PAD,), SENT, dtype=dtype, device="cuda")
    return buf, buf[PAD:PAD + n].view(shape)


def _bands_intact(out):
    for k, (buf, view) in out.items():
        n = view.numel()
        assert bool((buf[:PAD] == SENT).all()) and bool((buf[PAD + n:] == SENT).all()), k


def _bits(t):
    return t.contiguous().view(torch.int32) if t.dtype == torch.float32 else t


def _motions(kind, B):
    """fp32 [B,12]: ``random`` -- a rotation about all three axes and a translation of scale 5 per slot; ``identity`` -- R = 1, t = 0"""
    if kind == "identity":
        return torch.cat([torch.eye(3).reshape(1, 9).expand(B, 9), torch.zeros(B, 3)], 1).contiguous()
    table, has_t = D._motion_table(B, "xyz", 5.0, 12)
    assert has_t
    return torch.from_numpy(table)


def _direct(ds, ids, N, motion, has_t, spoil=None):
    """plan + the moved gather + the mean over the moved loc_0, every output carved from a larger sentinel-filled buffer; ``spoil``:
    (slot, word, value) written into the slot table between the plan and the gather -> ({name: (buffer, view)}, ptr, slots)"""
    ids_dev, B = torch.tensor(ids, dtype=torch.int64, device="cuda"), len(ids)
    shapes = dict(loc_0=(N, 3), loc_t=(N, 3), vel_0=(N, 3), node_feat=(N, 2), node_attr=(N, 1), loc_mean=(B, 3, C_))
    out = {k: _banded(s, torch.float32) for k, s in shapes.items()}
    out.update(batch=_banded((N,), torch.int64))
    v = {k: view for k, (_, view) in out.items()}
    ptr, slots = torch.empty(B + 1, dtype=torch.int64, device="cuda"), torch.empty(B, 4, dtype=torch.int64, device="cuda")
    ops = D.HipTrajOps
    ops.plan(ids_dev, ds.samples_dev, ds.row0, ds.n, ds.T, ds.kind0, ds.delta_t, ptr, slots)
    if spoil is not None:
        slots[spoil[0], spoil[1]] = spoil[2]
    ops.gather_moved(ptr, slots, N, ds.pos, ds.kind, ds.kind_scaled, *[v[k] for k in NODE_OUT], v["batch"], motion.cuda(), has_t)
    ops.mean_of(ptr, v["loc_0"], v["loc_mean"])
    torch.cuda.synchronize()   # an error of the runtime would surface here
    return out, ptr, slots


def _mirror(ds, ptr, slots, N, motion, has_t):
    """the restatement on host copies, outputs pre-filled with the sentinel"""
    want = dict(loc_0=torch.full((N, 3), float(SENT)), loc_t=torch.full((N, 3), float(SENT)), vel_0=torch.full((N, 3), float(SENT)),
                node_feat=torch.full((N, 2), float(SENT)), node_attr=torch.full((N, 1), float(SENT)),
                batch=torch.full((N,), SENT, dtype=torch.int64))
    MovedTrajOps.gather_moved(ptr.cpu(), slots.cpu(), N, ds.pos.cpu(), ds.kind.cpu(), ds.kind_scaled.cpu(), *[want[k] for k in NODE_OUT],
                              want["batch"], motion, has_t)
    return want


# ---- 1. the moved gather against the restatement ----
@pytest.mark.parametrize("has_t", [0, 1])
@pytest.mark.parametrize("kind", ["random", "identity"])
@pytest.mark.parametrize("name", list(BATCHES))
def test_moved_gather_against_the_restatement(ds, name, kind, has_t):
    ids = BATCHES[name]
    N, B = int(ds._node_cnt[ids].sum()), len(ids)
    motion = _motions(kind, B)
    out, ptr, slots = _direct(ds, ids, N, motion, has_t)
    _bands_intact(out)
    want = _mirror(ds, ptr, slots, N, motion, has_t)
    for k in NODE_OUT + ("batch",):
        assert torch.equal(_bits(out[k][1].cpu()), _bits(want[k])), k
        assert not bool((out[k][1] == SENT).any()), k                        # every element was written
    # loc_mean: the bits of fastegnn_traj_mean on a table that holds the moved rows (slot word 0 = the slot's first row)
    table_slots = torch.zeros(B, 4, dtype=torch.int64, device="cuda")
    table_slots[:, 0] = ptr[:-1]
    mean = torch.empty(B, 3, C_, device="cuda")
    D.HipTrajOps.mean(ptr, table_slots, out["loc_0"][1].contiguous(), mean)
    assert torch.equal(_bits(out["loc_mean"][1]), _bits(mean))
    # the -0.0 coordinates: kept by the identity without a translation, +0.0 once t = 0 is added
    p = ptr.tolist()
    for slot, i in enumerate(ids):
        key = ds.frames[i]
        if key[1] == 0 and key[0] in ZERO_ROWS and kind == "identity":
            row = out["loc_0"][1][p[slot] + ZERO_ROWS[key[0]]]
            assert bool((row == 0).all()), (slot, row)
            assert bool(torch.signbit(row).all()) if has_t == 0 else not bool(torch.signbit(row).any()), (slot, row)
    if kind == "identity" and has_t == 0:                                       # R = 1 reproduces the plain gather's values
        plain = ds.batch(ids)
        assert all(torch.equal(out[k][1], plain[k]) for k in NODE_OUT + ("batch",))


def test_a_slot_whose_source_rows_leave_the_table_writes_nothing(ds):
    ids = BATCHES["all four, mixed"]
    N, B = int(ds._node_cnt[ids].sum()), len(ids)
    motion = _motions("random", B)
    for spoil in ((2, 2, ds.pos.size(0) - 130 + 1), (3, 0, -1), (0, 3, ds.kind.size(0))):   # frame f + dt of C, frame f of D, the kinds of A
        out, ptr, slots = _direct(ds, ids, N, motion, 1, spoil=spoil)
        _bands_intact(out)
        want = _mirror(ds, ptr, slots, N, motion, 1)
        s, e = ptr.tolist()[spoil[0]], ptr.tolist()[spoil[0] + 1]
        for k in NODE_OUT + ("batch",):
            assert torch.equal(_bits(out[k][1].cpu()), _bits(want[k])), (spoil, k)
            assert bool((out[k][1][s:e] == SENT).all()) and not bool((out[k][1][:s] == SENT).any()), (spoil, k)


# ---- 2. fastegnn_rollout_graph_moved ----
SIZES = (1, 255, 256, 257, 1025)   # across the 256-thread workgroup and the 1 024-node tile


@pytest.mark.parametrize("has_t", [0, 1])
def test_graph_moved_against_the_restatement(has_t):
    g = torch.Generator().manual_seed(3)
    ptr = [0] + np.cumsum(SIZES).tolist()
    N, B = ptr[-1], len(SIZES)
    loc, x_new, pos = torch.rand(N, 3, generator=g), torch.rand(N, 3, generator=g) * 9, torch.rand(N + 11, 3, generator=g)
    truth = torch.tensor([N + 11 - 1, 300, 900, -1, 1200 - 1025 + 11], dtype=torch.int64)   # each range lies inside pos; graph 3 has none
    assert all(t < 0 or t + n <= pos.size(0) for t, n in zip(truth.tolist(), SIZES))
    motion = _motions("random", B)
    out = dict(loc_mean=_banded((B, 3, C_), torch.float32), sse=_banded((B,), torch.float64))
    plain = dict(loc_mean=_banded((B, 3, C_), torch.float32), sse=_banded((B,), torch.float64))
    dev = lambda t: t.cuda()  # noqa: E731
    ops = R.HipRolloutOps
    ops.graph_moved(dev(torch.tensor(ptr)), dev(loc), dev(x_new), dev(pos), dev(truth), out["loc_mean"][1], out["sse"][1], dev(motion), has_t)
    ops.graph(dev(torch.tensor(ptr)), dev(loc), dev(x_new), dev(pos), dev(truth), plain["loc_mean"][1], plain["sse"][1])
    torch.cuda.synchronize()
    _bands_intact(out)
    assert torch.equal(_bits(out["loc_mean"][1]), _bits(plain["loc_mean"][1]))          # loc_mean does not see the motion
    got = out["sse"][1].cpu()
    want = torch.empty(B, dtype=torch.float64)
    MovedRolloutOps.graph_moved(torch.tensor(ptr), loc, x_new, pos, truth, torch.empty(B, 3, C_), want, motion, has_t)
    for b, (s, e) in enumerate(zip(ptr, ptr[1:])):
        if int(truth[b]) < 0:
            assert torch.isnan(got[b]) and torch.isnan(want[b])
            continue
        r = int(truth[b])
        exact = ((x_new[s:e].double() - D.apply_motion(pos[r:r + e - s], *split(motion[b], has_t)).double()) ** 2).sum()
        print(f"graph {b} (n = {e - s}): sse {float(got[b])!r}, torch fp64 over the moved truth {float(exact)!r}")
        assert abs(float(got[b]) - float(exact)) <= 1e-11 * float(exact)
        assert abs(float(want[b]) - float(exact)) <= 1e-11 * float(exact)
        assert abs(float(plain["sse"][1][b]) - float(exact)) > 1e-3 * float(exact)      # the unmoved score is another number
    # without a score the motion is not read
    ops.graph_moved(dev(torch.tensor(ptr)), dev(loc), None, None, None, out["loc_mean"][1], None, dev(motion), has_t)
    torch.cuda.synchronize()
    assert torch.equal(_bits(out["loc_mean"][1]), _bits(plain["loc_mean"][1]))


# ---- 3. end to end on the lattice ----
@pytest.fixture(scope="module")
def lattice():
    tr = lattice_trajectories()
    args = dict(samples=LATTICE_SAMPLES, device="cuda")
    plain = D.TrajectoryDataset(tr, C_, LATTICE_DT, LATTICE_RADIUS, 0.0, **args)
    moved = D.TrajectoryDataset(tr, C_, LATTICE_DT, LATTICE_RADIUS, 0.0, rotation="xyz", translation=5.0, **args)
    assert float(moved.motion[:, 9:].abs().max()) < 31.0       # (tests/motion_ref.py: what the fixture's margin was reasoned for)
    return tr, plain, moved


@pytest.fixture(scope="module")
def model():
    cfg = REF.Config(2, 0, 2, 64, C_, n_layers=2)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, C_, device="cuda", n_layers=2)
    m.load_state_dict(REF.init_params(cfg, seed=5, coord_gain=0.05), strict=True)   # tests/test_gpu_properties.py: _models
    return m.cuda().eval()


def test_moved_and_unmoved_batches_have_one_edge_set(lattice):
    _, plain, moved = lattice
    ids = [2, 0, 3, 1]
    a, b = plain.batch(ids), moved.batch(ids)
    N = a["loc_0"].size(0)
    ka, ea = sorted_edges(a["edge_index"], a["edge_attr"], N)
    kb, eb = sorted_edges(b["edge_index"], b["edge_attr"], N)
    assert ka.numel() > 20000 and torch.equal(ka, kb)
    rel = float(((ea - eb).abs() / ea).max())
    print(f"{ka.numel()} edges; edge_attr moved against unmoved: max relative difference {rel:.3e}; largest moved coordinate "
          f"{float(b['loc_0'].abs().max()):.3f}")
    assert rel <= 1e-5
    ptr = a["ptr"].tolist()
    for s, (lo, hi) in enumerate(zip(ptr, ptr[1:])):      # the moved batch is the rule applied to the unmoved one, bit for bit
        Rm, t = split(moved.motion[ids[s]], True)
        assert torch.equal(_bits(D.apply_motion(a["loc_0"][lo:hi], Rm, t)), _bits(b["loc_0"][lo:hi]))
        assert torch.equal(_bits(D.apply_motion(a["vel_0"][lo:hi], Rm)), _bits(b["vel_0"][lo:hi]))


def test_getitem_collate_and_data_loader_see_the_moved_clouds(lattice):
    _, _, moved = lattice
    ids = [1, 3, 0]
    a, b = D.collate([moved[i] for i in ids]), moved.batch(ids)
    for k in ("loc_0", "loc_t", "vel_0", "node_attr", "batch", "ptr"):
        assert torch.equal(_bits(a[k]), _bits(b[k])), k
    N = a["loc_0"].size(0)                                   # and the same pairs, in whatever order the two graph paths leave them
    assert torch.equal(sorted_edges(a["edge_index"], a["edge_attr"], N)[0], sorted_edges(b["edge_index"], b["edge_attr"], N)[0])
    first = next(iter(D.DataLoader(moved, 2)))
    assert torch.equal(first["loc_0"], moved.batch([0, 1])["loc_0"])


def test_the_model_is_equivariant_across_the_two_batches(lattice, model):
    _, plain, moved = lattice
    ids = [2, 0, 3, 1]
    a, b = plain.batch(ids), moved.batch(ids)
    from fastegnn_amd.train import _predict, augment_edge_attr
    with torch.no_grad():
        xa, xb = (_predict(model, d, augment_edge_attr(d.get("edge_attr"), d["loc_0"], d["edge_index"]))[0].clone() for d in (a, b))
    ptr = a["ptr"].tolist()
    for s, (lo, hi) in enumerate(zip(ptr, ptr[1:])):
        want = D.apply_motion(xa[lo:hi], *split(moved.motion[ids[s]], True))
        print(f"slot {s} (n = {hi - lo}): max |apply_motion(x_unmoved) - x_moved| = {float((want - xb[lo:hi]).abs().max()):.3e}; "
              f"max displacement {float((xa[lo:hi] - a['loc_0'][lo:hi]).abs().max()):.3e}")
        assert torch.allclose(want, xb[lo:hi], atol=2e-4, rtol=0.0)
    assert float((xa - a["loc_0"]).abs().max()) > 1e-3                               # the model moves the points: the check sees something


def test_teacher_forced_rollout_in_the_moved_frame(lattice, model):
    """before every step the model is called by hand on the rollout's own batch (tests/test_gpu_rollout.py: the two calls differ in the
    arrival order of the pool sums only, ``OUT_TOL``); the score is the error against the MOVED truth frames"""
    from fastegnn_amd.train import _predict, augment_edge_attr
    tr, _, moved = lattice
    ids, steps = [0, 2, 3], 2
    ro = R.Rollout(model, moved, ids, steps=steps, record=True)
    batch = moved.batch(ids)
    assert all(torch.equal(ro.batch[k], batch[k]) for k in ro.batch.keys())             # step 0 is the moved batch
    for k in range(steps):
        b = ro.batch
        with torch.no_grad():
            hand = _predict(model, b, augment_edge_attr(b.get("edge_attr"), b["loc_0"], b["edge_index"]))[0].clone()
        assert rel_err(ro.step(), hand) <= OUT_TOL
    out = ro.result()
    assert out["stopped"] is None and out["counted"].tolist() == [3, 3]
    want = torch.empty(steps, len(ids), dtype=torch.float64)
    at = 0
    for b, i in enumerate(ids):
        t_, f = (int(v) for v in moved.samples[i])
        n = int(moved.n_host[t_])
        Rm, t = split(moved.motion[i].cpu(), True)
        for k in range(steps):
            truth = D.apply_motion(torch.from_numpy(tr[t_][1][f + (k + 1) * LATTICE_DT]), Rm, t)
            want[k, b] = float(((out["pred"][k, at:at + n].cpu().double() - truth.double()) ** 2).sum()) / (3 * n)
        at += n
    print(f"per_graph {out['per_graph'].tolist()} by hand {want.tolist()}")
    assert float(((out["per_graph"] - want).abs() / want).max()) <= 1e-11
    assert fastegnn_amd.rollout(model, moved, ids, steps)["counted"].tolist() == [3, 3]   # the driver takes the moved dataset as well


# ---- 4. the loader, and the launch count ----
def test_loader_batches_equal_batch(lattice):
    _, _, moved = lattice
    gen = lambda: torch.Generator().manual_seed(8)  # noqa: E731
    order = torch.randperm(len(moved), generator=gen()).tolist()
    got = list(D.TrajectoryLoader(moved, 3, shuffle=True, generator=gen()))
    assert [b.num_graphs for b in got] == [3, 1]
    for i, b in enumerate(got):
        want = moved.batch(order[3 * i:3 * i + 3])
        assert all(torch.equal(b[k], want[k]) for k in want.keys())


def test_the_moved_node_side_is_two_library_calls_and_no_synchronisation(lattice, monkeypatch):
    from fastegnn_amd import _lib as K
    _, plain, moved = lattice
    ids = torch.tensor([2, 1, 0], dtype=torch.int64)
    want = moved.batch(ids)   # warm-up
    calls, lib = [], K.lib()

    class Counting:
        def __getattr__(self, name):
            f = getattr(lib, name)
            if not name.startswith("fastegnn_"):
                return f

            def call(*args):
                calls.append(name)
                return f(*args)
            return call
    monkeypatch.setitem(K._libs, K.LIB_PATH, Counting())
    ids_dev = ids.cuda()
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        got = moved._assemble_nodes(ids_dev, ids.numpy())
        moved_calls = list(calls)
        del calls[:]
        plain._assemble_nodes(ids_dev, ids.numpy())
    finally:
        torch.cuda.set_sync_debug_mode("default")
    # plan, (torch's index_select of the motion rows), the moved gather, the mean: four launches, nothing uploaded or read back
    assert moved_calls == ["fastegnn_traj_plan", "fastegnn_traj_gather_moved", "fastegnn_rollout_graph"]
    assert calls == ["fastegnn_traj_plan", "fastegnn_traj_gather", "fastegnn_traj_mean"]
    assert all(torch.equal(got[k], want[k]) for k in NODE_OUT + ("loc_mean", "batch", "ptr"))
    assert torch.equal(got["motion"][0], moved.motion.index_select(0, ids_dev)) and got["motion"][1] is True
