"""Times a rollout of a FastEGNN over Water-3D-sized clouds on one GPU, two ways that alternate in one process (host wall clock around a
whole rollout that ends in a device synchronise; the median of REPEATS rollouts after WARM warm-ups with [min .. max], per step):

  (a) by hand         the loop a user writes on the same tree: ds.batch for step 0, then per step augment + forward, torch ops for the
                      velocity, the speed feature and the per-graph mean, B slices + cat for the truth frame, ONE .item() for the error,
                      the batched graph build
  (b) rollout()       fastegnn_amd.rollout: the same forward and graph build, the state update as two launches, no read-back per step
                      besides the graph build's

and the split of (b)'s step into graph build / augment + forward / state update, from a third pass with a device synchronise after
every section (sections timed that way add up to more than an unsynchronised step), plus the two state-update launches under the
library's event pairs.  Shape: 4 trajectories x 21 frames of 7600..8400 particles in a 0.42^3 box (a random walk of 0.001 per frame),
delta_t = 2, 20 rollouts (start frames 0..4 of every trajectory) of 8 steps, r = 0.035.  Prints what profiles/rollout.txt holds.

    python tools/gpu_rollout_timing.py [output file]
"""
import importlib
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastegnn_amd  # noqa: E402
from fastegnn_amd import _lib as K  # noqa: E402
from fastegnn_amd import data as D  # noqa: E402
from fastegnn_amd.train import _predict, augment_edge_attr  # noqa: E402

R = importlib.import_module("fastegnn_amd.rollout")

REPEATS, WARM, C = 15, 2, 3
N_TRAJ, T, DELTA_T, RADIUS, STARTS, STEPS = 4, 21, 2, 0.035, 5, 8


def make_trajectories(seed):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(N_TRAJ):
        n = int(rng.integers(7600, 8401))
        steps = rng.normal(0.0, 0.001, size=(T, n, 3)).astype(np.float32)
        steps[0] = rng.random((n, 3), dtype=np.float32) * 0.42
        out.append((f"traj{t}", np.cumsum(steps, 0, dtype=np.float32), rng.integers(1, 3, size=n).astype(np.float32)))
    return out


def by_hand(model, ds, ids):
    """(a) -> the per-step errors (mean over all nodes and components, what one .item() per step gives)"""
    b = ds.batch(ids)
    loc, vel, feat, mean, ptr, batch = b["loc_0"], b["vel_0"], b["node_feat"].clone(), b["loc_mean"], b["ptr"], b["batch"]
    ei, ea = b["edge_index"], b["edge_attr"]
    ptr_host = [0] + np.cumsum(ds._node_cnt[ids]).tolist()
    counts = (ptr[1:] - ptr[:-1]).to(torch.float32).unsqueeze(-1)
    data, errs = dict(node_feat=feat, batch=batch, ptr=ptr), []
    for k in range(STEPS):
        data.update(loc_0=loc, vel_0=vel, loc_mean=mean, edge_index=ei)
        x = _predict(model, data, augment_edge_attr(ea, loc, ei))[0]
        truth = []
        for i in ids:
            t, f = (int(v) for v in ds.samples[i])
            n, r0, frame = int(ds.n_host[t]), int(ds.row0_host[t]), f + (k + 1) * ds.delta_t
            truth.append(ds.pos[r0 + frame * n:r0 + (frame + 1) * n])
        errs.append((x - torch.cat(truth, 0)).pow(2).mean().item())
        vel = (x - loc) / ds.delta_t
        feat[:, 0] = vel.pow(2).sum(-1).sqrt()
        loc = x
        mean = (torch.zeros(len(ids), 3, device=loc.device).index_add_(0, batch, loc) / counts).unsqueeze(-1).repeat(1, 1, C)
        if k + 1 < STEPS:
            ei, dist = D.HipTrajOps.edges(loc, ptr, ptr_host, ds.radius, ds.cutoff_rate)
            ea = dist.unsqueeze(-1)
    return errs


def sections(model, ds, ids):
    """(b)'s step with a synchronise after every section -> seconds per rollout in (graph build, augment + forward, state update)"""
    sync, clock = torch.cuda.synchronize, time.perf_counter
    t = [0.0, 0.0, 0.0]
    ro = R.Rollout(model, ds, ids, steps=STEPS)
    ops, s = R.HipRolloutOps, ro._state
    for k in range(STEPS):
        sync()
        t0 = clock()
        data = ro.batch
        x = _predict(model, data, augment_edge_attr(data["edge_attr"], data["loc_0"], data["edge_index"]))[0]
        sync()
        t1 = clock()
        ops.advance(x, ds.delta_t, s["loc_0"], s["vel_0"], s["node_feat"], None, ro._flag)
        ops.graph(s["ptr"], s["loc_0"], x, ds.pos, ro._truth[k], s["loc_mean"], ro._sse[k])
        sync()
        t2 = clock()
        ro._build_graph()
        sync()
        t3 = clock()
        t[0] += t3 - t2
        t[1] += t1 - t0
        t[2] += t2 - t1
    return t


def launches_us(model, ds, ids, runs=20):
    """advance and graph by themselves under the library's per-launch HIP events"""
    ro = R.Rollout(model, ds, ids, steps=1)
    ops, s = R.HipRolloutOps, ro._state
    x = s["loc_0"] + 0.001

    def measure(call):
        for _ in range(3):
            call()
        torch.cuda.synchronize()
        K.lib().fastegnn_profile_enable(1)
        K.profile_collect()
        for _ in range(runs):
            call()
        K.lib().fastegnn_profile_enable(0)
        ms, n = K.profile_collect()["misc"]
        return ms / n * 1e3
    a = measure(lambda: ops.advance(x, ds.delta_t, s["loc_0"], s["vel_0"], s["node_feat"], None, ro._flag))
    g = measure(lambda: ops.graph(s["ptr"], s["loc_0"], x, ds.pos, ro._truth[0], s["loc_mean"], ro._sse[0]))
    return a, g, x.size(0)


def fmt(name, ts):
    per = [v / STEPS * 1e3 for v in ts]
    return f"    {name:<14} median {statistics.median(per):8.3f} ms per step   [{min(per):.3f} .. {max(per):.3f}]   of {len(ts)} rollouts after {WARM} warm-ups"


def main():
    ds = D.TrajectoryDataset(make_trajectories(3), C, DELTA_T, RADIUS, 0.0, device="cuda",
                             samples=np.asarray([(t, f) for t in range(N_TRAJ) for f in range(STARTS)]))
    ids = np.arange(len(ds))
    torch.manual_seed(0)
    model = fastegnn_amd.FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2, hidden_nf=64, virtual_channels=C, device="cuda",
                                  n_layers=4)
    model.eval()
    ts, sec = {"(a) by hand": [], "(b) rollout()": []}, []
    with torch.no_grad():
        for it in range(WARM + REPEATS):
            for name in ts:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                got = by_hand(model, ds, ids) if name.startswith("(a)") else fastegnn_amd.rollout(model, ds, ids, STEPS)
                torch.cuda.synchronize()
                if it >= WARM:
                    ts[name].append(time.perf_counter() - t0)
                if name.startswith("(a)"):
                    hand = got
                else:
                    res = got
            s = sections(model, ds, ids)
            if it >= WARM:
                sec.append(s)
        a_us, g_us, N = launches_us(model, ds, ids)
        first = ds.batch(ids)
    a, b = ts["(a) by hand"], ts["(b) rollout()"]
    n = torch.tensor(ds._node_cnt[ids], dtype=torch.float64)
    pooled = [float((res["per_graph"][k] * n).sum() / n.sum()) for k in range(STEPS)]   # (a)'s error is the mean over all nodes
    drift = max(abs(p - h) / h for p, h in zip(pooled, hand))
    med = [statistics.median(s[i] for s in sec) / STEPS * 1e3 for i in range(3)]
    rng = [(min(s[i] for s in sec) / STEPS * 1e3, max(s[i] for s in sec) / STEPS * 1e3) for i in range(3)]
    out = [f"device: {torch.cuda.get_device_name(0)}; host wall clock around one rollout of {STEPS} steps ending in a device synchronise; "
           f"the two ways alternate in one process",
           f"Water-3D-like: {N_TRAJ} trajectories x {T} frames x {ds.n_host.tolist()} particles in a 0.42^3 box, delta_t = {DELTA_T}, "
           f"{len(ids)} rollouts, r = {RADIUS}: {first.num_nodes} nodes, {first['edge_index'].size(1)} edges at step 0 "
           f"({first['edge_index'].size(1) / first.num_nodes:.1f} per node)",
           "  FastEGNN hidden 64, 4 layers, C = 3, untrained, eval() under no_grad (the forward-only path)",
           f"  rollout(): stopped = {res['stopped']}, counted = {res['counted'].tolist()}, mse[0] = {float(res['mse'][0]):.6e}, "
           f"mse[{STEPS - 1}] = {float(res['mse'][STEPS - 1]):.6e}; node-weighted, against the hand loop's per-step error: "
           f"largest relative difference {drift:.2e} (the two loops round the state differently and are not teacher-forced)",
           "  whole rollout, per step:", fmt("(a) by hand", a), fmt("(b) rollout()", b),
           f"    (b) [{min(b) / STEPS * 1e3:.3f} .. {max(b) / STEPS * 1e3:.3f}] against (a) [{min(a) / STEPS * 1e3:.3f} .. "
           f"{max(a) / STEPS * 1e3:.3f}]: wholly below: {max(b) < min(a)}; ranges overlap: {not (max(b) < min(a) or max(a) < min(b))}",
           "  (b)'s step by section, a device synchronise after each (median [min .. max] ms per step):",
           f"    graph build {med[0]:.3f} [{rng[0][0]:.3f} .. {rng[0][1]:.3f}]   augment + forward {med[1]:.3f} [{rng[1][0]:.3f} .. "
           f"{rng[1][1]:.3f}]   state update (2 launches) {med[2]:.3f} [{rng[2][0]:.3f} .. {rng[2][1]:.3f}]",
           f"  the state update's launches under the library's event pairs (N = {N}, B = {len(ids)}, mean of 20): advance {a_us:.1f} us, "
           f"graph {g_us:.1f} us",
           "  not measured: a trained model, the wide path, EGNN / FastRF, clouds that do not fit the Infinity Cache, more than one GPU"]
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
