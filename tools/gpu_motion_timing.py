"""Times one epoch of ``TrajectoryLoader`` over the Water-3D-like set of tools/gpu_trajectory_timing.py (same shape, same protocol: host
wall clock around an epoch that ends in one device synchronise, the loaders alternating in one process, the median of 15 epochs
after 2 warm-ups with [min .. max]) with and without a rigid motion per sample:

  (u) unmoved            TrajectoryDataset(...)                                       plan, gather, mean
  (r) rotation           TrajectoryDataset(..., rotation="xyz")                       plan, index_select, gather_moved, mean
  (m) rotation + shift   TrajectoryDataset(..., rotation="xyz", translation=0.21)     the same four launches, has_t = 1

The three datasets hold the same positions (three copies of 6.6 MB).  Also the gather launches by themselves under the library's event
pairs.  Prints what profiles/trajectory_motion.txt holds.

    python tools/gpu_motion_timing.py [output file]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from gpu_trajectory_timing import BATCH, C, DELTA_T, RADIUS, epoch_times, line, make_trajectories  # noqa: E402
from fastegnn_amd import _lib as K  # noqa: E402
from fastegnn_amd import data as D  # noqa: E402


def launch_us(call, runs=20):
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


def gather_launches(ds, moved, ids_dev, ids_host):
    """(plain gather, moved gather without t, with t, the [N,3] mean) in us per launch, outputs allocated once"""
    out = ds._assemble_nodes(ids_dev, ids_host)
    slots = torch.empty((ids_host.size, 4), dtype=torch.int64, device="cuda")
    ops = D.HipTrajOps
    ops.plan(ids_dev, ds.samples_dev, ds.row0, ds.n, ds.T, ds.kind0, ds.delta_t, out["ptr"], slots)
    rows = moved.motion.index_select(0, ids_dev)
    args = (out["ptr"], slots, out["batch"].numel(), ds.pos, ds.kind, ds.kind_scaled, *[out[k] for k in D._NODE_KEYS], out["batch"])
    return (launch_us(lambda: ops.gather(*args)), launch_us(lambda: ops.gather_moved(*args, rows, False)),
            launch_us(lambda: ops.gather_moved(*args, rows, True)), launch_us(lambda: ops.mean_of(out["ptr"], out["loc_0"], out["loc_mean"])),
            launch_us(lambda: ops.mean(out["ptr"], slots, ds.pos, out["loc_mean"])))


def main():
    trajectories = make_trajectories(3)
    make = lambda **kw: D.TrajectoryDataset(trajectories, C, DELTA_T, RADIUS, 0.0, device="cuda", **kw)  # noqa: E731
    sets = [("(u) unmoved", make()), ("(r) rotation", make(rotation="xyz")), ("(m) rotation + shift", make(rotation="xyz", translation=0.21))]
    gen = lambda: torch.Generator().manual_seed(9)  # noqa: E731
    loaders = [(name, D.TrajectoryLoader(ds, BATCH, shuffle=True, generator=gen())) for name, ds in sets]
    nb = len(loaders[0][1])
    first = [next(iter(loader)) for _, loader in loaders]
    out = [f"device: {torch.cuda.get_device_name(0)}; host wall clock around one epoch ending in one device synchronise; the three loaders "
           f"alternate in one process",
           f"Water-3D-like (tools/gpu_trajectory_timing.py): {len(trajectories)} trajectories x 17 frames x {sets[0][1].n_host.tolist()} "
           f"particles in a 0.42^3 box, delta_t = {DELTA_T}: {len(sets[0][1])} samples, r = {RADIUS}, batch size {BATCH}",
           f"  {nb} batches per epoch; first batch: {first[0].num_nodes} nodes; edges unmoved / rotated / rotated + shifted: "
           + " / ".join(str(b['edge_index'].size(1)) for b in first)
           + " (pairs within rounding of the radius may fall on either side in another frame)"]
    ids = torch.randperm(len(sets[0][1]), generator=torch.Generator().manual_seed(4))[:BATCH]
    g, g0, g1, m_of, m = gather_launches(sets[0][1], sets[2][1], ids.cuda(), ids.numpy())
    out.append(f"  one batch of {BATCH} samples under the library's event pairs (HIP events around the launch, mean of 20): gather {g:.1f} us, "
               f"gather_moved {g0:.1f} us without t, {g1:.1f} us with t; mean over pos {m:.1f} us, mean over the moved loc_0 {m_of:.1f} us")
    out.append("  loader alone:")
    ts = epoch_times(loaders, lambda batch: None)
    out += [line(name, ts[name], nb) for name, _ in loaders]
    u = ts[loaders[0][0]]
    for name, _ in loaders[1:]:
        x = ts[name]
        apart = min(x) > max(u) or max(x) < min(u)
        out.append(f"    {name} [{min(x) * 1e3:.3f} .. {max(x) * 1e3:.3f}] against (u) [{min(u) * 1e3:.3f} .. {max(u) * 1e3:.3f}]: ranges "
                   f"{'apart' if apart else 'overlap: no difference is claimed'}; at the medians "
                   f"{(statistics.median(x) - statistics.median(u)) / nb * 1e3:+.3f} ms per batch")
    out.append("  not measured: the loader with a train_step behind it, tables beyond the Infinity Cache, the protein shape")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
