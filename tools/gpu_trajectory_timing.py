"""Times one epoch of three ways to the same Water-3D-like batches on one GPU (the protocol of tools/gpu_loader_timing.py: host wall clock
around an epoch that ends in one device synchronise, the loaders alternating in one process, the median of EPOCHS epochs after WARM
warm-ups with [min .. max]), each alone and with an eager train_step per batch:

  (a) water3d_batch   data.water3d_batch called per batch on slices of the device-resident position table: B slices, the per-cloud
                      feature and mean evaluations, six torch.cat, two uploads -- the only way to such a batch without stored frames
  (b) PackedLoader    over a PackedDataset of the stored frames (every sample materialised with its edge list)
  (c) TrajectoryLoader  positions and kinds on the device, three launches for the node side, the batched graph build per batch

Shape: 4 trajectories x 17 frames of 7600..8400 particles in a 0.42^3 box (a random walk of 0.001 per frame), delta_t = 2: 60 samples,
r = 0.035, batch size 20.  Also: device bytes per sample of (b) and (c) from the tensors' sizes, and the gather launch under the library's
event pair.  Prints what profiles/trajectory_loader.txt holds.

    python tools/gpu_trajectory_timing.py [output file]
"""
import math
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
from fastegnn_amd.train import FusedAdam, MMDSampler, train_step  # noqa: E402

EPOCHS, WARM, C = 15, 2, 3
N_TRAJ, T, DELTA_T, RADIUS, BATCH = 4, 17, 2, 0.035, 20


def make_trajectories(seed):
    rng = np.random.default_rng(seed)
    out = []
    for t in range(N_TRAJ):
        n = int(rng.integers(7600, 8401))
        steps = rng.normal(0.0, 0.001, size=(T, n, 3)).astype(np.float32)
        steps[0] = rng.random((n, 3), dtype=np.float32) * 0.42
        out.append((f"traj{t}", np.cumsum(steps, 0, dtype=np.float32), rng.integers(1, 3, size=n).astype(np.float32)))
    return out


class SliceLoader:
    """(a): the order of the other two loaders; every batch is water3d_batch of slices of the dataset's device tables"""

    def __init__(self, ds, batch_size, generator):
        self.ds, self.batch_size, self.generator = ds, batch_size, generator

    def __len__(self):
        return math.ceil(len(self.ds) / self.batch_size)

    def __iter__(self):
        ds = self.ds
        order = torch.randperm(len(ds), generator=self.generator).tolist()
        for i in range(len(self)):
            loc_0, vel_0, loc_t, kind, ptr = [], [], [], [], [0]
            for j in order[i * self.batch_size:(i + 1) * self.batch_size]:
                t, f = (int(v) for v in ds.samples[j])
                n, r0, k0 = int(ds.n_host[t]), int(ds.row0_host[t]), int(ds.kind0_host[t])
                at = lambda frame: ds.pos[r0 + frame * n:r0 + (frame + 1) * n]  # noqa: E731
                loc_0.append(at(f))
                vel_0.append(at(f + 1) - at(f))
                loc_t.append(at(f + ds.delta_t))
                kind.append(ds.kind[k0:k0 + n])
                ptr.append(ptr[-1] + n)
            yield D.water3d_batch(torch.cat(loc_0, 0), torch.cat(vel_0, 0), torch.cat(loc_t, 0), torch.cat(kind, 0), ptr, C, ds.radius,
                                  ds.cutoff_rate)


def epoch_times(loaders, body):
    ts = {name: [] for name, _ in loaders}
    for it in range(WARM + EPOCHS):
        for name, loader in loaders:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in loader:
                body(batch)
            torch.cuda.synchronize()
            if it >= WARM:
                ts[name].append(time.perf_counter() - t0)
    return ts


def line(name, ts, n_batches):
    med = statistics.median(ts)
    return (f"    {name:<18} median {med * 1e3:9.3f} ms per epoch ({med / n_batches * 1e3:8.3f} ms per batch)   "
            f"[{min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f}] ms   of {len(ts)} epochs after {WARM} warm-ups")


def verdict(ts, nb):
    a, b, c = (ts[k] for k in ("(a) water3d_batch", "(b) PackedLoader", "(c) TrajectoryLoader"))
    return (f"    (c) [{min(c) * 1e3:.3f} .. {max(c) * 1e3:.3f}] against (a) [{min(a) * 1e3:.3f} .. {max(a) * 1e3:.3f}]: wholly below: "
            f"{max(c) < min(a)};  (c) - (b) at the medians: {(statistics.median(c) - statistics.median(b)) / nb * 1e3:.3f} ms per batch")


def gather_us(ds, ids_dev, ids_host, runs=20):
    """the gather launch of one batch by itself (outputs allocated once, the plan run once) under the library's per-launch HIP events"""
    out = ds._assemble_nodes(ids_dev, ids_host)
    slots = torch.empty((ids_host.size, 4), dtype=torch.int64, device="cuda")
    ops = D.HipTrajOps
    ops.plan(ids_dev, ds.samples_dev, ds.row0, ds.n, ds.T, ds.kind0, ds.delta_t, out["ptr"], slots)

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
        return ms / n * 1e3, n
    g = measure(lambda: ops.gather(out["ptr"], slots, out["batch"].numel(), ds.pos, ds.kind, ds.kind_scaled,
                                   *[out[k] for k in D._NODE_KEYS], out["batch"]))
    m = measure(lambda: ops.mean(out["ptr"], slots, ds.pos, out["loc_mean"]))
    p = measure(lambda: ops.plan(ids_dev, ds.samples_dev, ds.row0, ds.n, ds.T, ds.kind0, ds.delta_t, out["ptr"], slots))
    nbytes = sum(out[k].numel() * out[k].element_size() for k in D._NODE_KEYS + ("batch",)) + out["batch"].numel() * 44
    return g, m, p, nbytes


def main():
    trajectories = make_trajectories(3)
    ds = D.TrajectoryDataset(trajectories, C, DELTA_T, RADIUS, 0.0, device="cuda")
    frames = [ds[i] for i in range(len(ds))]
    packed = D.PackedDataset(frames)
    gen = lambda: torch.Generator().manual_seed(9)  # noqa: E731
    loaders = [("(a) water3d_batch", SliceLoader(ds, BATCH, gen())),
               ("(b) PackedLoader", D.PackedLoader(packed, BATCH, shuffle=True, generator=gen())),
               ("(c) TrajectoryLoader", D.TrajectoryLoader(ds, BATCH, shuffle=True, generator=gen()))]
    nb = len(loaders[2][1])
    exact = ("loc_0", "loc_t", "vel_0", "node_attr", "batch", "ptr", "edge_index", "edge_attr")
    same, ulps, first = True, 0.0, None
    for a, c in zip(loaders[0][1], loaders[2][1]):
        first = first or c
        same &= list(a.keys()) == list(c.keys()) and all(torch.equal(a[k], c[k]) for k in exact)
        same &= torch.equal(a["node_feat"][:, 1], c["node_feat"][:, 1])
        x, y = a["node_feat"][:, 0].cpu().numpy(), c["node_feat"][:, 0].cpu().numpy()
        ulps = max(ulps, float((np.abs(x - y) / np.spacing(np.abs(x))).max()))
    out = [f"device: {torch.cuda.get_device_name(0)}; host wall clock around one epoch ending in one device synchronise; the three loaders "
           f"alternate in one process",
           f"Water-3D-like: {N_TRAJ} trajectories x {T} frames x {ds.n_host.tolist()} particles in a 0.42^3 box, delta_t = {DELTA_T}: {len(ds)} "
           f"samples, r = {RADIUS}, batch size {BATCH}",
           f"  {nb} batches per epoch; first batch: {first.num_nodes} nodes, {first['edge_index'].size(1)} edges; TrajectoryLoader's batches "
           f"equal water3d_batch's (torch.equal: {', '.join(exact)}, node_feat[:,1]): {same}; node_feat[:,0] differs by at most {ulps:.1f} "
           f"units in the last place"]
    b_bytes = sum(t.numel() * t.element_size() for t in packed.tables.values())
    b_bytes += (packed.node_ptr.numel() + packed.edge_ptr.numel()) * 8
    c_tensors = (ds.pos, ds.kind, ds.kind_scaled, ds.samples_dev, ds.row0, ds.n, ds.T, ds.kind0)
    c_bytes = sum(t.numel() * t.element_size() for t in c_tensors)
    out.append(f"  device bytes per sample, from the tensors' sizes: (b) PackedDataset {b_bytes / len(ds) / 1e3:.1f} KB (tables and offsets; "
               f"+ 16 B per edge with graphs=), (c) TrajectoryDataset {c_bytes / len(ds) / 1e3:.1f} KB ({T} frames shared by "
               f"{len(ds) // N_TRAJ} samples per trajectory): a factor of {b_bytes / c_bytes:.1f}")
    ids = torch.randperm(len(ds), generator=torch.Generator().manual_seed(4))[:BATCH]
    (g_us, g_n), (m_us, m_n), (p_us, p_n), nbytes = gather_us(ds, ids.cuda(), ids.numpy())
    out.append(f"  one batch of {BATCH} samples under the library's event pairs (HIP events around the launch, mean of {g_n}): plan {p_us:.1f} us, "
               f"gather {g_us:.1f} us = {nbytes / g_us / 1e3:.0f} GB/s read + written ({nbytes / 1e6:.2f} MB), mean {m_us:.1f} us")
    out.append("  loader alone:")
    ts = epoch_times(loaders, lambda batch: None)
    out += [line(k, ts[k], nb) for k, _ in loaders] + [verdict(ts, nb)]
    model = fastegnn_amd.FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2, hidden_nf=64, virtual_channels=C, device="cuda",
                                  n_layers=4)
    opt, smp = FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-12), MMDSampler(0)
    out.append("  loader + eager train_step (FastEGNN hidden 64, 4 layers, C = 3, device-side MMD sample):")
    ts = epoch_times(loaders, lambda batch: train_step(model, opt, batch, None, sigma=1.0, weight=0.01, sampler=smp, num_sample=3 * C))
    out += [line(k, ts[k], nb) for k, _ in loaders] + [verdict(ts, nb)]
    out.append("  not measured: tables beyond the Infinity Cache (this set is 6.6 MB of positions), the protein shape, more than one GPU")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
