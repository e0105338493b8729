"""Test infrastructure for the trajectory loader (fastegnn_amd/data.py: TrajectoryDataset / TrajectoryLoader): the synthetic set of
four trajectories the CPU and the GPU tests share, and ``TorchTrajOps``, a torch restatement of the three device calls of
csrc/traj.hip (same argument order as ``data.HipTrajOps``), so that tests/test_trajectory_cpu.py drives the orchestration without a
GPU -- what ``TorchCollateOps`` of tests/packed_ref.py is to the packed loader."""
import numpy as np
import torch

# (key, frames T, particles n): not a multiple of 16 or 64 | a one-point cloud (no edges, the mean is the point) | more than two waves,
# across a 128-lane boundary | across the gather's tile (1 024 nodes) and across 2 048
SHAPES = (("A", 6, 37), ("B", 4, 1), ("C", 9, 130), ("D", 3, 2049))
DELTA_T = 2
RADIUS = 0.3          # A, C and D have edges at this radius in the unit cube, B (one point) has none
KINDS = (1.0, 3.0, 5.0)
# samples="all" at DELTA_T: start frames 0 .. T - 3 of every trajectory, trajectory by trajectory
FIRST = {"A": 0, "B": 4, "C": 6, "D": 13}
N_SAMPLES = 14


def make_trajectories(seed=0):
    """[(key, position float32 [T,n,3] in the unit cube, kind float32 [n] from KINDS)] from one seeded generator"""
    rng = np.random.default_rng(seed)
    out = []
    for key, T, n in SHAPES:
        out.append((key, rng.random((T, n, 3), dtype=np.float32), rng.choice(np.asarray(KINDS, dtype=np.float32), size=n)))
    return out


def write_npz(path, trajectories):
    """the ``<partition>.npz`` container ``read_trajectories`` reads: ``<key>/position``, ``<key>/particle_type``"""
    arrays = {}
    for key, position, kind in trajectories:
        arrays[f"{key}/position"] = position
        arrays[f"{key}/particle_type"] = kind
    np.savez(path, **arrays)


def sliced(trajectories, samples, ids, delta_t, device="cpu"):
    """(loc_0, vel_0, loc_t, kind [N,1], ptr list) of the samples ``ids``, sliced from the raw arrays by torch: the inputs of the
    yardstick ``water3d_batch``"""
    loc_0, vel_0, loc_t, kind, ptr = [], [], [], [], [0]
    for i in ids:
        t, f = (int(v) for v in samples[int(i)])
        pos = torch.from_numpy(trajectories[t][1]).float().to(device)
        loc_0.append(pos[f])
        vel_0.append(pos[f + 1] - pos[f])
        loc_t.append(pos[f + delta_t])
        kind.append(torch.from_numpy(np.asarray(trajectories[t][2])).float().reshape(-1, 1).to(device))
        ptr.append(ptr[-1] + pos.size(1))
    return torch.cat(loc_0, 0), torch.cat(vel_0, 0), torch.cat(loc_t, 0), torch.cat(kind, 0), ptr


class TorchTrajOps:
    """include/fastegnn_hip.h "mini-batch assembly from device-resident trajectories": fastegnn_traj_plan / _gather / _mean, restated
    in torch with their clamps and their skips.  ``edges`` is left to the test that uses the mirror (the batched radius graph has no CPU
    form)."""

    @staticmethod
    def plan(ids, samples, traj_row0, traj_n, traj_T, traj_kind0, delta_t, ptr_out, slots_out):
        sid = ids.clamp(0, samples.size(0) - 1)
        tr = samples[sid, 0].clamp(0, traj_n.numel() - 1)
        n, last = traj_n[tr].clamp(min=0), (traj_T[tr] - 1).clamp(min=0)
        f = torch.minimum(samples[sid, 1].clamp(min=0), last)
        for w, frame in enumerate((f, torch.minimum(f + 1, last), torch.minimum(f + delta_t, last))):
            slots_out[:, w] = traj_row0[tr] + frame * n
        slots_out[:, 3] = traj_kind0[tr]
        ptr_out[0] = 0
        ptr_out[1:] = torch.cumsum(n, 0)

    @staticmethod
    def _spans(ptr, slots, pos_rows, kind_rows=None):
        """(slot, first output node, node count, slot words) of every slot whose source rows lie inside the tables"""
        p, s = ptr.tolist(), slots.tolist()
        for b in range(len(p) - 1):
            n, (r0, r1, rt, k0) = p[b + 1] - p[b], s[b]
            ok = n > 0 and min(r0, r1, rt, k0) >= 0 and max(r0, r1, rt) + n <= pos_rows and (kind_rows is None or k0 + n <= kind_rows)
            if ok:
                yield b, p[b], n, (r0, r1, rt, k0)

    @staticmethod
    def gather(ptr, slots, n_nodes, pos, kind, kind_scaled, loc_0, loc_t, vel_0, node_feat, node_attr, batch_out):
        for b, at, n, (r0, r1, rt, k0) in TorchTrajOps._spans(ptr, slots, pos.size(0), kind.size(0)):
            n = min(n, n_nodes - at)   # nothing is written at or beyond n_nodes
            if n <= 0:
                continue
            v = pos[r1:r1 + n] - pos[r0:r0 + n]
            loc_0[at:at + n], loc_t[at:at + n], vel_0[at:at + n] = pos[r0:r0 + n], pos[rt:rt + n], v
            # (numpy's square root: torch's vectorised one on the CPU is not correctly rounded at every input)
            node_feat[at:at + n, 0] = torch.from_numpy(np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).numpy()))
            node_feat[at:at + n, 1] = kind_scaled[k0:k0 + n, 0]
            node_attr[at:at + n] = kind[k0:k0 + n]
            batch_out[at:at + n] = b

    @staticmethod
    def mean(ptr, slots, pos, loc_mean):
        loc_mean.zero_()
        for b, _, n, (r0, _, _, _) in TorchTrajOps._spans(ptr, slots, pos.size(0)):
            loc_mean[b] = (pos[r0:r0 + n].double().sum(0) / n).float().unsqueeze(-1)
