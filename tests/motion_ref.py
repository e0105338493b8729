"""Test infrastructure for rigid motions on the trajectory path (include/fastegnn_hip.h "rigid motions"; fastegnn_amd/data.py:
``TrajectoryDataset(rotation=, translation=)``, ``apply_motion``; fastegnn_amd/rollout.py): torch restatements of the new device calls
(same argument order as ``data.HipTrajOps`` / ``rollout.HipRolloutOps``), built on ``TorchTrajOps`` (tests/trajectory_ref.py) and
``TorchRolloutOps`` (tests/rollout_ref.py) with ``apply_motion`` for the rule, and the lattice fixture of the end-to-end tests."""
import numpy as np
import torch

from fastegnn_amd.data import apply_motion
from oracle import graphs_ref
from tests.rollout_ref import TorchRolloutOps, speed
from tests.trajectory_ref import TorchTrajOps


def rule_numpy(x: np.ndarray, R: np.ndarray, t=None) -> np.ndarray:
    """the rule once more, in numpy float32 scalars column by column: ((x0*R0j + x1*R1j) + x2*R2j) (+ tj), every operation rounded"""
    x, R = x.astype(np.float32), R.astype(np.float32)
    q = np.stack([(x[:, 0] * R[0, j] + x[:, 1] * R[1, j]) + x[:, 2] * R[2, j] for j in range(3)], 1)
    return q if t is None else q + np.asarray(t, dtype=np.float32)[None, :]


def split(motion_row: torch.Tensor, has_t):
    """(R [3,3], t [3] or None) of one row of a motion table"""
    return motion_row[:9].view(3, 3), (motion_row[9:] if has_t else None)


class MovedTrajOps(TorchTrajOps):
    """``TorchTrajOps`` plus fastegnn_traj_gather_moved and the mean over a [N,3] tensor, restated in torch with the gather's clamps and
    skips, plus brute-force edges (per cloud the float32 brute force and the cutoff of oracle/graphs_ref.py).  ``calls`` lists the ops
    in the order they ran."""
    calls = []

    @staticmethod
    def plan(*args):
        MovedTrajOps.calls.append("plan")
        TorchTrajOps.plan(*args)

    @staticmethod
    def gather(*args):
        MovedTrajOps.calls.append("gather")
        TorchTrajOps.gather(*args)

    @staticmethod
    def mean(*args):
        MovedTrajOps.calls.append("mean")
        TorchTrajOps.mean(*args)

    @staticmethod
    def gather_moved(ptr, slots, n_nodes, pos, kind, kind_scaled, loc_0, loc_t, vel_0, node_feat, node_attr, batch_out, motion, has_t):
        MovedTrajOps.calls.append("gather_moved")
        assert motion.shape == (ptr.numel() - 1, 12) and motion.dtype == torch.float32
        for b, at, n, (r0, r1, rt, k0) in TorchTrajOps._spans(ptr, slots, pos.size(0), kind.size(0)):
            n = min(n, n_nodes - at)   # nothing is written at or beyond n_nodes
            if n <= 0:
                continue
            R, t = split(motion[b], has_t)
            v = apply_motion(pos[r1:r1 + n] - pos[r0:r0 + n], R)   # the difference first, then its rotation, no translation
            loc_0[at:at + n], loc_t[at:at + n], vel_0[at:at + n] = apply_motion(pos[r0:r0 + n], R, t), apply_motion(pos[rt:rt + n], R, t), v
            node_feat[at:at + n, 0] = speed(v)   # (numpy's square root, tests/trajectory_ref.py)
            node_feat[at:at + n, 1] = kind_scaled[k0:k0 + n, 0]
            node_attr[at:at + n] = kind[k0:k0 + n]
            batch_out[at:at + n] = b

    @staticmethod
    def mean_of(ptr, loc, loc_mean):
        MovedTrajOps.calls.append("mean_of")
        TorchRolloutOps.graph(ptr, loc, None, None, None, loc_mean, None)

    @staticmethod
    def edges(loc_0, ptr, ptr_host, radius, cutoff_rate):
        assert ptr.tolist() == list(ptr_host)
        ei, dist = [], []
        for a, b in zip(ptr_host, ptr_host[1:]):
            e, d = graphs_ref.cutoff_edges(*graphs_ref.radius_graph_bruteforce(loc_0[a:b].numpy(), radius), cutoff_rate)
            ei.append(torch.from_numpy(e) + a)
            dist.append(torch.from_numpy(d))
        return torch.cat(ei, 1), torch.cat(dist, 0)


class MovedRolloutOps(TorchRolloutOps):
    """``TorchRolloutOps`` plus fastegnn_rollout_graph_moved: the truth rows moved in fp32 by the rule before the fp64 difference"""
    calls = []

    @staticmethod
    def graph(*args):
        MovedRolloutOps.calls.append("graph")
        TorchRolloutOps.graph(*args)

    @staticmethod
    def graph_moved(ptr, loc, x_new, pos, truth_rows, loc_mean, sse, motion, has_t):
        MovedRolloutOps.calls.append("graph_moved")
        TorchRolloutOps.graph(ptr, loc, None, None, None, loc_mean, None)
        if sse is None:
            return
        p, N = ptr.tolist(), loc.size(0)
        for b in range(len(p) - 1):
            at, n, r = p[b], p[b + 1] - p[b], int(truth_rows[b])
            if n <= 0 or at < 0 or at + n > N or r < 0 or r + n > pos.size(0):
                sse[b] = float("nan")
                continue
            d = x_new[at:at + n].double() - apply_motion(pos[r:r + n], *split(motion[b], has_t)).double()
            sse[b] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum()


# ---- the lattice fixture ----
LATTICE_SHAPES = ((5, 5, 5), (4, 4, 3), (11, 11, 9), (1, 1, 1))   # 125, 48, 1 089 (beyond the gather's 1 024-node tile) and 1 points
LATTICE_SPACING, LATTICE_JITTER, LATTICE_RADIUS = 0.1, 0.002, 0.1865
LATTICE_T, LATTICE_DT = 4, 1
LATTICE_FLOOR = 0.01   # every pair distance is at least this fraction of the radius away from the radius


def lattice_trajectories():
    """[(key, position float32 [T,n,3], kind)]: per cloud a cubic lattice of spacing 0.1 whose every frame carries its own jitter,
    uniform in +-0.002 per coordinate, all from ``default_rng(0)``.  The lattice's pair distances are 0.1, 0.1414, 0.1732, 0.2, ..; the
    radius 0.1865 lies between the third and the fourth, and a jitter moves a distance by at most 2 * sqrt(3) * 0.002 = 0.0070, so the
    nearest a distance can come to the radius is 0.1865 - 0.1802 = 0.0063 = 3.4 % of it from below and 0.1931 - 0.1865 = 0.0066 from
    above.  Asserted here in fp64, with a floor of 1 % = 1.9e-3, for every frame, before anything uses the clouds.  A rigid motion in
    fp32 displaces a point by a few units in the last place of its largest coordinate -- for coordinates below 32 (asserted by the
    tests that draw translations) under 4 * 2^-19 = 7.6e-6 -- so no pair can cross the radius under the motion."""
    rng = np.random.default_rng(0)
    out = []
    for i, shape in enumerate(LATTICE_SHAPES):
        grid = np.stack(np.meshgrid(*[np.arange(s) for s in shape], indexing="ij"), -1).reshape(-1, 3) * LATTICE_SPACING
        frames = grid[None] + rng.uniform(-LATTICE_JITTER, LATTICE_JITTER, size=(LATTICE_T,) + grid.shape)
        frames = frames.astype(np.float32)
        for f in frames.astype(np.float64):
            d = np.sqrt(((f[:, None, :] - f[None, :, :]) ** 2).sum(-1))
            gap = np.abs(d - LATTICE_RADIUS)[~np.eye(len(f), dtype=bool)]
            assert gap.size == 0 or gap.min() >= LATTICE_FLOOR * LATTICE_RADIUS, (shape, gap.min() / LATTICE_RADIUS)
        out.append((f"L{i}", frames, rng.choice(np.asarray([1.0, 3.0], dtype=np.float32), size=len(grid))))
    return out


LATTICE_SAMPLES = np.asarray([[t, 0] for t in range(len(LATTICE_SHAPES))], dtype=np.int64)


def sorted_edges(edge_index: torch.Tensor, edge_attr: torch.Tensor, n_nodes: int):
    """(pair keys ascending, the attribute in that order): the edge SET of a batch, whatever order the cutoff left it in"""
    key = edge_index[0].cpu() * n_nodes + edge_index[1].cpu()
    order = torch.argsort(key)
    return key[order], edge_attr.cpu()[order]
