"""Test infrastructure for rollouts (fastegnn_amd/rollout.py): ``TorchRolloutOps``, a torch restatement of the three device calls of
csrc/rollout.hip with their rounding rules, their clamps and their skips (same argument order as ``rollout.HipRolloutOps``), so that
tests/test_rollout_cpu.py drives the orchestration without a GPU and tests/test_gpu_rollout.py has something to compare the kernels
with -- what ``TorchTrajOps`` of tests/trajectory_ref.py is to the trajectory loader."""
import numpy as np
import torch

from oracle import graphs_ref
from tests.trajectory_ref import TorchTrajOps


def speed(v: torch.Tensor) -> torch.Tensor:
    """sqrt((vx*vx + vy*vy) + vz*vz), every operation rounded to fp32 by itself (numpy's square root: torch's vectorised one on the
    CPU is not correctly rounded at every input) -- ``TorchTrajOps.gather``'s expression"""
    v = v.cpu()
    return torch.from_numpy(np.sqrt(((v[:, 0] * v[:, 0] + v[:, 1] * v[:, 1]) + v[:, 2] * v[:, 2]).numpy()))


class TorchRolloutOps:
    """include/fastegnn_hip.h "rollouts": fastegnn_rollout_plan / _advance / _graph restated in torch (host tensors)."""

    @staticmethod
    def plan(ids, samples, traj_row0, traj_n, traj_T, delta_t, truth_rows):
        sid = ids.clamp(0, samples.size(0) - 1)
        tr = samples[sid, 0].clamp(0, traj_n.numel() - 1)
        n, T = traj_n[tr].clamp(min=0), traj_T[tr]
        f = torch.minimum(samples[sid, 1].clamp(min=0), (T - 1).clamp(min=0))
        for k in range(truth_rows.size(0)):
            frame = f + (k + 1) * int(delta_t)
            truth_rows[k] = torch.where(frame < T, traj_row0[tr] + frame * n, torch.full_like(frame, -1))

    @staticmethod
    def advance(x_new, delta_t, loc, vel, node_feat, record, flag):
        inv = torch.tensor(1.0, dtype=torch.float32) / torch.tensor(float(int(delta_t)), dtype=torch.float32)   # the fp32 value 1.0f / dt
        ok = torch.isfinite(x_new)
        d = x_new - loc                      # one fp32 subtraction,
        v = d * inv                          # then one fp32 multiplication: torch fuses nothing here
        v = torch.where(ok, v, torch.zeros_like(v))
        if record is not None:
            record.copy_(x_new)
        loc.copy_(torch.where(ok, x_new, loc))
        vel.copy_(v)
        node_feat[:, 0] = speed(v)
        if not bool(ok.all()):
            flag.set(1)

    @staticmethod
    def graph(ptr, loc, x_new, pos, truth_rows, loc_mean, sse):
        p, N = ptr.tolist(), loc.size(0)
        for b in range(len(p) - 1):
            at, n = p[b], p[b + 1] - p[b]
            if n < 0 or at < 0 or at + n > N:
                n = 0
            # (tests/trajectory_ref.py's mean: the fp64 sum rounded once; its order is the kernel's to within fp64 rounding)
            loc_mean[b] = (loc[at:at + n].double().sum(0) / n).float().unsqueeze(-1) if n > 0 else 0.0
            if sse is None:
                continue
            r = int(truth_rows[b])
            if r < 0 or r + n > pos.size(0) or n == 0:
                sse[b] = float("nan")
                continue
            d = x_new[at:at + n].double() - pos[r:r + n].double()
            sse[b] = ((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2]).sum()

    @staticmethod
    def augment(edge_attr, loc_0, edge_index):
        """``cat([edge_attr, ||loc_0[row] - loc_0[col]||], 1)`` (train.augment_edge_attr)"""
        row, col = edge_index
        length = (loc_0[row] - loc_0[col]).pow(2).sum(-1, keepdim=True).sqrt()
        return length if edge_attr is None else torch.cat([edge_attr.float(), length], 1)


class MirrorTrajOps(TorchTrajOps):
    """the trajectory loader's mirror plus the edges the product path gets from the batched graph calls: per cloud the float32 brute
    force and the cutoff of oracle/graphs_ref.py, ids shifted by the cloud's first node.  ``seen`` keeps every ``loc_0`` the graph build
    was handed."""
    seen = []

    @staticmethod
    def edges(loc_0, ptr, ptr_host, radius, cutoff_rate):
        assert ptr.tolist() == list(ptr_host)
        MirrorTrajOps.seen.append(loc_0.clone())
        ei, dist = [], []
        for a, b in zip(ptr_host, ptr_host[1:]):
            e, d = graphs_ref.cutoff_edges(*graphs_ref.radius_graph_bruteforce(loc_0[a:b].numpy(), radius), cutoff_rate)
            ei.append(torch.from_numpy(e) + a)
            dist.append(torch.from_numpy(d))
        return torch.cat(ei, 1), torch.cat(dist, 0)


class StandIn(torch.nn.Module):
    """a small torch model with FastEGNN's call signature whose prediction depends on ``edge_index`` / ``edge_attr`` (a sum over each
    node's neighbours), ``vel_0``, ``node_feat`` and ``loc_mean``; ``nan_at``: the call (counted from 0) that returns a NaN and an Inf"""

    def __init__(self, nan_at=None):
        super().__init__()
        self.calls, self.nan_at = 0, nan_at

    def forward(self, node_loc, node_vel, node_attr, node_feat, edge_index, loc_mean, data_batch, edge_attr):
        row, col = edge_index
        pull = torch.zeros_like(node_loc).index_add_(0, row, (node_loc[col] - node_loc[row]) * edge_attr[:, -1:])
        centre = loc_mean[data_batch, :, 0]
        out = node_loc + 0.5 * node_vel + 0.01 * pull + 0.125 * node_feat[:, :1] * (centre - node_loc) + 0.001 * node_feat[:, 1:]
        if self.calls == self.nan_at:
            out = out.clone()
            out[0, 1], out[-1, 2] = float("nan"), float("inf")
        self.calls += 1
        return out, loc_mean


def equal_with_nan(a: torch.Tensor, b: torch.Tensor) -> bool:
    """bit-for-bit where finite, NaN exactly where the other is NaN"""
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(a.nan_to_num(nan=0.0), b.nan_to_num(nan=0.0))
