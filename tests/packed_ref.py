"""Test infrastructure for the packed loader (fastegnn_amd/data.py: PackedDataset / PackedLoader): the ragged dataset the CPU and
the GPU tests share, and ``TorchCollateOps``, a torch restatement of the two device calls of csrc/collate.hip (same argument
order as ``data.HipCollateOps``), so that tests/test_packed_cpu.py drives the loader's orchestration without a GPU -- what
``TorchOps`` of tests/test_wide_cpu.py is to the wide path."""
import torch

from fastegnn_amd import data as D

# 23 frames: the sizes that matter (one node, two, a repeated size, more than one wave), two frames without edges, then random
RAGGED_NODES = [1, 2, 5, 5, 17, 64, 3, 3]
ZERO_EDGE_FRAMES = (6, 7)
N_RAGGED = 23


def make_frame(n, e, C=3, edge_width=1, gen=None, device="cpu") -> D.Frame:
    """a frame of n nodes and e edges (random local ids, self loops allowed: collate only shifts them) with random fields"""
    r = lambda *shape: torch.rand(*shape, generator=gen)  # noqa: E731
    ei = torch.randint(0, n, (2, e), generator=gen, dtype=torch.int64)
    return D.Frame(ei, r(e, edge_width), r(n, 3), r(n, 3), r(n, 3), r(n, 2), r(n, 1), r(1, 3, C)).to(device)


def ragged_frames(C=3, seed=0, device="cpu"):
    gen = torch.Generator().manual_seed(seed)
    nodes = RAGGED_NODES + torch.randint(3, 41, (N_RAGGED - len(RAGGED_NODES),), generator=gen).tolist()
    frames = []
    for i, n in enumerate(nodes):
        e = 0 if i in ZERO_EDGE_FRAMES else int(torch.randint(1, 3 * n + 1, (1,), generator=gen))
        frames.append(make_frame(n, e, C, 1, gen, device))
    return frames


def assert_batches_equal(got: D.Batch, want: D.Batch):
    assert list(got.keys()) == list(want.keys())
    for k in want.keys():
        assert got[k].dtype == want[k].dtype and got[k].shape == want[k].shape, (k, got[k].shape, want[k].shape)
        assert got[k].is_contiguous(), k
        assert torch.equal(got[k], want[k]), k


class TorchCollateOps:
    """include/fastegnn_hip.h "mini-batch assembly from a packed dataset": fastegnn_collate_plan / _gather, restated in torch"""

    @staticmethod
    def plan(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out):
        idc = ids.clamp(0, src_node_ptr.numel() - 2)
        for src, out in ((src_node_ptr, node_ptr_out), (src_edge_ptr, edge_ptr_out)):
            out[0] = 0
            out[1:] = torch.cumsum(src[idc + 1] - src[idc], 0)

    @staticmethod
    def gather(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out, src_tables, dst_tables, batch_out):
        idc = ids.clamp(0, src_node_ptr.numel() - 2).tolist()
        npo, epo, snp, sep = node_ptr_out.tolist(), edge_ptr_out.tolist(), src_node_ptr.tolist(), src_edge_ptr.tolist()
        for i, f in enumerate(idc):
            for t in range(5):
                dst_tables[t][npo[i]:npo[i + 1]] = src_tables[t][snp[f]:snp[f + 1]]
            dst_tables[5][epo[i]:epo[i + 1]] = src_tables[5][sep[f]:sep[f + 1]]
            dst_tables[6][i] = src_tables[6][f]
            dst_tables[7][:, epo[i]:epo[i + 1]] = src_tables[7][:, sep[f]:sep[f + 1]] + npo[i]
            batch_out[npo[i]:npo[i + 1]] = i
