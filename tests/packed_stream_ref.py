"""Test infrastructure for the packed stream (fastegnn_amd/data.py: PackedStream): datasets of equal-sized frames, the mirror of the
stream's order -- include/fastegnn_hip.h, fastegnn_collate_draw, through tests/mmd_sampler_ref.py's ``perm_ref`` as it stands -- and
``TorchStreamOps``, tests/packed_graph_ref.py's ``TorchGraphOps`` extended by torch restatements of ``fastegnn_collate_draw`` and
``fastegnn_collate_gather_uniform`` (same argument order as ``data.HipCollateOps``), so that tests/test_packed_stream_cpu.py drives the
stream's orchestration without a GPU."""
import numpy as np
import torch

from fastegnn_amd import data as D
from tests.mmd_sampler_ref import perm_ref
from tests.packed_graph_ref import CHUNK_EDGES, TorchGraphOps, assert_graph_equals, stable_csr
from tests.packed_ref import assert_batches_equal, make_frame

STREAM_TAG = 0x5354524D   # the `b` of the keyed permutation in a stream's draw
M64 = (1 << 64) - 1


def uniform_frames(n_frames, nodes, edges, C=3, edge_width=2, seed=0, device="cpu"):
    """n_frames frames of `nodes` nodes and `edges` edges: node rows of 3 / 2 / 1 floats, edge rows of `edge_width`, loc_mean [1,3,C]"""
    gen = torch.Generator().manual_seed(seed)
    return [make_frame(nodes, edges, C, edge_width, gen).to(device) for _ in range(n_frames)]


def ids_ref(seed, epoch, cursor, B, n, shuffle=True):
    """the frame numbers a draw writes from the state words {seed, epoch, cursor} (Python ints, taken mod 2^64) -> int64 array [B]"""
    nb = n // B
    c = (int(cursor) & M64) % nb
    j = np.arange(c * B, c * B + B, dtype=np.int64)
    if not shuffle:
        return j
    return perm_ref(int(seed) & M64, int(epoch) & M64, STREAM_TAG, n, j).astype(np.int64)


def advance_ref(epoch, cursor, B, n):
    """-> (epoch, cursor) behind a draw with advance != 0"""
    nb = n // B
    c = (int(cursor) & M64) % nb
    return ((int(epoch) + 1) & M64, 0) if c + 1 >= nb else (int(epoch) & M64, c + 1)


def sequence_ref(seed, B, n, draws, shuffle=True, epoch=0, cursor=0):
    """the ids of `draws` consecutive next() calls from a state -> list of int64 arrays"""
    out = []
    for _ in range(draws):
        out.append(ids_ref(seed, epoch, cursor, B, n, shuffle))
        epoch, cursor = advance_ref(epoch, cursor, B, n)
    return out


def _u64(v):
    return int(v) & M64


def _i64(v):
    v = _u64(v)
    return v - (1 << 64) if v >= 1 << 63 else v


def check_stream_batch(stream, batch, packed, ids):
    """the stream's current batch against ``collate`` of the frames `ids`: the frame numbers, then every key in order, ``ptr`` and
    ``batch`` included, with torch.equal (``"graph"``, when the batch carries one, is the caller's to compare)"""
    assert batch is stream._batch
    assert stream.ids.tolist() == [int(i) for i in ids]
    want = D.collate([packed[int(i)] for i in ids])
    keys = [k for k in batch.keys() if k != "graph"]
    assert keys == list(want.keys()) and list(batch.keys())[len(keys):] in ([], ["graph"])
    assert_batches_equal(D.Batch(**{k: batch[k] for k in keys}), want)
    return want


class TorchStreamOps(TorchGraphOps):
    """``data.HipCollateOps.draw`` / ``.gather_uniform`` restated in torch"""

    @staticmethod
    def draw(state, batch_size, n_frames, shuffle, advance, ids_out):
        seed, epoch, cursor, _ = [_u64(v) for v in state.tolist()]
        ids_out.copy_(torch.from_numpy(ids_ref(seed, epoch, cursor, batch_size, n_frames, shuffle)))
        if advance:
            epoch, cursor = advance_ref(epoch, cursor, batch_size, n_frames)
            state[1], state[2] = _i64(epoch), _i64(cursor)

    @staticmethod
    def gather_uniform(ids, n_frames, nodes, edges, src_tables, dst_tables, src_graph=None, dst_graph=None, chunk_row=None, call=None):
        idc = ids.clamp(0, n_frames - 1).tolist()
        B = len(idc)
        for i, f in enumerate(idc):
            for t in range(5):
                dst_tables[t][i * nodes:(i + 1) * nodes] = src_tables[t][f * nodes:(f + 1) * nodes]
            dst_tables[5][i * edges:(i + 1) * edges] = src_tables[5][f * edges:(f + 1) * edges]
            dst_tables[6][i] = src_tables[6][f]
            dst_tables[7][:, i * edges:(i + 1) * edges] = src_tables[7][:, f * edges:(f + 1) * edges] + i * nodes
        if dst_graph is None:
            return 0
        g_rowptr, g_erow, g_col, g_perm, g_cscptr, g_csc_eid = src_graph
        rowptr, erow, col, perm, cscptr, csc_eid = dst_graph
        N, E = B * nodes, B * edges
        for i, j in enumerate(idc):
            no, eo, ns, es = i * nodes, i * edges, slice(j * nodes, (j + 1) * nodes), slice(j * edges, (j + 1) * edges)
            rowptr[no:no + nodes] = (g_rowptr[ns] - j * edges + eo).int()
            erow[eo:eo + edges] = g_erow[es] + no
            col[eo:eo + edges] = g_col[es] + no
            perm[eo:eo + edges] = g_perm[es] + eo
            if cscptr is not None:
                cscptr[no:no + nodes] = (g_cscptr[ns] - j * edges + eo).int()
                csc_eid[eo:eo + edges] = g_csc_eid[es] + eo
        rowptr[N] = E
        if cscptr is not None:
            cscptr[N] = E
        n_chunks = E // CHUNK_EDGES + 1
        targets = torch.arange(n_chunks) * CHUNK_EDGES
        chunk_row[:n_chunks] = torch.searchsorted(rowptr[:N].contiguous(), targets.int(), right=False).int()
        chunk_row[n_chunks] = N
        return n_chunks


__all__ = ["TorchStreamOps", "uniform_frames", "ids_ref", "advance_ref", "sequence_ref", "check_stream_batch", "assert_graph_equals",
           "stable_csr", "STREAM_TAG"]
