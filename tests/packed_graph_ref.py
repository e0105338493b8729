"""Test infrastructure for the packed loader's sorted graphs (fastegnn_amd/data.py: PackedDataset.build_graphs, graphs=...): the
ragged dataset A and the dataset B the CPU and GPU tests share, ``stable_csr`` -- what ``fastegnn_build_csr`` returns, restated with
torch's stable sort -- and ``TorchGraphOps``, tests/packed_ref.py's ``TorchCollateOps`` extended by torch restatements of the
per-slab sort and of ``fastegnn_collate_graph`` (same argument order as ``data.HipCollateOps``)."""
import torch

from fastegnn_amd import data as D
from tests.packed_ref import TorchCollateOps, make_frame

CHUNK_EDGES = 32   # fastegnn_chunk_edges() of the product build (checked by the CPU test)

# dataset A: (nodes, edges) of its nine frames.  One 2048-element tile is frame 5's edge list exactly; frame 8 spans several tiles;
# frames 0..4 share one; 64 and 2048 are multiples of CHUNK_EDGES, 33 and 5000 are not (33 is one past a multiple)
A_SHAPES = [(1, 0), (2, 2), (5, 20), (17, 0), (64, 64), (300, 2048), (1, 0), (33, 33), (700, 5000)]
A_FLAT_TAIL = (5, 8)   # frames whose highest-numbered node has no edge: the tail of the frame's rowptr range is flat
A_BATCHES = [list(range(9)), list(range(8, -1, -1)), [3, 3, 3], [4], [5], [0, 3, 6], [2, 0, 8, 6, 5]]
A_BATCH_NAMES = ["in order", "reversed", "one edgeless frame thrice", "B=1 (64 edges)", "B=1 (one tile)", "no edges at all", "mixed"]


def frames_a(C=3, seed=0, device="cpu"):
    """random endpoints: self loops, repeated edges and isolated nodes occur"""
    gen = torch.Generator().manual_seed(seed)
    frames = []
    for i, (n, e) in enumerate(A_SHAPES):
        f = make_frame(n, e, C, 1, gen)
        if i in A_FLAT_TAIL:
            f.edge_index = torch.randint(0, n - 1, (2, e), generator=gen, dtype=torch.int64)
        frames.append(f.to(device))
    return frames


def frames_b(n_frames=1100, C=3, seed=1, device="cpu"):
    """frames of 5 nodes and 20 edges: 1 100 of them are more than one 1024-frame round of the plan kernel, a hundred per tile"""
    gen = torch.Generator().manual_seed(seed)
    return [make_frame(5, 20, C, 1, gen).to(device) for _ in range(n_frames)]


def stable_csr(edge_index, n_nodes, csc=True):
    """the arrays of ``SortedGraph(edge_index, n_nodes, csc=csc)`` (include/fastegnn_hip.h, fastegnn_build_csr) as a dict of int32
    tensors + n_chunks: stable sort by row; the col-keyed index is the stable sort of the row-sorted columns; chunk k starts at the
    first row whose first edge position is >= k * CHUNK_EDGES; chunk_row[n_chunks] = n_nodes"""
    E = edge_index.size(1)
    i32 = lambda t: t.to(torch.int32)  # noqa: E731
    perm = torch.sort(edge_index[0], stable=True).indices
    erow, col = edge_index[0][perm], edge_index[1][perm]
    ids = torch.arange(n_nodes + 1, device=edge_index.device)
    rowptr = torch.searchsorted(erow.contiguous(), ids, right=False)
    out = dict(rowptr=i32(rowptr), erow=i32(erow), col=i32(col), perm=i32(perm), cscptr=None, csc_eid=None)
    if csc:
        csc_eid = torch.sort(col, stable=True).indices
        out["cscptr"] = i32(torch.searchsorted(col[csc_eid].contiguous(), ids, right=False))
        out["csc_eid"] = i32(csc_eid)
    n_chunks = E // CHUNK_EDGES + 1
    targets = torch.arange(n_chunks, device=edge_index.device) * CHUNK_EDGES
    chunk_row = torch.searchsorted(rowptr[:n_nodes].contiguous(), targets, right=False)
    out["chunk_row"] = i32(torch.cat([chunk_row, torch.tensor([n_nodes], device=edge_index.device)]))
    out["n_chunks"] = n_chunks
    return out


GRAPH_ARRAYS = ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid", "chunk_row")


def assert_graph_equals(graph, want, csc):
    """``graph``: a SortedGraph; ``want``: a SortedGraph or ``stable_csr``'s dict.  ``==`` on every element: the edge arrays over
    [:E] (both sides allocate max(E, 1), the one element of an edgeless graph is never written), chunk_row over [:n_chunks + 1]"""
    get = (lambda k: want[k]) if isinstance(want, dict) else (lambda k: getattr(want, k))  # noqa: E731
    E, nch = graph.E, graph.n_chunks
    assert nch == get("n_chunks") and nch == E // CHUNK_EDGES + 1
    assert (graph.cscptr is not None) == (graph.csc_eid is not None) == csc
    for k in GRAPH_ARRAYS:
        a, b = getattr(graph, k), get(k)
        if a is None:
            continue
        assert a.dtype == torch.int32 and b is not None, k
        n = {"rowptr": graph.n_rows + 1, "cscptr": graph.n_src + 1, "chunk_row": nch + 1}.get(k, E)
        assert a.numel() >= n and b.numel() >= n, (k, a.numel(), b.numel(), n)
        assert torch.equal(a[:n], b[:n]), k


class TorchGraphOps(TorchCollateOps):
    """``data.HipCollateOps.sort`` / ``.graph`` restated in torch"""

    @staticmethod
    def sort(edge_index, n_nodes):
        g = stable_csr(edge_index, n_nodes, csc=True)
        return g["rowptr"], g["erow"], g["col"], g["perm"], g["cscptr"], g["csc_eid"]

    @staticmethod
    def graph(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out, n_nodes_out, n_edges_out, src_graph, dst_graph, chunk_row):
        g_rowptr, g_erow, g_col, g_perm, g_cscptr, g_csc_eid = src_graph
        rowptr, erow, col, perm, cscptr, csc_eid = dst_graph
        idc = ids.clamp(0, src_node_ptr.numel() - 2).tolist()
        npo, epo, snp, sep = node_ptr_out.tolist(), edge_ptr_out.tolist(), src_node_ptr.tolist(), src_edge_ptr.tolist()
        for i, j in enumerate(idc):
            no, eo, nodes, edges = npo[i], epo[i], slice(snp[j], snp[j + 1]), slice(sep[j], sep[j + 1])
            rowptr[no:npo[i + 1]] = (g_rowptr[nodes] - sep[j] + eo).int()
            erow[eo:epo[i + 1]] = g_erow[edges] + no
            col[eo:epo[i + 1]] = g_col[edges] + no
            perm[eo:epo[i + 1]] = g_perm[edges] + eo
            if cscptr is not None:
                cscptr[no:npo[i + 1]] = (g_cscptr[nodes] - sep[j] + eo).int()
                csc_eid[eo:epo[i + 1]] = g_csc_eid[edges] + eo
        rowptr[n_nodes_out] = n_edges_out
        if cscptr is not None:
            cscptr[n_nodes_out] = n_edges_out
        n_chunks = n_edges_out // CHUNK_EDGES + 1
        targets = torch.arange(n_chunks) * CHUNK_EDGES
        chunk_row[:n_chunks] = torch.searchsorted(rowptr[:n_nodes_out].contiguous(), targets.int(), right=False).int()
        chunk_row[n_chunks] = n_nodes_out
        return n_chunks
