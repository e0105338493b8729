"""The packed loader's sorted graphs without a GPU (fastegnn_amd/data.py: PackedDataset.build_graphs, batch(graphs=...),
PackedLoader(graphs=...); model.SortedGraph.from_arrays): the packing-time tables, the orchestration and the argument checks, driven
through the torch restatements of tests/packed_graph_ref.py.  Integers only: every comparison is ``==`` on every element."""
import ctypes as C
import os
import re

import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from fastegnn_amd.model import SortedGraph
from tests.packed_graph_ref import (A_BATCH_NAMES, A_BATCHES, A_FLAT_TAIL, A_SHAPES, CHUNK_EDGES, TorchGraphOps, assert_graph_equals,
                                    frames_a, stable_csr)
from tests.packed_ref import assert_batches_equal

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def frames():
    return frames_a()


@pytest.fixture
def torch_ops(monkeypatch):
    monkeypatch.setattr(D, "_COLLATE_OPS", TorchGraphOps)


@pytest.fixture
def packed(frames, torch_ops):
    return D.PackedDataset(frames)


def test_dataset_a_is_what_the_tests_say(frames):
    assert [(f.num_nodes, f.edge_index.size(1)) for f in frames] == A_SHAPES and len(A_SHAPES) == 9
    assert K.lib().fastegnn_chunk_edges() == CHUNK_EDGES
    for i in A_FLAT_TAIL:
        assert int(frames[i].edge_index.max()) < frames[i].num_nodes - 1
    ei = frames[8].edge_index
    assert bool((ei[0] == ei[1]).any()) and torch.unique(ei, dim=1).size(1) < ei.size(1)   # self loops, repeated edges
    assert torch.unique(frames[4].edge_index).numel() < 64                                    # isolated nodes


def test_default_allocates_no_graph_tables(frames, torch_ops):
    p = D.PackedDataset(frames)
    assert p.graph_tables is None
    p.batch([0, 1, 2])
    list(D.PackedLoader(p, batch_size=4))
    assert p.graph_tables is None


def test_packed_tables_hold_each_frames_own_sort(frames, packed):
    assert packed.build_graphs() is packed
    G, nodes, edges = packed.graph_tables, sum(n for n, _ in A_SHAPES), sum(e for _, e in A_SHAPES)
    for k in ("g_rowptr", "g_cscptr"):
        assert G[k].dtype == torch.int64 and G[k].shape == (nodes + 1,) and int(G[k][nodes]) == edges
        assert torch.equal(G[k][packed.node_ptr[:-1]], packed.edge_ptr[:-1])   # frames are contiguous
    for k in ("g_erow", "g_col", "g_perm", "g_csc_eid"):
        assert G[k].dtype == torch.int32 and G[k].shape == (edges,)
    for i, f in enumerate(frames):
        a, b = int(packed.node_ptr_host[i]), int(packed.node_ptr_host[i + 1])
        ea, eb = int(packed.edge_ptr_host[i]), int(packed.edge_ptr_host[i + 1])
        want = stable_csr(f.edge_index, f.num_nodes)
        assert torch.equal(G["g_rowptr"][a:b] - ea, want["rowptr"][:-1].long()) and torch.equal(G["g_cscptr"][a:b] - ea, want["cscptr"][:-1].long())
        for k in ("erow", "col", "perm", "csc_eid"):
            assert torch.equal(G["g_" + k][ea:eb], want[k]), (i, k)
    tabs = packed.graph_tables
    assert packed.build_graphs().graph_tables is tabs   # idempotent


@pytest.mark.parametrize("limit", ["frames", "nodes", "edges"])
def test_the_slab_seam_leaves_the_tables_unchanged(frames, torch_ops, monkeypatch, limit):
    one = D.PackedDataset(frames).build_graphs().graph_tables
    calls = []

    class Counting(TorchGraphOps):
        @staticmethod
        def sort(edge_index, n_nodes):
            calls.append((n_nodes, edge_index.size(1)))
            return TorchGraphOps.sort(edge_index, n_nodes)
    monkeypatch.setattr(D, "_COLLATE_OPS", Counting)
    if limit == "frames":
        monkeypatch.setattr(D, "GRAPH_SLAB_FRAMES", 2)
    elif limit == "nodes":
        monkeypatch.setattr(D, "GRAPH_SLAB_NODES", 80)     # frame 5 (300 nodes) and frame 8 (700) are slabs of their own
    else:
        monkeypatch.setattr(D, "GRAPH_SLAB_EDGES", 100)
    many = D.PackedDataset(frames).build_graphs().graph_tables
    if limit == "frames":
        assert calls == [(3, 2), (22, 20), (364, 2112), (34, 33), (700, 5000)]   # two frames per slab
    else:
        assert len(calls) > 2 and (300, 2048) in calls and (700, 5000) in calls
    assert sum(n for n, _ in calls) == sum(n for n, _ in A_SHAPES) and sum(e for _, e in calls) == sum(e for _, e in A_SHAPES)
    for k in one:
        assert torch.equal(one[k], many[k]), k


def test_a_frame_beyond_the_sorted_graphs_limits_raises(frames, torch_ops, monkeypatch):
    monkeypatch.setattr(D, "_GRAPH_MAX_EDGES", 4999)
    with pytest.raises(ValueError, match="frame 8"):
        D.PackedDataset(frames).build_graphs()
    assert D.GRAPH_SLAB_NODES * 8 <= (1 << 30) // 68 and D.GRAPH_SLAB_EDGES * 8 <= (1 << 30) // 8   # far inside the ABI's limits


@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csr+csc"])
@pytest.mark.parametrize("ids", A_BATCHES, ids=A_BATCH_NAMES)
def test_assembled_graph_is_the_stable_sort_of_the_batch(frames, packed, ids, csc):
    want_batch = D.collate([frames[i] for i in ids])
    got = packed.batch(ids, graphs="csr+csc" if csc else "csr")
    assert list(got.keys()) == list(want_batch.keys()) + ["graph"]
    for k in want_batch.keys():
        assert torch.equal(got[k], want_batch[k]), k
    g, N = got["graph"], want_batch.num_nodes
    assert isinstance(g, SortedGraph) and (g.n_rows, g.n_src, g.E) == (N, N, want_batch["edge_index"].size(1)) and g._key is None
    assert_graph_equals(g, stable_csr(want_batch["edge_index"], N, csc=csc), csc)


def test_graphs_none_is_the_loader_as_it_was(frames, packed):
    for ids in A_BATCHES:
        assert_batches_equal(packed.batch(ids), D.collate([frames[i] for i in ids]))
        assert_batches_equal(packed.batch(ids, graphs=None), D.collate([frames[i] for i in ids]))
    old = D.DataLoader(frames, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(3))
    new = D.PackedLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(3), graphs=None)
    for a, b in zip(new, old):
        assert_batches_equal(a, b)
    assert packed.graph_tables is None


def test_a_callable_decides_the_col_keyed_index_per_batch(frames, packed):
    seen = []

    def small(n_edges):
        seen.append(n_edges)
        return n_edges <= 512
    loader = D.PackedLoader(packed, batch_size=4, graphs=small)
    assert packed.graph_tables is None          # sorted when the first batch is drawn, not before
    batches = list(loader)
    edges = [b["edge_index"].size(1) for b in batches]
    assert seen == edges == [22, 2145, 5000]
    assert [b["graph"].cscptr is not None for b in batches] == [True, False, False]
    assert [b["graph"].csc_eid is not None for b in batches] == [True, False, False]
    for b in batches:
        csc = b["graph"].cscptr is not None
        assert_graph_equals(b["graph"], stable_csr(b["edge_index"], b.num_nodes, csc=csc), csc)
        assert b.detach()["graph"] is b["graph"] and b.to("cpu")["graph"] is b["graph"] and "SortedGraph" in repr(b)


def test_graphs_argument_is_checked(packed):
    for bad in ("csc", 1, "CSR"):
        with pytest.raises(ValueError, match="graphs"):
            packed.batch([0], graphs=bad)
        with pytest.raises(ValueError, match="graphs"):
            D.PackedLoader(packed, graphs=bad)


def test_graphs_on_a_cpu_dataset_have_no_fallback(frames):
    p = D.PackedDataset(frames)
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.build_graphs()
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        p.batch([0, 1], graphs="csr")


def _arrays(n=4, E=6, csc=True):
    z = lambda k: torch.zeros(k, dtype=torch.int32)  # noqa: E731
    return dict(rowptr=z(n + 1), erow=z(E), col=z(E), perm=z(E), cscptr=z(n + 1) if csc else None, csc_eid=z(E) if csc else None,
                chunk_row=z(2), n_chunks=1, n_rows=n, n_src=n, E=E)


def test_from_arrays_takes_the_arrays_as_they_are():
    a = _arrays()
    g = SortedGraph.from_arrays(**a)
    assert all(getattr(g, k) is a[k] for k in ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid", "chunk_row"))
    assert (g.n_rows, g.n_src, g.E, g.n_chunks, g._key) == (4, 4, 6, 1, None) and not hasattr(g, "_keepalive")
    s = g.struct()
    assert (s.n_rows, s.n_src, s.n_edges, s.n_chunks) == (4, 4, 6, 1) and s.rowptr == a["rowptr"].data_ptr() and s.cscptr == a["cscptr"].data_ptr()
    g = SortedGraph.from_arrays(**_arrays(csc=False))
    assert g.cscptr is None and g.csc_eid is None and g.struct().cscptr is None
    SortedGraph.from_arrays(**{**_arrays(E=0), "erow": torch.zeros(1, dtype=torch.int32)})   # longer than E: as __init__ allocates


def test_from_arrays_rejects_what_does_not_fit():
    for k in ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid", "chunk_row"):
        with pytest.raises(TypeError, match=k):
            SortedGraph.from_arrays(**{**_arrays(), k: _arrays()[k].long()})
        with pytest.raises(ValueError, match=k):
            SortedGraph.from_arrays(**{**_arrays(), k: _arrays()[k][:1]})            # too short
        if k != "rowptr":
            with pytest.raises(ValueError, match=k + " lives on"):
                SortedGraph.from_arrays(**{**_arrays(), k: _arrays()[k].to("meta")})   # another device than rowptr's
    with pytest.raises(ValueError, match="rowptr"):
        SortedGraph.from_arrays(**{**_arrays(), "rowptr": torch.zeros(6, dtype=torch.int32)})   # rowptr is [n_rows + 1] exactly
    with pytest.raises(ValueError, match="col"):
        SortedGraph.from_arrays(**{**_arrays(), "col": torch.zeros(12, dtype=torch.int32)[::2]})   # not contiguous
    with pytest.raises(TypeError, match="perm"):
        SortedGraph.from_arrays(**{**_arrays(), "perm": None})
    for k in ("cscptr", "csc_eid"):
        with pytest.raises(ValueError, match="together"):
            SortedGraph.from_arrays(**{**_arrays(), k: None})
    for k, v in (("n_rows", -1), ("E", -1), ("n_chunks", 0)):
        with pytest.raises(ValueError):
            SortedGraph.from_arrays(**{**_arrays(), k: v})


def test_the_symbol_is_in_all_four_libraries_and_the_revision_stays():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    assert re.search(r"\bint fastegnn_collate_graph\(", src) and "fastegnn_collate_graph" in K.EXPORTED
    assert K.ABI_VERSION == 108 and "#define FASTEGNN_ABI_VERSION 108" in re.sub(r"[ \t]+", " ", src)
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            assert hasattr(L, "fastegnn_collate_graph"), (act, wide)
            assert L.fastegnn_version() == 108


def test_entry_point_rejects_bad_arguments_before_any_launch():
    L = K.lib()
    S, nch = C.c_void_p(64), C.c_int32(0)
    #      0  1  2  3  4  5    6    7  8  9   10  11..16 packed tables  17..22 outputs      23 24              25
    ok = [S, 4, S, S, 5, 100, 200, S, S, 40, 80, S, S, S, S, S, S, S, S, S, S, S, S, S, C.byref(nch), None]

    assert len(ok) == 26

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    for args, msg in [(bad(a1=-1), b"B < 0"), (bad(a4=0), b"no frame"), (bad(a5=-1), b"negative size"), (bad(a9=-1), b"negative size"),
                      (bad(a10=-1), b"negative size"), (bad(a9=(1 << 31) - 1), b"int32"), (bad(a10=1 << 31), b"int32"),
                      (bad(a1=0), b"batch of no frames"), (bad(a17=None), b"null output"), (bad(a23=None), b"null output"),
                      (bad(a24=None), b"null output"), (bad(a21=None), b"given or omitted together"),
                      (bad(a22=None), b"given or omitted together"), (bad(a15=None), b"given or omitted together"),
                      (bad(a0=None), b"null pointer"), (bad(a7=None), b"null pointer"), (bad(a8=None), b"null pointer"),
                      (bad(a11=None), b"null pointer"), (bad(a13=None), b"null pointer"), (bad(a19=None), b"null pointer"),
                      (bad(a15=None, a16=None), b"the packed tables hold none")]:
        assert L.fastegnn_collate_graph(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"collate_graph" in L.fastegnn_last_error(), (msg, L.fastegnn_last_error())
