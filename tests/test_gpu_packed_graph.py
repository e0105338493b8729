"""The packed loader's sorted graphs on the device (csrc/collate.hip: fastegnn_collate_graph; data.PackedDataset.build_graphs,
batch(graphs=...), PackedLoader(graphs=...)).  The reference is the function the assembled graph replaces: ``SortedGraph(batch
["edge_index"], N, csc=...)``, i.e. ``fastegnn_build_csr`` on the collated batch.  Integers: every comparison of the index is
``torch.equal`` (the edge arrays over [:E], both sides allocate max(E, 1); chunk_row over [:n_chunks + 1]).  The model comparisons run
one input twice through one set of weights -- once sorting ``edge_index``, once on the assembled graph of identical arrays -- so what
is left is the run-to-run band of the float atomics: the limits are tests/stress_runner.py's, taken from there."""
import ctypes as C

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from fastegnn_amd import egnn as egnn_module
from fastegnn_amd.model import SortedGraph
from fastegnn_amd.train import FusedAdam, MMDSampler, augment_edge_attr, evaluate, train_step
from tests.packed_graph_ref import A_BATCH_NAMES, A_BATCHES, assert_graph_equals, frames_a, frames_b
from tests.packed_ref import assert_batches_equal
from tests.stress_runner import OUT_LIMIT, _limit, _rel

pytestmark = pytest.mark.gpu

SENT, PAD = -77, 67   # guard bands: sentinel value, elements on either side of every output (odd: the outputs start unaligned)


@pytest.fixture(scope="module")
def packed_a():
    return D.PackedDataset(frames_a(device="cuda"))


@pytest.fixture(scope="module")
def packed_b():
    return D.PackedDataset(frames_b(device="cuda"))


def _parity(packed, ids, csc):
    want = D.collate([packed[int(i)] for i in ids])
    got = packed.batch(ids, graphs="csr+csc" if csc else "csr")
    assert list(got.keys()) == list(want.keys()) + ["graph"]
    for k in want.keys():
        assert got[k].dtype == want[k].dtype and torch.equal(got[k], want[k]), k
    g, N = got["graph"], want.num_nodes
    assert (g.n_rows, g.n_src, g.E) == (N, N, want["edge_index"].size(1))
    assert_graph_equals(g, SortedGraph(got["edge_index"], N, csc=csc), csc)
    return got


@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csr+csc"])
@pytest.mark.parametrize("ids", A_BATCHES, ids=A_BATCH_NAMES)
def test_ragged_batches_carry_the_graph_build_csr_would_sort(packed_a, ids, csc):
    got = _parity(packed_a, ids, csc)
    if ids == [0, 3, 6]:   # no edge at all: zero offsets and the one chunk, as build_csr writes them
        g = got["graph"]
        assert g.E == 0 and g.n_chunks == 1 and g.chunk_row[:2].tolist() == [0, 19] and not g.rowptr.any()
        assert not csc or not g.cscptr.any()


@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csr+csc"])
def test_more_frames_than_one_scan_round(packed_b, csc):
    got = _parity(packed_b, list(range(1100)), csc)
    assert got.num_graphs == 1100 and got["graph"].E == 22000


def test_packed_tables_are_built_once_and_cost_what_the_docs_say(packed_a):
    G = packed_a.build_graphs().graph_tables
    assert packed_a.build_graphs().graph_tables is G
    nodes, edges = int(packed_a.node_ptr_host[-1]), int(packed_a.edge_ptr_host[-1])
    assert sum(t.numel() * t.element_size() for t in G.values()) == 16 * edges + 16 * (nodes + 1)
    assert all(t.device == packed_a.device for t in G.values())


def _direct(packed, ids_dev, n_nodes, n_edges, node_ptr_out, edge_ptr_out, csc):
    """fastegnn_collate_graph itself with every output carved from a larger sentinel-filled buffer -> (return code, {name: (buffer,
    element count)}, n_chunks)"""
    G = packed.graph_tables
    sizes = dict(rowptr=n_nodes + 1, erow=n_edges, col=n_edges, perm=n_edges, cscptr=n_nodes + 1, csc_eid=n_edges,
                 chunk_row=n_edges // K.lib().fastegnn_chunk_edges() + 2)
    if not csc:
        del sizes["cscptr"], sizes["csc_eid"]
    bufs = {k: (torch.full((n + 2 * PAD,), SENT, dtype=torch.int32, device="cuda"), n) for k, n in sizes.items()}
    # (the address itself: the data_ptr() of an empty view -- an edge array of a batch without edges -- is null)
    out = {k: C.c_void_p(b.data_ptr() + 4 * PAD) for k, (b, n) in bufs.items()}
    nch = C.c_int32(-1)
    st = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    rc = K.lib().fastegnn_collate_graph(
        K.ptr(ids_dev), ids_dev.numel(), K.ptr(packed.node_ptr), K.ptr(packed.edge_ptr), len(packed), G["g_rowptr"].numel() - 1,
        G["g_erow"].numel(), K.ptr(node_ptr_out), K.ptr(edge_ptr_out), n_nodes, n_edges,
        *[K.ptr(G[k]) for k in D._GRAPH_KEYS], *[out.get(k) for k in ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid")],
        out["chunk_row"], C.byref(nch), st)
    torch.cuda.synchronize()
    return rc, bufs, nch.value


def _bands_intact(bufs):
    for k, (b, n) in bufs.items():
        assert bool((b[:PAD] == SENT).all()) and bool((b[PAD + n:] == SENT).all()), k


def _plan(packed, ids):
    ids_dev = torch.tensor(ids, dtype=torch.int64, device="cuda")
    node_ptr_out, edge_ptr_out = (torch.empty(len(ids) + 1, dtype=torch.int64, device="cuda") for _ in range(2))
    D.HipCollateOps.plan(ids_dev, packed.node_ptr, packed.edge_ptr, node_ptr_out, edge_ptr_out)
    return ids_dev, node_ptr_out, edge_ptr_out, int(packed._node_cnt[ids].sum()), int(packed._edge_cnt[ids].sum())


@pytest.mark.parametrize("csc", [False, True], ids=["csr", "csr+csc"])
@pytest.mark.parametrize("ids", [list(range(9)), [2, 0, 8, 6, 5], [0, 3, 6]], ids=["in order", "mixed", "no edges at all"])
def test_nothing_is_written_outside_the_outputs(packed_a, ids, csc):
    packed_a.build_graphs()
    ids_dev, npo, epo, n_nodes, n_edges = _plan(packed_a, ids)
    rc, bufs, nch = _direct(packed_a, ids_dev, n_nodes, n_edges, npo, epo, csc)
    assert rc == 0, K.lib().fastegnn_last_error()
    _bands_intact(bufs)
    want = SortedGraph(packed_a.batch(ids)["edge_index"], n_nodes, csc=csc)
    assert nch == want.n_chunks
    for k, (b, n) in bufs.items():
        assert not bool((b[PAD:PAD + n] == SENT).any()), k                      # every element of every output is written
        m = nch + 1 if k == "chunk_row" else n
        assert torch.equal(b[PAD:PAD + m], getattr(want, k)[:m]), k


@pytest.mark.parametrize("replan", [False, True], ids=["ids corrupted behind the plan", "the plan sees the corrupted ids too"])
def test_corrupted_ids_are_clamped(packed_a, replan):
    """the device id array overwritten after the upload with -7 and n_frames + 3: the kernels clamp every id to [0, n_frames) and
    skip what does not fall inside its frame's segment, so the call returns, reads nothing outside the packed tables (by reading
    csrc/collate.hip: every index is a clamped id, an offset below B, or checked against the table's rows) and writes nothing
    outside the outputs.  With the plan rerun on the corrupted ids the offsets no longer add up to the host's totals either."""
    packed_a.build_graphs()
    ids = [2, 0, 8, 6, 5]
    ids_dev, npo, epo, n_nodes, n_edges = _plan(packed_a, ids)
    ids_dev[1], ids_dev[3] = -7, len(packed_a) + 3
    if replan:
        D.HipCollateOps.plan(ids_dev, packed_a.node_ptr, packed_a.edge_ptr, npo, epo)
    rc, bufs, nch = _direct(packed_a, ids_dev, n_nodes, n_edges, npo, epo, True)
    assert rc == 0 and nch == n_edges // K.lib().fastegnn_chunk_edges() + 1
    _bands_intact(bufs)
    if not replan:   # the frames whose ids are intact are assembled as before
        want = SortedGraph(packed_a.batch(ids)["edge_index"], n_nodes, csc=True)
        a, b = int(packed_a._edge_cnt[[2, 0]].sum()), int(packed_a._edge_cnt[[2, 0, 8]].sum())
        for k in ("erow", "col", "perm"):
            assert torch.equal(bufs[k][0][PAD + a:PAD + b], getattr(want, k)[a:b]), k


def _no_sort(*a, **k):
    raise AssertionError("a batch that carries its graph reached fastegnn_build_csr")


def _compare(name, got, want):
    assert set(got) == set(want)
    for k in want:
        assert bool(torch.isfinite(got[k]).all()) and bool(torch.isfinite(want[k]).all()), (name, k)
        e = _rel(got[k], want[k])
        print(f"{name}: {k}: {e:.3g} (limit {_limit(k):.0e})")
        assert e <= _limit(k), (name, k, e)


@pytest.mark.parametrize("ids", [[2, 0, 8, 6, 5], [1, 2, 4]], ids=["7 068 edges (atomic scatter)", "86 edges (col-keyed sum)"])
@pytest.mark.parametrize("kind", ["FastEGNN", "FastRF", "EGNN"])
def test_models_take_the_assembled_graph(packed_a, monkeypatch, kind, ids):
    torch.manual_seed(0)
    if kind == "EGNN":
        m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
        graphs = "csr+csc" if m.deterministic else "csr"
    else:
        m = getattr(fastegnn_amd, kind)(2, 0, 2, 64, 3, device="cuda", n_layers=2)
        graphs = m.deterministic_for
    batch = packed_a.batch(ids, graphs=graphs)
    assert isinstance(batch["graph"], SortedGraph)
    if kind != "EGNN":
        assert (batch["graph"].cscptr is not None) == m.deterministic_for(batch["edge_index"].size(1))
    target = batch["loc_t"]

    def run(edge_index):
        for p in m.parameters():
            p.grad = None
        leaf = {k: batch[k].clone().requires_grad_(True) for k in ("loc_0", "vel_0", "node_feat", "loc_mean")}
        ea = augment_edge_attr(batch["edge_attr"], batch["loc_0"], batch["edge_index"]).requires_grad_(kind == "EGNN")
        if kind == "EGNN":
            x, v, h = m(x=leaf["loc_0"], h=leaf["node_feat"], edge_index=edge_index, edge_fea=ea, v=leaf["vel_0"])
            (torch.nn.functional.mse_loss(x, target) + 0.1 * h.square().mean()).backward()
            res = {"loc": x.detach(), "vloc": h.detach(), "grad:edge_fea": ea.grad}
            del leaf["loc_mean"]
        else:
            loc, vloc = m(node_feat=leaf["node_feat"], node_loc=leaf["loc_0"], node_vel=leaf["vel_0"], edge_index=edge_index,
                          data_batch=batch["batch"], loc_mean=leaf["loc_mean"], edge_attr=ea)
            (torch.nn.functional.mse_loss(loc, target) + 0.1 * vloc.square().mean()).backward()
            res = {"loc": loc.detach(), "vloc": vloc.detach()}
        res.update({"grad:" + k: v.grad for k, v in leaf.items()})
        res.update({k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None})
        return res
    want = run(batch["edge_index"])
    # from here on nothing may sort: SortedGraph(...) -- the one caller of fastegnn_build_csr, EGNN's included -- raises
    assert egnn_module.SortedGraph is SortedGraph
    monkeypatch.setattr(SortedGraph, "__init__", _no_sort)
    if kind != "EGNN":
        monkeypatch.setattr(m, "sorted_graph", _no_sort)
    got = run(batch["graph"])
    assert len(m._graph_cache) == 1 and not hasattr(batch["graph"], "_keepalive")   # the assembled graph is never cached
    _compare(kind, got, want)


def test_train_step_and_evaluate_on_a_loader_with_graphs():
    """200 frames of 5 nodes and 20 edges, batch size 50.  Two models from one seed, one fed by PackedLoader(graphs=None), one by
    PackedLoader(graphs=model.deterministic_for) and barred from sorting.  After every step the second model's weights are set to the
    first's, so that each pair of losses comes from ONE set of weights and one input: the repeated-pass limit of
    tests/stress_runner.py (OUT_LIMIT, relative) then applies to every step, not only to the first."""
    packed = D.PackedDataset(frames_b(200, device="cuda"))
    models, opts = [], []
    for _ in range(2):
        torch.manual_seed(0)
        models.append(fastegnn_amd.FastEGNN(2, 0, 2, 64, 3, device="cuda", n_layers=2))
        opts.append(FusedAdam(models[-1].parameters(), lr=5e-4, weight_decay=1e-12))
    plain, graphed = models
    graphed.sorted_graph = _no_sort
    loaders = [D.PackedLoader(packed, batch_size=50, shuffle=True, generator=torch.Generator().manual_seed(4), graphs=g)
               for g in (None, graphed.deterministic_for)]
    samplers = [MMDSampler(0), MMDSampler(0)]
    n = 0
    for a, b in zip(*loaders):
        assert "graph" not in a.keys() and isinstance(b["graph"], SortedGraph) and b["graph"].cscptr is None   # 1 000 edges: atomics
        assert_batches_equal(D.Batch(**{k: b[k] for k in a.keys()}), a)
        la, lb = (train_step(m, o, d, None, sigma=1.0, weight=0.01, sampler=s, num_sample=3)
                  for m, o, d, s in zip(models, opts, (a, b), samplers))
        for (la_k, lb_k), what in zip(zip(la, lb), ("loss", "mse")):
            la_k, lb_k = float(la_k), float(lb_k)
            print(f"train_step batch {n}: {what} {la_k:.8g} vs {lb_k:.8g}")
            assert la_k == la_k and abs(la_k - lb_k) <= OUT_LIMIT * abs(la_k), (n, what, la_k, lb_k)
        with torch.no_grad():
            for pa, pb in zip(plain.parameters(), graphed.parameters()):
                pb.copy_(pa)
        n += 1
    assert n == 4
    ea, eb = (evaluate(m, ld, sigma=1.0, weight=0.01, sampler=MMDSampler(1), num_sample=3) for m, ld in zip(models, loaders))
    print(f"evaluate: {ea} vs {eb}")
    assert ea["graphs"] == eb["graphs"] == 200
    for k in ("mse", "loss"):
        assert ea[k] == ea[k] and abs(ea[k] - eb[k]) <= OUT_LIMIT * abs(ea[k]), (k, ea, eb)


def test_an_epoch_with_graphs_does_not_synchronise(packed_a):
    small = lambda n_edges: n_edges <= 512  # noqa: E731
    loader = D.PackedLoader(packed_a, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(2), graphs=small)
    first = list(loader)   # warm-up epoch (the frames are sorted here if no test before did it)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        second = list(loader)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert len(first) == len(second) == 3
    for b in second:
        csc = b["edge_index"].size(1) <= 512
        assert_graph_equals(b["graph"], SortedGraph(b["edge_index"], b.num_nodes, csc=csc), csc)
