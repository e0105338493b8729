"""PackedStream on the device (csrc/collate.hip: collate_draw_kernel, collate_gather_uniform_kernel) against ``data.collate`` of the
frames the mirrored order names, and against ``SortedGraph`` of the batch's own edge list.  Copies and integer additions are exact:
every comparison is ``torch.equal``; no tolerance anywhere.  Then the two entry points by themselves between guard bands, the claim
that ``next()`` does no host work, a captured ``next()`` (alone: no model code inside a capture), and fastegnn_loss_accumulate."""
import numpy as np
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from fastegnn_amd.model import SortedGraph, _stream
from tests.packed_graph_ref import assert_graph_equals
from tests.packed_stream_ref import M64, advance_ref, check_stream_batch, ids_ref, sequence_ref, uniform_frames

pytestmark = pytest.mark.gpu

# (nodes, edges, frames, B): node rows are 3 / 3 / 3 / 2 / 1 floats wide, edge rows 2, loc_mean 9
SHAPES = {
    "every float segment a multiple of 16 bytes": (4, 6, 10, 3),
    "odd segments, odd edge total: row 1 of edge_index 8-byte aligned": (5, 7, 37, 5),
    "segments 2 mod 4": (6, 10, 9, 4),
    "no edges": (7, 0, 6, 4),
    "jobs longer than one tile, frames straddling tiles": (100, 300, 20, 8),
    "B = 1": (4, 6, 5, 1),
    "B = n": (5, 7, 6, 6),
    "one frame": (6, 10, 1, 1),
}


def _i64(v):
    v = int(v) & M64
    return v - (1 << 64) if v >= 1 << 63 else v


def _check_graph(batch, csc=True):
    n = batch["batch"].numel()
    assert_graph_equals(batch["graph"], SortedGraph(batch["edge_index"], n, csc=csc), csc)


@pytest.mark.parametrize("name", list(SHAPES))
def test_three_epochs_equal_collate_and_the_sorted_graph(name):
    nodes, edges, n, B = SHAPES[name]
    packed = D.PackedDataset(uniform_frames(n, nodes, edges, seed=n + B), device="cuda")
    assert packed.frame_shape == (nodes, edges) and (packed.tables["edge_index"].size(1) % 2 == 1) == (name.startswith("odd"))
    plain = D.PackedStream(packed, B, seed=41)
    graph = D.PackedStream(packed, B, seed=41, graphs="csr+csc")
    assert len(plain) == len(graph) == n // B
    want_ids = sequence_ref(41, B, n, 3 * len(plain))
    for epoch in range(3):
        for i, (bp, bg) in enumerate(zip(plain, graph)):
            ids = want_ids[epoch * len(plain) + i]
            check_stream_batch(plain, bp, packed, ids)
            check_stream_batch(graph, bg, packed, ids)
            assert "graph" not in bp.keys()
            _check_graph(bg)
    assert plain.state_dict() == graph.state_dict() == {"seed": 41, "epoch": 3, "cursor": 0}


def test_without_shuffle_and_with_the_row_keyed_graph_alone():
    packed = D.PackedDataset(uniform_frames(7, 5, 7, seed=2), device="cuda")
    stream = D.PackedStream(packed, 3, shuffle=False, graphs="csr")
    for epoch in range(2):
        for i, b in enumerate(stream):
            check_stream_batch(stream, b, packed, range(3 * i, 3 * i + 3))
            assert b["graph"].cscptr is None and b["graph"].csc_eid is None
            _check_graph(b, csc=False)


def test_more_tiles_than_the_block_cap():
    """two frames of 300 001 nodes and 100 001 edges in one batch: some 3 800 tiles of 2 048 elements for a launch of at most 2 048
    workgroups, so the grid-stride loop runs twice; odd segments, one element per lane"""
    packed = D.PackedDataset(uniform_frames(2, 300001, 100001, C=1, edge_width=1, seed=8), device="cuda")
    stream = D.PackedStream(packed, 2, seed=3)
    out_elems = sum(v.numel() for k, v in stream._batch._t.items() if k not in ("ptr", "batch"))
    assert out_elems // 2048 > 2048        # CL_TILE elements per tile, CL_MAX_BLOCKS workgroups (csrc/collate.hip)
    for ids in sequence_ref(3, 2, 2, 2):
        check_stream_batch(stream, stream.next(), packed, ids)


# ---- the two entry points called directly, every output carved out of a poisoned buffer ----
POISON_F, POISON_I = -7777.0, -0x0123456789ABCDE


def _carve(shape, dtype, guard):
    """a contiguous tensor of `shape` inside a poisoned buffer, `guard` elements in front and behind -> (view, buffer)"""
    n = int(np.prod(shape))
    poison = POISON_F if dtype == torch.float32 else (POISON_I if dtype == torch.int64 else -123456789)
    buf = torch.full((n + 2 * guard,), poison, dtype=dtype, device="cuda")
    return buf[guard:guard + n].view(*shape), buf


def _guards_intact(carved, guard):
    for name, (view, buf) in carved.items():
        n = view.numel()
        poison = buf[0].item()
        assert (buf[:guard] == poison).all() and (buf[guard + n:] == poison).all(), name


@pytest.mark.parametrize("guard", [1, 2, 4], ids=["outputs 4-byte aligned", "outputs 8-byte aligned", "outputs 16-byte aligned"])
@pytest.mark.parametrize("state", [(M64, 1 << 63), (5, 2)], ids=["cursor 2^63, epoch 2^64 - 1", "epoch 5, cursor 2"])
def test_the_entry_points_between_guard_bands(state, guard):
    """(4, 6) frames: every segment allows 16-byte accesses, so the access width is decided by where the guard puts the outputs"""
    nodes, edges, n, B, seed = 4, 6, 11, 3, 77
    packed = D.PackedDataset(uniform_frames(n, nodes, edges, seed=1), device="cuda").build_graphs()
    epoch, cursor = state
    ops, T, G = D.HipCollateOps, packed.tables, packed.graph_tables
    carved = {"ids": _carve((B,), torch.int64, guard), "state": _carve((4,), torch.int64, guard)}
    st = carved["state"][0]
    st.copy_(torch.tensor([seed, _i64(epoch), _i64(cursor), 0x1234], dtype=torch.int64))
    ids = carved["ids"][0]
    ops.draw(st, B, n, True, True, ids)
    want_ids = ids_ref(seed, epoch, cursor, B, n)
    assert 0 <= ids.min().item() and ids.max().item() < n and ids.tolist() == want_ids.tolist()
    e2, c2 = advance_ref(epoch, cursor, B, n)
    assert st.tolist() == [seed, _i64(e2), _i64(c2), 0x1234]
    ops.draw(st, B, n, True, False, ids)           # advance == 0 leaves the state
    assert st.tolist() == [seed, _i64(e2), _i64(c2), 0x1234] and ids.tolist() == ids_ref(seed, e2, c2, B, n).tolist()
    for k in D._PACK_KEYS:
        rows = B * (nodes if k in D._NODE_KEYS else edges if k == "edge_attr" else 1)
        shape = (2, B * edges) if k == "edge_index" else (rows,) + T[k].shape[1:]
        carved[k] = _carve(shape, T[k].dtype, guard)
    N, E = B * nodes, B * edges
    for k, cnt in (("rowptr", N + 1), ("erow", E), ("col", E), ("perm", E), ("cscptr", N + 1), ("csc_eid", E),
                   ("chunk_row", E // K.lib().fastegnn_chunk_edges() + 2)):
        carved[k] = _carve((cnt,), torch.int32, guard)
    dst_graph = [carved[k][0] for k in ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid")]
    for given in (ids, torch.tensor([-5, 10 ** 12, 4], device="cuda")):   # then ids far outside: clamped to [0, n)
        n_chunks = ops.gather_uniform(given, n, nodes, edges, [T[k] for k in D._PACK_KEYS], [carved[k][0] for k in D._PACK_KEYS],
                                      [G[k] for k in D._GRAPH_KEYS], dst_graph, carved["chunk_row"][0])
        chosen = given.clamp(0, n - 1).tolist()
        want = D.collate([packed[i] for i in chosen])
        for k in D._PACK_KEYS:
            assert torch.equal(carved[k][0], want[k]), k
        g = SortedGraph.from_arrays(*dst_graph, carved["chunk_row"][0], n_chunks, N, N, E)
        assert_graph_equals(g, SortedGraph(want["edge_index"], N, csc=True), True)
        _guards_intact(carved, guard)


# ---- no host work ----
@pytest.mark.parametrize("graphs", [None, "csr+csc"])
def test_next_allocates_nothing_synchronises_nothing_and_is_two_or_three_launches(graphs):
    nodes, edges, n, B = 5, 20, 40, 8
    packed = D.PackedDataset(uniform_frames(n, nodes, edges, edge_width=1, seed=6), device="cuda")
    stream = D.PackedStream(packed, B, seed=9, graphs=graphs)
    for _ in range(2):
        stream.next()
    torch.cuda.synchronize()
    tensors = dict(stream._batch._t, ids=stream.ids)
    if graphs:
        g = tensors.pop("graph")
        tensors.update({k: getattr(g, k) for k in ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid", "chunk_row")})
    ptrs = {k: v.data_ptr() for k, v in tensors.items()}
    before = torch.cuda.memory_allocated()
    torch.cuda.set_sync_debug_mode("error")
    try:
        batches = [stream.next() for _ in range(10)]
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert torch.cuda.memory_allocated() == before
    assert all(b is batches[0] for b in batches)
    assert {k: v.data_ptr() for k, v in tensors.items()} == ptrs
    check_stream_batch(stream, batches[-1], packed, sequence_ref(9, B, n, 12)[-1])
    L = K.lib()
    L.fastegnn_profile_enable(1)
    K.profile_collect()
    try:
        for _ in range(4):
            stream.next()
    finally:
        L.fastegnn_profile_enable(0)
        prof = K.profile_collect()
    per_next = 3 if graphs else 2
    assert set(prof) == {"misc"} and 4 <= prof["misc"][1] <= 4 * per_next, prof
    check_stream_batch(stream, stream._batch, packed, sequence_ref(9, B, n, 16)[-1])


# ---- capture of next() alone ----
@pytest.mark.parametrize("graphs", [None, "csr+csc"])
def test_a_captured_next_walks_through_the_epochs(graphs):
    nodes, edges, n, B, seed = 5, 7, 13, 4, 23
    packed = D.PackedDataset(uniform_frames(n, nodes, edges, seed=4), device="cuda")
    captured, eager = D.PackedStream(packed, B, seed=seed, graphs=graphs), D.PackedStream(packed, B, seed=seed, graphs=graphs)
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):                  # loads the kernels outside the capture
        captured.next()
    torch.cuda.current_stream().wait_stream(side)
    eager.next()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=side):
        batch = captured.next()
    assert captured.state_dict() == {"seed": seed, "epoch": 0, "cursor": 1}      # capturing ran nothing
    replays = 2 * len(captured) + 1
    want_ids = sequence_ref(seed, B, n, replays + 1)
    for r in range(replays):
        graph.replay()
        other = eager.next()
        torch.cuda.synchronize()
        check_stream_batch(captured, batch, packed, want_ids[r + 1])
        assert captured.ids.tolist() == eager.ids.tolist()
        for k in batch.keys():
            if k != "graph":
                assert torch.equal(batch[k], other[k]), (r, k)
        if graphs:
            assert_graph_equals(batch["graph"], other["graph"], True)
            _check_graph(batch)
    draws = replays + 1
    assert captured.state_dict() == eager.state_dict() == {"seed": seed, "epoch": draws // len(captured), "cursor": draws % len(captured)}


# ---- fastegnn_loss_accumulate ----
def test_loss_accumulate_is_exact_in_fp64():
    vals = np.array([[0.1, 0.7], [1e-8, 3.0], [123456.7, 1e-3], [2.5, 2.5], [1e10, 1e-10], [0.333333, 0.666666], [7.0, 9.0]],
                    dtype=np.float32)               # (loss, mse) of seven steps
    Bs = [1, 3, 100, 100, 3, 1, 100]
    dev = torch.from_numpy(vals).cuda()
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    L = K.lib()
    want = [0.0, 0.0, 0.0]
    for (loss, mse), B, row in zip(vals, Bs, dev):
        K.check(L.fastegnn_loss_accumulate(K.ptr(row[0:1]), K.ptr(row[1:2]), B, K.ptr(acc), _stream(acc.device)),
                "fastegnn_loss_accumulate")
        want[0] += float(B) * float(mse)            # B * an fp32 value is exact in fp64: one rounding per addition on both sides
        want[1] += float(B) * float(loss)
        want[2] += float(B)
    K.check(L.fastegnn_loss_accumulate(K.ptr(dev[0, 0:1]), K.ptr(dev[0, 1:2]), 0, K.ptr(acc), _stream(acc.device)),
            "fastegnn_loss_accumulate")            # B == 0: nothing moves
    assert acc.tolist() == want and want[2] == 308.0
