"""PackedStream (fastegnn_amd/data.py) without a GPU: its orchestration driven through the torch restatement of its two device calls
(tests/packed_stream_ref.py, swapped in for ``data._COLLATE_OPS`` as tests/test_packed_cpu.py does), the order against the mirror of
the header's permutation, the state words, the argument checks of the three new entry points."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from tests.packed_graph_ref import CHUNK_EDGES, assert_graph_equals, stable_csr
from tests.packed_ref import ragged_frames
from tests.packed_stream_ref import M64, TorchStreamOps, advance_ref, check_stream_batch, ids_ref, sequence_ref, uniform_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N_FRAMES, NODES, EDGES = 11, 5, 7


@pytest.fixture(scope="module")
def packed():
    return D.PackedDataset(uniform_frames(N_FRAMES, NODES, EDGES, seed=3))


@pytest.fixture
def torch_ops(monkeypatch):
    monkeypatch.setattr(D, "_COLLATE_OPS", TorchStreamOps)


def test_frame_shape(packed):
    assert packed.frame_shape == (NODES, EDGES)
    assert D.PackedDataset(ragged_frames()).frame_shape is None
    assert D.PackedDataset(uniform_frames(3, 7, 0)).frame_shape == (7, 0)
    same_nodes = uniform_frames(2, 4, 6) + uniform_frames(1, 4, 5)      # the edge counts alone differ
    assert D.PackedDataset(same_nodes).frame_shape is None
    assert D.PackedDataset(uniform_frames(1, 2, 2)).frame_shape == (2, 2)


def test_ragged_frames_and_oversized_batches_raise_naming_the_alternative(packed):
    with pytest.raises(ValueError, match="PackedLoader"):
        D.PackedStream(D.PackedDataset(ragged_frames()), 4)
    with pytest.raises(ValueError, match="PackedLoader"):
        D.PackedStream(packed, N_FRAMES + 1)
    with pytest.raises(ValueError, match="PackedLoader"):
        D.PackedStream(packed, 0)
    with pytest.raises(ValueError, match="graphs"):
        D.PackedStream(packed, 4, graphs="coo")


@pytest.mark.parametrize("graphs", [None, "csr", "csr+csc"])
def test_three_epochs_equal_collate_of_the_mirrored_ids(packed, torch_ops, graphs):
    B = 4
    assert K.lib().fastegnn_chunk_edges() == CHUNK_EDGES       # the chunk size the mirror assumes
    stream = D.PackedStream(packed, B, shuffle=True, seed=17, graphs=graphs)
    assert len(stream) == N_FRAMES // B == 2
    want_ids = sequence_ref(17, B, N_FRAMES, 3 * len(stream))
    ptrs = {k: v.data_ptr() for k, v in stream._batch._t.items() if isinstance(v, torch.Tensor)}
    seen = []
    for epoch in range(3):
        for i, batch in enumerate(stream):
            ids = want_ids[epoch * len(stream) + i]
            want = check_stream_batch(stream, batch, packed, ids)
            seen.append(ids)
            if graphs is None:
                assert "graph" not in batch.keys()
                continue
            csc = graphs == "csr+csc"
            g = batch["graph"]
            assert (g.n_rows, g.n_src, g.E) == (B * NODES, B * NODES, B * EDGES)
            assert_graph_equals(g, stable_csr(want["edge_index"], B * NODES, csc=csc), csc)
    assert {k: v.data_ptr() for k, v in stream._batch._t.items() if isinstance(v, torch.Tensor)} == ptrs   # the same buffers throughout
    for epoch in range(3):       # the ids of an epoch are distinct; two epochs differ
        flat = np.concatenate(seen[2 * epoch:2 * epoch + 2])
        assert len(set(flat.tolist())) == 2 * B and flat.min() >= 0 and flat.max() < N_FRAMES
    assert not np.array_equal(np.concatenate(seen[0:2]), np.concatenate(seen[2:4]))
    assert not np.array_equal(np.concatenate(seen[2:4]), np.concatenate(seen[4:6]))


def test_a_callable_graphs_is_evaluated_once_with_the_batch_edge_total(packed, torch_ops):
    calls = []

    def want_csc(n_edges):
        calls.append(n_edges)
        return True
    stream = D.PackedStream(packed, 3, graphs=want_csc)
    for _ in range(4):
        assert stream.next()["graph"].cscptr is not None
    assert calls == [3 * EDGES]


def test_without_shuffle_the_frames_come_in_order(packed, torch_ops):
    stream = D.PackedStream(packed, 3, shuffle=False)
    assert len(stream) == 3
    for epoch in range(2):
        got = [stream.ids.tolist() for _ in stream]
        assert sum(got, []) == list(range(9))     # frames 9 and 10 are left over in every epoch
    check_stream_batch(stream, stream._batch, packed, [6, 7, 8])


def test_the_cursor_wraps_and_the_epoch_increments_exactly_at_n_over_b(packed, torch_ops):
    B = 2
    stream = D.PackedStream(packed, B, seed=(1 << 64) - 3)
    nb = N_FRAMES // B
    assert len(stream) == nb == 5
    assert stream.state_dict() == {"seed": (1 << 64) - 3, "epoch": 0, "cursor": 0}
    for k in range(1, 2 * nb + 2):
        stream.next()
        assert stream.state_dict() == {"seed": (1 << 64) - 3, "epoch": k // nb, "cursor": k % nb}, k


def test_a_state_dict_round_trip_continues_the_same_sequence(packed, torch_ops):
    a = D.PackedStream(packed, 4, seed=5)
    for _ in range(3):
        a.next()
    state = a.state_dict()
    assert state == {"seed": 5, "epoch": 1, "cursor": 1}
    b = D.PackedStream(packed, 4, seed=99)
    b.load_state_dict(state)
    assert b.state_dict() == state
    for _ in range(5):
        a.next(), b.next()
        assert a.ids.tolist() == b.ids.tolist()
        assert torch.equal(a._batch["loc_0"], b._batch["loc_0"])
    assert a.state_dict() == b.state_dict() == {"seed": 5, "epoch": 4, "cursor": 0}


def test_one_frame_and_one_batch_per_epoch(torch_ops):
    one = D.PackedDataset(uniform_frames(1, 3, 4))
    s = D.PackedStream(one, 1)
    for _ in range(3):
        check_stream_batch(s, s.next(), one, [0])
    assert s.state_dict()["epoch"] == 3
    p = D.PackedDataset(uniform_frames(6, 3, 4))
    s = D.PackedStream(p, 6, seed=2)          # B = n: every epoch is one batch of all frames, in that epoch's order
    first, second = s.next()["loc_0"].clone(), s.next()["loc_0"].clone()
    assert sorted(s.ids.tolist()) == list(range(6)) and not torch.equal(first, second)


def test_ids_stay_in_range_whatever_the_state_words_hold(packed, torch_ops):
    B = 4
    stream = D.PackedStream(packed, B, seed=12345)
    for epoch, cursor in ((M64, 1 << 63), (1 << 63, M64), (0, M64 - 1)):
        state = {"seed": 12345, "epoch": epoch, "cursor": cursor}
        stream.load_state_dict(state)
        assert stream.state_dict() == state
        batch = stream.next()
        ids = stream.ids.tolist()
        assert ids == ids_ref(12345, epoch, cursor, B, N_FRAMES).tolist()
        assert min(ids) >= 0 and max(ids) < N_FRAMES and len(set(ids)) == B
        check_stream_batch(stream, batch, packed, ids)
        e2, c2 = advance_ref(epoch, cursor, B, N_FRAMES)
        assert 0 <= c2 < N_FRAMES // B and e2 in (epoch, (epoch + 1) & M64)
        assert stream.state_dict() == {"seed": 12345, "epoch": e2, "cursor": c2}


def test_a_stream_on_a_cpu_dataset_has_no_fallback(packed):
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        D.PackedStream(packed, 4).next()


def test_new_symbols_are_declared_bound_and_the_revision_stays():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    for name in ("fastegnn_collate_draw", "fastegnn_collate_gather_uniform", "fastegnn_loss_accumulate"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in K.EXPORTED
        for act in (False, True):
            for wide in (False, True):
                assert hasattr(K.lib(act=act, wide=wide), name), (name, act, wide)
    assert K.ABI_VERSION == 108 and K.lib().fastegnn_version() == 108
    import fastegnn_amd
    assert "train_epoch" in fastegnn_amd.__all__ and callable(fastegnn_amd.train_epoch)


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = K.lib()
    SOME = C.c_void_p(64)
    draw, gather, accumulate = L.fastegnn_collate_draw, L.fastegnn_collate_gather_uniform, L.fastegnn_loss_accumulate
    for args, msg in [((None, 4, 8, 1, 1, SOME, None), b"null pointer"), ((SOME, 4, 8, 1, 1, None, None), b"null pointer"),
                      ((SOME, 0, 8, 1, 1, SOME, None), b"B < 1"), ((SOME, -3, 8, 1, 1, SOME, None), b"B < 1"),
                      ((SOME, 9, 8, 1, 1, SOME, None), b"n_frames < B")]:
        assert draw(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"collate_draw" in L.fastegnn_last_error()
    for args, msg in [((None, SOME, 3, SOME, None), b"null pointer"), ((SOME, None, 3, SOME, None), b"null pointer"),
                      ((SOME, SOME, 3, None, None), b"null pointer"), ((SOME, SOME, -1, SOME, None), b"B < 0")]:
        assert accumulate(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"loss_accumulate" in L.fastegnn_last_error()
    assert accumulate(SOME, SOME, 0, SOME, None) == 0    # no graph: nothing launched
    tabs, w = (C.c_void_p * 8)(*([64] * 8)), (C.c_int32 * 7)(3, 3, 3, 2, 1, 2, 9)
    nch = C.c_int32(0)
    #     ids   B  n  nodes edges src_n src_e src   dst   w  [6 packed graph tables] [6 outputs] chunk_row n_chunks stream
    ok = [SOME, 4, 10, 5, 20, 50, 200, tabs, tabs, w] + [SOME] * 6 + [SOME] * 6 + [SOME, C.byref(nch), None]

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    wide = (C.c_int32 * 7)(3, 3, 3, 2, 1, 2, (1 << 20) + 1)
    holes = (C.c_void_p * 8)(*([64] * 7 + [None]))
    for args, msg in [(bad(a1=0), b"B < 1"), (bad(a2=0), b"no frame"), (bad(a3=-1), b"negative size"), (bad(a4=-1), b"negative size"),
                      (bad(a5=49), b"not n_frames times"), (bad(a6=201), b"not n_frames times"), (bad(a0=None), b"null pointer"),
                      (bad(a7=None), b"null pointer"), (bad(a9=None), b"null pointer"), (bad(a9=wide), b"row width out of range"),
                      (bad(a7=holes), b"null edge_index"), (bad(a22=None), b"null output"), (bad(a23=None), b"null output"),
                      (bad(a20=None), b"given or omitted together"), (bad(a21=None), b"given or omitted together"),
                      (bad(a15=None), b"hold none"), (bad(a14=None, a15=None), b"hold none"), (bad(a11=None), b"null pointer"), (bad(a17=None), b"null pointer"),
                      (bad(a1=1 << 30, a2=1 << 30, a5=5 << 30, a6=20 << 30), b"int32 sizes")]:
        assert gather(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"collate_gather_uniform" in L.fastegnn_last_error(), (msg, L.fastegnn_last_error())
