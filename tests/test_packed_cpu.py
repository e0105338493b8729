"""PackedDataset / PackedLoader (fastegnn_amd/data.py) without a GPU: the packing, the argument checks, and the loader's
orchestration driven through the torch restatement of its two device calls (tests/packed_ref.py)."""
import ctypes as C
import os
import re
from dataclasses import fields, replace

import numpy as np
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd import data as D
from tests.packed_ref import N_RAGGED, RAGGED_NODES, ZERO_EDGE_FRAMES, TorchCollateOps, assert_batches_equal, make_frame, ragged_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def frames():
    return ragged_frames(C=3, seed=0)


@pytest.fixture(scope="module")
def packed(frames):
    return D.PackedDataset(frames)


@pytest.fixture
def torch_ops(monkeypatch):
    monkeypatch.setattr(D, "_COLLATE_OPS", TorchCollateOps)


def test_the_ragged_dataset_is_what_the_tests_say(frames):
    nodes = [f.num_nodes for f in frames]
    assert len(frames) == N_RAGGED == 23 and nodes[:8] == RAGGED_NODES == [1, 2, 5, 5, 17, 64, 3, 3]
    assert all(3 <= n <= 40 for n in nodes[8:])
    assert [i for i, f in enumerate(frames) if f.edge_index.size(1) == 0] == list(ZERO_EDGE_FRAMES)


def test_offsets_are_the_cumulative_counts(frames, packed):
    assert len(packed) == len(frames)
    nodes = np.cumsum([0] + [f.num_nodes for f in frames])
    edges = np.cumsum([0] + [f.edge_index.size(1) for f in frames])
    for host, dev, want in ((packed.node_ptr_host, packed.node_ptr, nodes), (packed.edge_ptr_host, packed.edge_ptr, edges)):
        assert host.dtype == np.int64 and dev.dtype == torch.int64
        assert host.tolist() == want.tolist() == dev.tolist()
    assert packed.tables["edge_index"].shape == (2, edges[-1]) and packed.tables["loc_mean"].shape == (len(frames), 3, 3)
    assert int(packed.tables["edge_index"].max()) < max(f.num_nodes for f in frames)   # local ids


def test_getitem_returns_the_frames_as_views(frames, packed):
    for i, f in enumerate(frames):
        got = packed[i]
        for fld in fields(D.Frame):
            a, b = getattr(got, fld.name), getattr(f, fld.name)
            assert a.shape == b.shape and a.dtype == b.dtype and torch.equal(a, b), (i, fld.name)
    assert packed[5].loc_0.untyped_storage().data_ptr() == packed.tables["loc_0"].untyped_storage().data_ptr()
    assert torch.equal(packed[-1].loc_0, frames[-1].loc_0)
    for bad in (len(frames), -len(frames) - 1):
        with pytest.raises(IndexError):
            packed[bad]


def test_a_packed_dataset_feeds_the_old_loader(frames, packed):
    for got, want in zip(D.DataLoader(packed, batch_size=4), D.DataLoader(frames, batch_size=4)):
        assert_batches_equal(got, want)


def test_empty_sequence_raises():
    with pytest.raises(ValueError, match="empty"):
        D.PackedDataset([])


@pytest.mark.parametrize("what", ["node_feat width", "edge_attr width", "C", "float64 field", "int32 edge_index", "float16 field"])
def test_frames_that_do_not_fit_one_table_raise(frames, what):
    g = torch.Generator().manual_seed(1)
    odd = make_frame(4, 6, C=3, gen=g)
    if what == "node_feat width":
        odd = replace(odd, node_feat=torch.rand(4, 3))
    elif what == "edge_attr width":
        odd = replace(odd, edge_attr=torch.rand(6, 2))
    elif what == "C":
        odd = replace(odd, loc_mean=torch.rand(1, 3, 4))
    elif what == "float64 field":
        odd = replace(odd, vel_0=odd.vel_0.double())
    elif what == "int32 edge_index":
        odd = replace(odd, edge_index=odd.edge_index.int())
    else:
        odd = replace(odd, edge_attr=odd.edge_attr.half())
    with pytest.raises(ValueError, match="frame 2"):
        D.PackedDataset([frames[0], frames[1], odd])
    if "width" not in what and what != "C":   # a wrong dtype is wrong in a dataset of one frame too
        with pytest.raises(ValueError, match="frame 0"):
            D.PackedDataset([odd])


@pytest.mark.parametrize("ids", [[0, 23], [-1], np.array([3, 99]), torch.tensor([22, 23])])
def test_an_id_outside_the_dataset_raises_index_error(packed, ids):
    with pytest.raises(IndexError):
        packed.batch(ids)


def test_ids_that_are_no_id_list_raise_value_error(packed):
    for ids in ([], [[0, 1]], [0.5, 1.0]):
        with pytest.raises(ValueError):
            packed.batch(ids)


def test_batch_on_a_cpu_dataset_has_no_fallback(packed):
    assert packed.device.type == "cpu"
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        packed.batch([0, 1, 2])
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        next(iter(D.PackedLoader(packed, batch_size=4)))


@pytest.mark.parametrize("drop_last", [False, True])
@pytest.mark.parametrize("shuffle", [False, True])
def test_packed_loader_yields_the_batches_of_the_old_loader(frames, packed, torch_ops, shuffle, drop_last):
    gen = lambda: torch.Generator().manual_seed(11) if shuffle else None  # noqa: E731
    old = D.DataLoader(frames, batch_size=4, shuffle=shuffle, drop_last=drop_last, generator=gen())
    new = D.PackedLoader(packed, batch_size=4, shuffle=shuffle, drop_last=drop_last, generator=gen())
    assert len(new) == len(old) == (5 if drop_last else 6)
    got, want = list(new), list(old)
    assert len(got) == len(want) == len(old)
    for a, b in zip(got, want):
        assert_batches_equal(a, b)
    assert got[-1].num_graphs == (4 if drop_last else 3)


def test_shuffled_epochs_follow_the_generator_like_the_old_loader(frames, packed, torch_ops):
    """two epochs from ONE generator each: the second epoch's order is the generator's second draw in both loaders"""
    old = D.DataLoader(frames, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5))
    new = D.PackedLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(5))
    got, want = [list(new), list(new)], [list(old), list(old)]
    for epoch in range(2):
        assert len(got[epoch]) == len(want[epoch]) == 6
        for a, b in zip(got[epoch], want[epoch]):
            assert_batches_equal(a, b)
    assert not all(torch.equal(a["loc_0"], b["loc_0"]) for a, b in zip(got[0], got[1]))


def test_batch_with_repeats_and_any_order_equals_collate(frames, packed, torch_ops):
    for ids in ([3, 3, 0], list(range(22, -1, -1)), list(ZERO_EDGE_FRAMES), [6], np.array([5, 4], dtype=np.int32)):
        assert_batches_equal(packed.batch(ids), D.collate([frames[int(i)] for i in ids]))


def test_new_symbols_are_declared_bound_and_the_revision_stays():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    for name in ("fastegnn_collate_plan", "fastegnn_collate_gather"):
        assert re.search(r"\bint " + name + r"\(", src), name
        assert name in K.EXPORTED
    assert K.ABI_VERSION == 108
    assert "#define FASTEGNN_ABI_VERSION 108" in re.sub(r"[ \t]+", " ", src)
    assert re.search(r"#define FASTEGNN_COLLATE_TABLES 8\b", src) and len(D._PACK_KEYS) == 8
    import fastegnn_amd
    assert "PackedDataset" not in fastegnn_amd.__all__ and "PackedLoader" not in fastegnn_amd.__all__


def test_entry_points_reject_bad_arguments_before_any_launch():
    L = K.lib()
    SOME = C.c_void_p(64)
    tabs, w = (C.c_void_p * 8)(*([64] * 8)), (C.c_int32 * 7)(3, 3, 3, 2, 1, 1, 9)
    plan, gather = L.fastegnn_collate_plan, L.fastegnn_collate_gather
    for args, msg in [((SOME, -1, SOME, SOME, 5, SOME, SOME, None), b"B < 0"),
                      ((SOME, 4, SOME, SOME, 0, SOME, SOME, None), b"no frame"),
                      ((SOME, 4, SOME, SOME, 5, None, SOME, None), b"null output"),
                      ((None, 4, SOME, SOME, 5, SOME, SOME, None), b"null pointer")]:
        assert plan(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"collate_plan" in L.fastegnn_last_error()
    ok = [SOME, 4, SOME, SOME, 5, 100, 200, SOME, SOME, 40, 80, tabs, tabs, w, SOME, None]

    def bad(**kw):
        a = list(ok)
        for k, v in kw.items():
            a[int(k[1:])] = v
        return a
    wide = (C.c_int32 * 7)(3, 3, 3, 2, 1, 1, (1 << 20) + 1)
    holes = (C.c_void_p * 8)(*([64] * 7 + [None]))
    for args, msg in [(bad(a1=-1), b"B < 0"), (bad(a4=0), b"no frame"), (bad(a5=-1), b"negative size"), (bad(a10=-1), b"negative size"),
                      (bad(a0=None), b"null pointer"), (bad(a7=None), b"null pointer"), (bad(a13=None), b"null pointer"),
                      (bad(a13=wide), b"row width out of range"), (bad(a11=holes), b"null edge_index")]:
        assert gather(*args) == -1, msg
        assert msg in L.fastegnn_last_error() and b"collate_gather" in L.fastegnn_last_error()
    assert gather(*bad(a1=0)) == 0   # no frames: nothing to do, nothing launched
