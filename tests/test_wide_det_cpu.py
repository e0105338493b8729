"""CPU: the ORDERED mode of the wide path (`deterministic = True` on hidden_nf > 64 / EGNN flat=True) through a torch restatement of
the ordered operators (test infrastructure, as tests/test_wide_cpu.py is for the atomic ones) and a call recorder.  What this pins
without a GPU: with the flag set no warning is raised, none of the atomic operators is called and every segment sum is handed a
SORTED index; outputs and gradients still match the goldens; with the flag unset the operator sequence is the one recorded before the
mode existed (tests/golden/wide_h128_op_sequence.txt)."""
import os
import warnings

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import wide
from tests.helpers import Golden, check_parity, golden_loss, rel_err
from tests.test_wide_cpu import TorchOps, _fn

ATOMIC = {"scatter_add", "scatter_add_perm", "act_scatter", "linear_dw", "head_dw"}
ORDERED = {"segment_sum_ordered", "linear_dw_ordered", "head_dw_ordered"}


class RecordingOps(TorchOps):
    """TorchOps + the ordered entry points of include/fastegnn_hip.h, every call's name kept in `calls`"""
    calls = []

    @staticmethod
    def call(name, *a):
        RecordingOps.calls.append(name)
        getattr(RecordingOps, name)(*a)

    @staticmethod
    def query(name, *a):
        assert name in ("segment_sum_ws_bytes", "linear_dw_ws_bytes") and all(isinstance(v, int) for v in a)
        return 64

    @staticmethod
    def segment_sum_ordered(table, idx_sorted, perm, M, W, rows, kind, p, y, ws, ws_bytes):
        assert idx_sorted.numel() == M and rows.shape == (M, W) and ws is not None and ws.numel() >= ws_bytes
        assert bool((idx_sorted[1:] >= idx_sorted[:-1]).all()), "the ordered segment sum needs a sorted index"
        assert (kind == K.ACT_NONE) == (y is None)
        r = rows
        if y is not None:
            y.copy_(_fn(kind, p)(rows))
            r = y
        table.index_add_(0, idx_sorted, r if perm is None else r[perm])

    @staticmethod
    def linear_dw_ordered(G, X, M, O, Kc, dW, ldw, c0, db, kind, p, ws, ws_bytes):
        assert ws is not None and ws.numel() >= ws_bytes
        TorchOps.linear_dw(G, X, M, O, Kc, dW, ldw, c0, db, kind, p)

    @staticmethod
    def head_dw_ordered(gs, w2, Zc, X, M, O, Kc, dW, ldw, c0, db, dw2, kind, p, x_kind, x_p, ws, ws_bytes):
        assert ws is not None and ws.numel() >= ws_bytes
        TorchOps.head_dw(gs, w2, Zc, X, M, O, Kc, dW, ldw, c0, db, dw2, kind, p, x_kind, x_p)


@pytest.fixture
def rec(monkeypatch):
    monkeypatch.setattr(wide, "_OPS", RecordingOps)
    RecordingOps.calls = []
    return RecordingOps


def _assert_ordered_only(rec, caught):
    assert not [str(w.message) for w in caught if issubclass(w.category, RuntimeWarning)]
    used = set(rec.calls)
    assert not used & ATOMIC, used & ATOMIC
    assert {"segment_sum_ordered", "linear_dw_ordered"} <= used


def _fastegnn(det):
    from tests.gpu_util import model_from_golden
    g = Golden("wide_h128_two_graphs")
    m = model_from_golden(g, device="cpu")
    m.deterministic = det
    kw, target, wv = g.model_kwargs()
    leaf = {k: kw[k].clone().requires_grad_(True) for k in ("node_feat", "node_loc", "node_vel", "loc_mean")}
    kw.update(leaf)
    loc, vloc = wide.forward(m, **kw)
    golden_loss(loc, vloc, target, wv).backward()
    G = {k: (p.grad if p.grad is not None else torch.zeros_like(p)) for k, p in m.named_parameters()}
    return check_parity(g, loc.detach(), vloc.detach(), G, {k: v.grad for k, v in leaf.items()})


def test_ordered_fastegnn_calls_no_atomic_operator_and_matches_the_golden(rec):
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        msgs = _fastegnn(True)
    _assert_ordered_only(rec, caught)
    assert "head_dw_ordered" in rec.calls
    assert not msgs, msgs


def test_ordered_fastegnn_with_a_batch_vector_that_is_not_monotone(rec):
    """data_batch is sorted like col in this mode: nodes of the two graphs interleaved give the outputs of the sorted batch, permuted"""
    from tests.gpu_util import model_from_golden
    g = Golden("wide_h128_two_graphs")
    kw, _, _ = g.model_kwargs()
    N = kw["node_loc"].size(0)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(1))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    kw2 = dict(kw)
    for k in ("node_feat", "node_loc", "node_vel", "data_batch"):
        kw2[k] = kw[k][perm]
    kw2["edge_index"] = inv[kw["edge_index"]]
    assert not bool((kw2["data_batch"][1:] >= kw2["data_batch"][:-1]).all())
    outs = []
    for args in (kw, kw2):
        m = model_from_golden(g, device="cpu")
        m.deterministic = True
        outs.append(wide.forward(m, **args))
    assert not set(rec.calls) & ATOMIC
    assert rel_err(outs[1][0][inv], outs[0][0]) < 1e-5 and rel_err(outs[1][1], outs[0][1]) < 1e-5


def test_ordered_fastrf_calls_no_atomic_operator_and_matches_the_golden(rec):
    from tests.gpu_util import model_from_golden
    g = Golden("fastrf_h128")
    m = model_from_golden(g, device="cpu", cls=fastegnn_amd.FastRF)
    m.deterministic = True
    kw, target, wv = g.model_kwargs()
    kw.pop("node_attr")
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loc, vloc = wide.forward(m, **kw)
        golden_loss(loc, vloc, target, wv).backward()
    _assert_ordered_only(rec, caught)
    assert rel_err(loc, g.out["loc"]) < 1e-5 and rel_err(vloc, g.out["vloc"]) < 1e-5
    for k, p in m.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        assert rel_err(got, g.gp[k]) < 5e-5, (k, rel_err(got, g.gp[k]))


@pytest.mark.parametrize("name", ["egnn_flat", "egnn_h128"])
def test_ordered_egnn_calls_no_atomic_operator_and_matches_the_golden(rec, name):
    from tests.test_egnn_oracle_cpu import egnn_loss, load_egnn
    g = load_egnn(name)
    m = fastegnn_amd.EGNN(n_layers=int(g["meta"]["L"]), in_node_nf=2, in_edge_nf=2, hidden_nf=int(g["meta"]["hidden"]),
                          with_v=bool(int(g["meta"]["with_v"])), norm=bool(int(g["meta"]["norm"])), flat=bool(int(g["meta"]["flat"])))
    m.load_state_dict(g["p"], strict=True)
    m.deterministic = True
    i = g["in"]
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        x, h = wide.egnn_forward(m, i["x"], i["h"], i["edge_index"], i["edge_fea"], i.get("v"))
        egnn_loss(x, h, i["target"], i["wh"]).backward()
    _assert_ordered_only(rec, caught)
    assert rel_err(x, g["out"]["x"]) < 1e-5 and rel_err(h, g["out"]["h"]) < 2e-5
    for k, p in m.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        assert rel_err(got, g["gp"][k]) < 5e-5, (k, rel_err(got, g["gp"][k]))


def test_default_mode_runs_the_operator_sequence_recorded_before_the_ordered_mode(rec):
    """flag unset: the same operators in the same order as before the mode existed (forward + backward of wide_h128_two_graphs)"""
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "wide_h128_op_sequence.txt")
    want = open(path).read().split()
    msgs = _fastegnn(None)
    assert not msgs, msgs
    assert not set(rec.calls) & ORDERED
    assert rec.calls == want
