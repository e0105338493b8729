"""-m gpu: ``copy.deepcopy`` and ``torch.save`` / ``torch.load(weights_only=False)`` of FastEGNN, FastRF and EGNN, on the fused and on
the wide path, before and after a forward (a guarded forward leaves host-mapped words behind a ctypes pointer in the module's
RangeGuard, and derived pointer tables).  Every copy is an independent module with an equal ``state_dict`` that computes the same
function -- outputs within the parity rule of tests/test_gpu_properties.py (1e-5 of the reference outputs, scale-relative) of the
original's, for FastEGNN on the fused path against the CPU oracle as well -- that allocates guard words of its own, and that trains."""
import copy
import ctypes as C
import io

import pytest
import torch

import fastegnn_amd
from oracle import fastegnn_ref as R
from tests.helpers import rel_err
from tests.test_gpu_properties import _batch, _models

pytestmark = pytest.mark.gpu

KINDS = {
    "FastEGNN": lambda: fastegnn_amd.FastEGNN(2, 0, 2, 64, 3, device="cuda", n_layers=2, gravity=[0.0, -1.0, 0.0]),
    "FastEGNN_wide": lambda: fastegnn_amd.FastEGNN(2, 0, 2, 128, 3, device="cuda", n_layers=2, gravity=[0.0, -1.0, 0.0]),
    "FastRF": lambda: fastegnn_amd.FastRF(2, 0, 2, 64, 3, device="cuda", n_layers=2),
    "FastRF_wide": lambda: fastegnn_amd.FastRF(2, 0, 2, 128, 3, device="cuda", n_layers=2),
    "EGNN": lambda: fastegnn_amd.EGNN(2, 2, 2, 64, device="cuda", with_v=True),
    "EGNN_wide": lambda: fastegnn_amd.EGNN(2, 2, 2, 128, device="cuda", with_v=True),
}


@pytest.fixture(scope="module")
def inputs():
    return {k: v.cuda() for k, v in _batch([7, 12, 9], 4, 3, seed=17).items()}


def _forward(m, inp):
    """-> the module's float outputs, as a tuple"""
    if type(m).__name__ == "EGNN":
        x, _, h = m(x=inp["node_loc"], h=inp["node_feat"], edge_index=inp["edge_index"], edge_fea=inp["edge_attr"], v=inp["node_vel"])
        return x, h
    return tuple(m(**inp))


def _pickled(m):
    buf = io.BytesIO()
    torch.save(m, buf)
    buf.seek(0)
    return torch.load(buf, weights_only=False)


def _words_address(m):
    w = m._range._words
    return None if w is None else C.addressof(w.contents)


def _check_copy(m, c, inp, want):
    assert type(c) is type(m) and c is not m and c._range is not m._range
    assert c._range._words is None                                     # the words are the original's: a copy allocates its own
    assert (c._range.wide, c._range.mode, c._range.forced) == (m._range.wide, m._range.mode, m._range.forced)
    sa, sb = m.state_dict(), c.state_dict()
    assert list(sa) == list(sb)
    assert all(torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr() for k in sa)
    out = _forward(c, inp)
    for a, b in zip(out, want):
        assert rel_err(a, b) < 1e-5
    if _words_address(m) is not None:                                  # a guarded path: the copy's forward made words of its own
        assert _words_address(c) not in (None, _words_address(m))
    sum(o.pow(2).sum() for o in out).backward()                        # the copy trains: its own parameters get the gradients
    assert sum(p.grad is not None for p in c.parameters()) > 2 and all(p.grad is None for p in m.parameters())
    return out


@pytest.mark.parametrize("kind", list(KINDS))
def test_copies_before_and_after_a_forward_compute_the_same_function(kind, inputs):
    torch.manual_seed(3)
    m = KINDS[kind]()
    early = copy.deepcopy(m), _pickled(m)                              # before any forward
    with torch.no_grad():
        want_eval = _forward(m, inputs)                                # the forward-only path (planned buffers) ...
    want = tuple(o.detach() for o in _forward(m, inputs))              # ... and the autograd path; both leave their caches behind
    for a, b in zip(want, want_eval):
        assert rel_err(a, b) < 1e-5
    for c in early + (copy.deepcopy(m), _pickled(m)):
        _check_copy(m, c, inputs, want)
    # independent: moving the original's parameters moves its outputs and not the copy's
    c = copy.deepcopy(m)
    with torch.no_grad():
        for p in m.parameters():
            p.mul_(1.5)
        moved, kept = _forward(m, inputs), _forward(c, inputs)
    assert rel_err(moved[0], want[0]) > 1e-3
    for a, b in zip(kept, want):
        assert rel_err(a, b) < 1e-5


def test_a_copy_of_the_fused_model_matches_the_oracle():
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=2)
    inp = _batch([7, 12, 9], 4, 3, seed=18)
    p, m = _models(cfg, seed=5)
    kw = {k: v.cuda() for k, v in inp.items()}
    m(**kw)[0].sum().backward()
    l32, v32 = R.forward(p, cfg, **inp)
    for c in (copy.deepcopy(m), _pickled(m)):
        loc, vloc = c(**kw)
        assert rel_err(loc, l32) < 1e-5 and rel_err(vloc, v32) < 1e-5


def test_a_copy_keeps_the_build_its_original_had_moved_to():
    m = KINDS["FastEGNN"]()
    if m._range.forced is not False:
        m._range.load_state_dict({"wide": True})
        assert m._range.wide
    m.deterministic = True
    c = copy.deepcopy(m)
    assert c._range.wide == m._range.wide and c.deterministic is True and c._range.warned == m._range.warned
