"""-m gpu: the ORDERED training loss (fastegnn_loss_mse_mmd_ordered, csrc/train.hip; ``mse_mmd_loss(..., ordered=True)``): no
floating-point atomics, every sum in an order fixed by (N, B, C, S) and the counts.

(1) values and gradients against float64 -- oracle.fastegnn_ref.loss_mse_mmd_nodes under autograd for full rows,
    tests/mmd_sampler_ref.mse_mmd_ragged_fp64 for ragged rows -- at the tolerances tests/test_gpu_train.py holds the atomic kernel to
    (test_loss_gradient_matches_oracle_autograd: 1e-5 absolute on loss and mse, rel_err < 1e-5 on both gradients);
(2) eight calls on the same inputs: identical bits in loss2, g_loc and g_vloc;
(3) invalid arguments are refused before any launch; B == 0 writes the MSE only.
"""
import ctypes as C

import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd.train import mse_mmd_loss
from oracle import fastegnn_ref as R
from tests.helpers import rel_err
from tests.mmd_sampler_ref import mse_mmd_ragged_fp64

pytestmark = pytest.mark.gpu

SIGMA, WEIGHT = 1.3, 0.7

# name: (nodes per graph, B, C, S, counts or None (every row full), coincident virtual nodes)
CASES = {
    "n60_b3_c5_s7_coincident": (20, 3, 5, 7, None, True),            # the case of test_loss_gradient_matches_oracle_autograd
    "ragged_0_3_S": (20, 3, 5, 7, [0, 3, 7], True),
    "one_channel": (20, 3, 1, 7, None, False),
    "c64_s300_rows_exceed_the_workgroup": (400, 2, 64, 300, None, False),
    "c64_s300_ragged_257": (400, 2, 64, 300, [300, 257], False),     # the stride loop's second pass, partly filled
    "n700_b1_several_mse_partials": (700, 1, 5, 7, None, False),      # 2100 elements: two MSE workgroups, no multiple of 256
}


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _inputs(name):
    n, B, Cn, S, counts, coincident = CASES[name]
    g = torch.Generator().manual_seed(4)
    N = n * B
    loc, tgt, vloc = torch.randn(N, 3, generator=g), torch.randn(N, 3, generator=g), torch.randn(B, 3, Cn, generator=g)
    if coincident:
        vloc[0, :, 1] = vloc[0, :, 0]                         # zero distance: zero subgradient
    samp = torch.stack([b * n + torch.randperm(n, generator=g)[:S] for b in range(B)]).to(torch.int32)
    cnt = None
    if counts is not None:
        cnt = torch.tensor(counts, dtype=torch.int32)
        samp = torch.where(torch.arange(S)[None, :] < cnt[:, None], samp, torch.full_like(samp, -1))   # as MMDSampler pads a row
    return loc, tgt, vloc, samp, cnt


@pytest.fixture(scope="module")
def reference():
    """{case: (loss, mse, g_loc, g_vloc)} in float64, computed once"""
    out = {}
    for name in CASES:
        loc, tgt, vloc, samp, cnt = _inputs(name)
        if cnt is None:
            a, v = loc.double().requires_grad_(True), vloc.double().requires_grad_(True)
            l, mse = R.loss_mse_mmd_nodes(a, v, tgt.double(), samp.long(), SIGMA, WEIGHT)
            l.backward()
            out[name] = (float(l.detach()), float(mse.detach()), a.grad, v.grad)
        else:
            r = mse_mmd_ragged_fp64(loc, vloc, tgt, samp, cnt, SIGMA, WEIGHT)
            out[name] = (float(r["loss"]), float(r["mse"]), r["g_loc"], r["g_vloc"])
    return out


def _call(loc, tgt, vloc, samp, cnt, ws_tensor=None, ws_doubles=None, over=None):
    """fastegnn_loss_mse_mmd_ordered on device tensors -> (rc, loss2, g_loc, g_vloc); `over` replaces arguments by name"""
    L, over = K.lib(), over or {}
    N, (B, _, Cn), S = loc.size(0), vloc.shape, samp.size(1)
    a = dict(N=N, B=B, C=Cn, S=S)
    a.update({k: v for k, v in over.items() if k in a})
    need = int(L.fastegnn_loss_ordered_ws_doubles(N, B))
    ws = torch.empty(need, dtype=torch.float64, device="cuda") if ws_tensor is None else ws_tensor
    loss2 = torch.full((2,), 7.0, device="cuda")
    g_loc, g_vloc = torch.full_like(loc, 9.0), torch.full_like(vloc, 9.0)
    p = dict(loc=K.ptr(loc), tgt=K.ptr(tgt), vloc=K.ptr(vloc), samp=K.ptr(samp), cnt=K.ptr(cnt), loss2=K.ptr(loss2), g_loc=K.ptr(g_loc),
             g_vloc=K.ptr(g_vloc), ws=K.ptr(ws))
    p.update({k: v for k, v in over.items() if k in p})
    rc = L.fastegnn_loss_mse_mmd_ordered(p["loc"], p["tgt"], p["vloc"], p["samp"], p["cnt"], a["N"], a["B"], a["C"], a["S"], SIGMA, WEIGHT,
                                         p["loss2"], p["g_loc"], p["g_vloc"], p["ws"], need if ws_doubles is None else ws_doubles, _st())
    return rc, loss2, g_loc, g_vloc


@pytest.mark.parametrize("name", list(CASES))
def test_ordered_loss_and_gradients_match_float64(name, reference):
    loc, tgt, vloc, samp, cnt = _inputs(name)
    l_ref, mse_ref, gl_ref, gv_ref = reference[name]
    a, v = loc.cuda().requires_grad_(True), vloc.cuda().requires_grad_(True)
    l, mse = mse_mmd_loss(a, v, tgt.cuda(), samp.cuda(), SIGMA, WEIGHT, None if cnt is None else cnt.cuda(), ordered=True)
    (2.0 * l).backward()
    e_l, e_m = abs(l.item() - l_ref), abs(float(mse) - mse_ref)
    e_a, e_v = rel_err(a.grad, 2 * gl_ref), rel_err(v.grad, 2 * gv_ref)
    print(f"{name}: |loss - fp64| {e_l:.3g}  |mse - fp64| {e_m:.3g}  rel_err g_loc {e_a:.3g}  g_vloc {e_v:.3g}")
    assert e_l < 1e-5 and e_m < 1e-5
    assert e_a < 1e-5 and e_v < 1e-5


@pytest.mark.parametrize("name", list(CASES))
def test_eight_calls_give_the_same_bits(name):
    loc, tgt, vloc, samp, cnt = (None if t is None else t.cuda() for t in _inputs(name))
    first = None
    for _ in range(8):
        rc, *got = _call(loc, tgt, vloc, samp, cnt)
        assert rc == 0
        if first is None:
            first = got
        assert all(torch.equal(x, y) for x, y in zip(first, got))
    assert bool(torch.isfinite(first[0]).all())


def test_workspace_query():
    L = K.lib()
    assert L.fastegnn_loss_ordered_ws_doubles(60, 3) == 1 + 3
    assert L.fastegnn_loss_ordered_ws_doubles(700, 1) == 2 + 1           # 2100 elements over workgroups of 2048
    assert L.fastegnn_loss_ordered_ws_doubles(100000, 1) == 147 + 1
    assert L.fastegnn_loss_ordered_ws_doubles(10 ** 7, 100) == 1024 + 100   # the grid's ceiling
    assert L.fastegnn_loss_ordered_ws_doubles(0, 0) == 1


def test_invalid_arguments_are_refused_before_any_launch():
    loc, tgt, vloc, samp, cnt = (None if t is None else t.cuda() for t in _inputs("ragged_0_3_S"))
    small = torch.empty(3, dtype=torch.float64, device="cuda")
    for what, kw in (("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("C < 0", dict(C=-1)), ("S < 0", dict(S=-1)), ("C > 256", dict(C=257)),
                     ("S > 4096", dict(S=4097)), ("null loss2", dict(loss2=None)), ("null ws", dict(ws=None)),
                     ("null loc_pred", dict(loc=None)), ("null loc_t", dict(tgt=None)), ("null vloc", dict(vloc=None)),
                     ("null sample_nodes", dict(samp=None)), ("null g_loc", dict(g_loc=None)), ("null g_vloc", dict(g_vloc=None))):
        rc, loss2, g_loc, g_vloc = _call(loc, tgt, vloc, samp, cnt, over=kw)
        assert rc == -1, what                                                  # FASTEGNN_E_INVALID
        assert bool((loss2 == 7).all()) and bool((g_loc == 9).all()) and bool((g_vloc == 9).all()), what   # nothing ran
    rc, loss2, g_loc, g_vloc = _call(loc, tgt, vloc, samp, cnt, ws_tensor=small, ws_doubles=3)
    assert rc == -1 and bool((loss2 == 7).all()) and bool((g_loc == 9).all())
    assert b"workspace" in K.lib().fastegnn_last_error()


def test_no_graph_writes_the_mse_only():
    loc, tgt, vloc, samp, cnt = (None if t is None else t.cuda() for t in _inputs("n60_b3_c5_s7_coincident"))
    rc, loss2, g_loc, g_vloc = _call(loc, tgt, vloc[:0].contiguous(), samp[:0].contiguous(), None)
    assert rc == 0
    d = loc.double() - tgt.double()
    mse = float((d * d).mean())
    assert abs(float(loss2[0]) - mse) < 1e-6 and torch.equal(loss2[0], loss2[1])
    assert rel_err(g_loc, 2 * d / d.numel()) < 1e-6
    assert bool((g_vloc == 9).all())
