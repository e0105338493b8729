"""-m gpu: the ORDERED mode of the wide path (`deterministic = True` with hidden_nf > 64, EGNN flat=True, the shapes beyond the fused
kernels' ceilings): fastegnn_wide_segment_sum_ordered / _linear_dw_ordered / _head_dw_ordered (csrc/wide.hip, csrc/wide_gemm.h).
(1) the ordered segment sum against the NumPy mirror of the order the header documents, bit for bit (tests/wide_det_ref.py), and
    against float64; (2) its activation form; (3) the ordered weight gradients against float64 at the ragged shapes of
    tests/test_gpu_wide.py; (4) every operator 8 times on the same inputs: identical bits; (5) whole models, fresh module state,
    5 forward + backward runs: every output and gradient identical; (6) the mode against the oracle under the wide path's rule, with
    the ratio to the PLAIN rule printed per case (DESIGN.md section 14 records it); (7) no warning.

Measured on an MI355X: worst ratio to the plain rule 0.66 (wide_det_h128), 1.14 (wide_det_h256), 0.98
(wide_det_h160_att), 0.38 (wide_det_ceilings); 68 tests in 6 s."""
import ctypes as C
import warnings

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from oracle import fastegnn_ref as R
from tests import wide_det_ref as M_
from tests.helpers import rel_err
from tests.test_gpu_properties import _batch, _compare_vs_oracle, _models, _oracle_results, _run_module

pytestmark = pytest.mark.gpu


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ws(nbytes):
    return torch.empty(max(nbytes, 16), dtype=torch.uint8, device="cuda")


def _repeat8(run):
    """`run` 8 times on the same inputs: every result tensor identical bit for bit -> the first result"""
    first = run()
    for _ in range(7):
        again = run()
        assert all(torch.equal(a, b) for a, b in zip(first, again))
    return first


def _segsum(idx_sorted, perm, rows, R_, kind=K.ACT_NONE, p=0.0):
    """-> (table,) or (table, y): a zeroed [R, W] table through fastegnn_wide_segment_sum_ordered"""
    L = K.lib()
    M, W = rows.shape
    nb = L.fastegnn_wide_segment_sum_ws_bytes(M, W)
    assert nb == M_.segment_sum_ws_bytes(M, W)
    ws = _ws(nb)

    def run():
        table = torch.zeros(R_, W, device="cuda")
        y = torch.full_like(rows, 9.0) if kind != K.ACT_NONE else None
        K.check(L.fastegnn_wide_segment_sum_ordered(K.ptr(table), K.ptr(idx_sorted), K.ptr(perm), M, W, K.ptr(rows), kind, p, K.ptr(y),
                                                    K.ptr(ws), nb, _st()), "segment_sum_ordered")
        return (table,) if y is None else (table, y)
    return _repeat8(run)


def _check_segsum(idx_sorted, perm, rows, R_):
    (table,) = _segsum(idx_sorted, perm, rows, R_)
    terms = rows if perm is None else rows[perm]
    mirror = M_.segment_sum_ordered(idx_sorted.cpu().numpy(), terms.cpu().numpy(), R_)
    assert np.array_equal(table.cpu().numpy(), mirror)
    ref = torch.zeros(R_, rows.size(1), dtype=torch.float64).index_add_(0, idx_sorted.cpu(), terms.double().cpu())
    assert rel_err(table.cpu(), ref) < 1e-6
    return table


@pytest.mark.parametrize("W", [136, 3, 1, 20, 2048])
def test_ordered_segment_sum_matches_the_documented_order(W):
    """3001 rows onto 400 targets, sorted and through a stable sorting permutation of an unsorted index; widths that are no multiple
    of 4, narrower than a lane group, wider than one workgroup's columns"""
    g = torch.Generator().manual_seed(W)
    R_, M = 400, 3001
    idx = torch.randint(0, R_, (M,), generator=g).cuda()
    rows = torch.randn(M, W, generator=g).cuda()
    sidx, perm = torch.sort(idx, stable=True)
    _check_segsum(sidx, None, rows, R_)
    t = _check_segsum(sidx, perm, rows, R_)
    assert rel_err(t.cpu(), torch.zeros(R_, W, dtype=torch.float64).index_add_(0, idx.cpu(), rows.double().cpu())) < 1e-6


@pytest.mark.parametrize("W", [136, 3])
def test_ordered_segment_sum_run_shapes(W):
    """what can break in the slot walk: one run through every slot, a run per row, two targets with untouched rows between, row counts
    around one slot's, no rows"""
    g = torch.Generator().manual_seed(10 + W)
    R_, M = 400, 3001
    rows = torch.randn(M, W, generator=g).cuda()
    rps = M_.rows_per_slot(M, W)
    assert rps == 16
    _check_segsum(torch.full((M,), 7, dtype=torch.long, device="cuda"), None, rows, R_)              # a chain across every slot
    _check_segsum(torch.arange(M, device="cuda"), None, rows, M)                                       # every row its own target
    two = torch.cat([torch.zeros(1500, dtype=torch.long), torch.full((M - 1500,), R_ - 1, dtype=torch.long)]).cuda()
    t = _check_segsum(two, None, rows, R_)
    assert not t[1:R_ - 1].any()                                                                       # rows nobody names stay zero
    # runs that end exactly on, one before and one behind slot boundaries
    edges = torch.tensor([0] * rps + [1] * (rps - 1) + [2] * (rps + 1) + [3] * (2 * rps) + [5] * 1 + [6] * (3 * rps - 1), device="cuda")
    _check_segsum(edges, None, rows[:edges.numel()].contiguous(), 8)
    for m in (rps - 1, rps, rps + 1, 1):
        idx = torch.sort(torch.randint(0, 5, (m,), generator=g))[0].cuda()
        _check_segsum(idx, None, rows[:m].contiguous(), 5)
        _check_segsum(torch.zeros(m, dtype=torch.long, device="cuda"), None, rows[:m].contiguous(), 5)
    # M = 0: nothing is touched (and no workspace is needed)
    L = K.lib()
    assert L.fastegnn_wide_segment_sum_ws_bytes(0, W) == 0
    table = torch.ones(R_, W, device="cuda")
    K.check(L.fastegnn_wide_segment_sum_ordered(K.ptr(table), None, None, 0, W, None, K.ACT_NONE, 0.0, None, None, 0, _st()), "M = 0")
    assert bool((table == 1).all())


@pytest.mark.parametrize("Wd", [128, 2048, 20])
def test_ordered_act_segment_sum_vs_float64(Wd):
    """the activation prologue: y = SiLU(z) stored and summed, sorted and through a permutation; tolerances of
    test_wide_rowwise_operators_vs_torch.  The table is also the documented sum of the STORED y, bit for bit."""
    g = torch.Generator().manual_seed(Wd)
    R_, M = 400, 3001
    idx = torch.randint(0, R_, (M,), generator=g).cuda()
    zz = torch.randn(M, Wd, generator=g).cuda()
    sidx, perm = torch.sort(idx, stable=True)
    yr = torch.nn.functional.silu(zz.double())
    for pm in (None, perm):
        tb, y = _segsum(sidx, pm, zz, R_, K.ACT_SILU)
        assert rel_err(y.cpu(), yr.cpu()) < 1e-6
        terms = yr if pm is None else yr[pm]
        assert rel_err(tb.cpu(), torch.zeros(R_, Wd, dtype=torch.float64).index_add_(0, sidx.cpu(), terms.cpu())) < 1e-6
        ys = y if pm is None else y[pm]
        assert np.array_equal(tb.cpu().numpy(), M_.segment_sum_ordered(sidx.cpu().numpy(), ys.cpu().numpy(), R_))


def _dw_ws(M, O, Kc):
    nb = K.lib().fastegnn_wide_linear_dw_ws_bytes(M, O, Kc)
    assert nb == 4 * M_.dw_splits(M, O, Kc)[2]
    return _ws(nb), nb


@pytest.mark.parametrize("M,K_,O,ldw,c0", [(1000, 128, 128, 300, 37), (777, 3, 96, 200, 190), (513, 160, 1, 160, 0),
                                           (300, 2048, 128, 2304, 256), (65, 1, 130, 261, 256), (0, 16, 16, 16, 0),
                                           (5000, 96, 160, 256, 5), (33, 130, 256, 130, 0), (2100, 9, 24, 40, 3),
                                           (3000, 128, 128, 128, 0), (7000, 3, 96, 200, 190)])
@pytest.mark.parametrize("kind", [K.ACT_NONE, K.ACT_SILU, K.ACT_TANH])
def test_ordered_linear_dw_vs_torch(M, K_, O, ldw, c0, kind):
    """the ragged shapes of test_wide_linear_forward_dx_dw_vs_torch (the block kernel and both small-side forms, plain and with the
    activation prologue) and two with at least three row ranges under the mode's own rule; += into ones: columns outside the block
    stay untouched, M = 0 touches nothing"""
    if M in (3000, 7000):
        assert M_.dw_splits(M, O, K_)[1] >= 3
    g = torch.Generator().manual_seed(M + K_ + O)
    X = torch.randn(M, K_, generator=g).cuda()
    G = torch.randn(M, O, generator=g).cuda()
    fn = (lambda t: t) if kind == K.ACT_NONE else {K.ACT_SILU: torch.nn.functional.silu, K.ACT_TANH: torch.tanh}[kind]
    L = K.lib()
    ws, nb = _dw_ws(M, O, K_)

    def run():
        dW = torch.ones(O, ldw, device="cuda")
        db = torch.ones(O, device="cuda")
        K.check(L.fastegnn_wide_linear_dw_ordered(K.ptr(G), K.ptr(X), M, O, K_, K.ptr(dW), ldw, c0, K.ptr(db), kind, 0.0, K.ptr(ws), nb, _st()),
                "linear_dw_ordered")
        return dW, db
    dW, db = _repeat8(run)
    refW = torch.ones(O, ldw, dtype=torch.float64)
    refW[:, c0:c0 + K_] += (G.double().t() @ fn(X.double())).cpu()
    assert rel_err(dW.cpu(), refW) < 3e-6                      # columns outside the block untouched
    assert rel_err(db.cpu(), 1 + G.double().sum(0).cpu()) < 3e-6
    outside = torch.ones(O, ldw, dtype=torch.bool)
    outside[:, c0:c0 + K_] = False
    assert bool((dW.cpu()[outside] == 1).all())
    if M == 0:
        assert bool((dW == 1).all()) and bool((db == 1).all())
    # either output alone
    dW2 = torch.ones(O, ldw, device="cuda")
    K.check(L.fastegnn_wide_linear_dw_ordered(K.ptr(G), K.ptr(X), M, O, K_, K.ptr(dW2), ldw, c0, None, kind, 0.0, K.ptr(ws), nb, _st()), "dW only")
    db2 = torch.ones(O, device="cuda")
    K.check(L.fastegnn_wide_linear_dw_ordered(K.ptr(G), K.ptr(X), M, O, K_, None, ldw, c0, K.ptr(db2), kind, 0.0, K.ptr(ws), nb, _st()), "db only")
    assert torch.equal(dW2, dW)
    assert rel_err(db2.cpu(), 1 + G.double().sum(0).cpu()) < 3e-6


@pytest.mark.parametrize("M,O,Kx", [(1000, 128, 128), (777, 96, 96), (4100, 256, 128), (500, 192, 224), (65, 160, 160), (0, 128, 128)])
@pytest.mark.parametrize("kind", [K.ACT_SILU, K.ACT_TANH])
def test_ordered_head_dw_vs_torch(M, O, Kx, kind):
    """fastegnn_wide_head_dw_ordered at the shapes of test_wide_head_backward_vs_torch: dW1, db1 and dw2 of a scalar head from its
    output gradient, against the products of the materialised hidden gradient in float64"""
    g = torch.Generator().manual_seed(M + O + Kx)
    fn = {K.ACT_SILU: torch.nn.functional.silu, K.ACT_TANH: torch.tanh}[kind]
    gs = torch.randn(M, generator=g).cuda()
    w2 = torch.randn(O, generator=g).cuda()
    Zc = torch.randn(M, O, generator=g).cuda()
    X = torch.randn(M, Kx, generator=g).cuda()
    ldw, c0 = Kx + 7, 3
    zz = Zc.double().requires_grad_(True)
    fn(zz).sum().backward()
    Gd = gs.double().unsqueeze(1) * w2.double().unsqueeze(0) * (zz.grad if M else torch.zeros_like(zz))
    L = K.lib()
    ws, nb = _dw_ws(M, O, Kx)

    def run():
        dW = torch.ones(O, ldw, device="cuda")
        db = torch.ones(O, device="cuda")
        dw2 = torch.ones(O, device="cuda")
        K.check(L.fastegnn_wide_head_dw_ordered(K.ptr(gs), K.ptr(w2), K.ptr(Zc), K.ptr(X), M, O, Kx, K.ptr(dW), ldw, c0, K.ptr(db), K.ptr(dw2),
                                                kind, 0.0, K.ACT_NONE, 0.0, K.ptr(ws), nb, _st()), "head_dw_ordered")
        return dW, db, dw2
    dW, db, dw2 = _repeat8(run)
    if M == 0:
        assert bool((dW == 1).all()) and bool((db == 1).all()) and bool((dw2 == 1).all())
        return
    refW = torch.ones(O, ldw, dtype=torch.float64)
    refW[:, c0:c0 + Kx] += (Gd.t() @ X.double()).cpu()
    assert rel_err(dW.cpu(), refW) < 3e-6
    assert rel_err(db.cpu(), 1 + Gd.sum(0).cpu()) < 3e-6
    assert rel_err(dw2.cpu(), 1 + (gs.double().unsqueeze(1) * fn(Zc.double())).sum(0).cpu()) < 3e-6
    assert bool((dW[:, :c0] == 1).all()) and bool((dW[:, c0 + Kx:] == 1).all())


# ---- whole models: 5 runs, fresh module state, every output and gradient identical ---------------------------------------------------

def _five_identical(make, inputs, call):
    """make() -> a fresh module; call(module, leaves) -> tuple of outputs; gradients of every parameter and every leaf"""
    first = None
    for _ in range(5):
        m = make()
        m.deterministic = True
        leaves = {k: (v.clone().cuda().requires_grad_(True) if v.is_floating_point() else v.cuda()) for k, v in inputs.items()}
        with warnings.catch_warnings(record=True) as caught:
            warnings.simplefilter("always")
            outs = call(m, leaves)
            sum(o.pow(2).mean() for o in outs).backward()
        assert not [str(w.message) for w in caught if "fastegnn_amd" in str(w.message) or "fastegnn_amd" in str(w.filename)]
        got = {"out%d" % i: o.detach() for i, o in enumerate(outs)}
        got.update({"p/" + k: v.grad for k, v in m.named_parameters() if v.grad is not None})
        got.update({"in/" + k: v.grad for k, v in leaves.items() if v.is_floating_point() and v.grad is not None})
        if first is None:
            first = got
            assert len([k for k in got if k.startswith("p/")]) > 10 and ("in/node_loc" in got or "in/x" in got)
        else:
            assert got.keys() == first.keys()
            diff = [k for k in got if not torch.equal(got[k], first[k])]
            assert not diff, diff
    torch.cuda.synchronize()


def _fast_case(cfg, inp, seed, cls=None):
    p = R.init_params(cfg, seed=seed, coord_gain=0.05)
    cls = cls or fastegnn_amd.FastEGNN

    def make():
        m = cls(cfg.node_feat_nf, cfg.node_attr_nf, cfg.edge_attr_nf, cfg.hidden_nf, cfg.virtual_channels, device="cuda",
                n_layers=cfg.n_layers, attention=cfg.attention, gravity=cfg.gravity)
        m.load_state_dict({k: v for k, v in p.items() if k in m.state_dict()}, strict=True)
        assert m._wide
        return m
    _five_identical(make, inp, lambda m, kw: m(**kw))


def _shuffled_nodes(inp, seed):
    """the same batch with its nodes in a random order: data_batch is no longer monotone"""
    N = inp["node_loc"].size(0)
    perm = torch.randperm(N, generator=torch.Generator().manual_seed(seed))
    inv = torch.empty_like(perm)
    inv[perm] = torch.arange(N)
    out = dict(inp)
    for k in ("node_feat", "node_loc", "node_vel", "data_batch"):
        out[k] = inp[k][perm].contiguous()
    out["edge_index"] = inv[inp["edge_index"]].contiguous()
    assert not bool((out["data_batch"][1:] >= out["data_batch"][:-1]).all())
    return out


@pytest.mark.parametrize("case", ["h128_att", "one_graph", "h256", "ceilings", "fastrf", "batch_not_monotone"])
def test_ordered_mode_repeats_bit_for_bit(case):
    grav = [0.3, -1, 0.2]
    if case == "h128_att":
        _fast_case(R.Config(2, 0, 2, 128, 3, n_layers=2, attention=True, gravity=grav), _batch([300, 141, 77], 6, 3, seed=1), 1)
    elif case == "one_graph":
        _fast_case(R.Config(2, 0, 2, 128, 3, n_layers=2, attention=True, gravity=grav), _batch([700], 6, 3, seed=2), 2)
    elif case == "h256":
        _fast_case(R.Config(2, 0, 2, 256, 3, n_layers=2, attention=True, gravity=grav), _batch([300, 141, 77], 6, 3, seed=3), 3)
    elif case == "ceilings":
        _fast_case(R.Config(2, 0, 2, 64, 70, n_layers=2, gravity=grav), _batch([150, 60], 5, 70, seed=4), 4)
    elif case == "fastrf":
        inp = _batch([300, 141, 77], 6, 3, seed=5)

        def make():
            torch.manual_seed(5)
            m = fastegnn_amd.FastRF(2, 0, 2, 128, 3, device="cuda", n_layers=2, attention=True, gravity=grav)
            with torch.no_grad():   # (the reference's gain-0.001 coordinate heads: scaled so that their gradients are not all rounding)
                for k, q in m.named_parameters():
                    if k.endswith(("coord_mlp_r.2.weight", "coord_mlp_r_virtual.2.weight", "coord_mlp_v_virtual.2.weight")):
                        q.mul_(50.0)
            assert m._wide
            return m
        _five_identical(make, inp, lambda m, kw: m(**kw))
    else:
        _fast_case(R.Config(2, 0, 2, 128, 3, n_layers=2, attention=True, gravity=grav), _shuffled_nodes(_batch([300, 141, 77], 6, 3, seed=6), 6), 6)


@pytest.mark.parametrize("flat", [False, True])
def test_ordered_mode_egnn_repeats_bit_for_bit(flat):
    g = torch.Generator().manual_seed(11)
    N, E = 400, 2400
    inp = dict(x=torch.randn(N, 3, generator=g), h=torch.rand(N, 2, generator=g), edge_index=torch.randint(0, N, (2, E), generator=g),
               edge_fea=torch.rand(E, 2, generator=g), v=torch.randn(N, 3, generator=g) * 0.3)

    def make():
        torch.manual_seed(11)
        return fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=32 if flat else 128, device="cuda", with_v=True, flat=flat)

    def call(m, kw):
        x, _, h = m(kw["x"], kw["h"], kw["edge_index"], kw["edge_fea"], kw["v"])
        return x, h
    _five_identical(make, inp, call)


def test_ordered_mode_raises_no_warning():
    """`deterministic = True` on a wide module used to be answered with a RuntimeWarning: the request is honoured now"""
    inp = _batch([40, 25], 4, 2, seed=8)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 96, 2, device="cuda", n_layers=1)
    m.deterministic = True
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loc, vloc = m(**{k: v.cuda() for k, v in inp.items()})
        (loc.pow(2).mean() + vloc.pow(2).mean()).backward()
    assert not [str(w.message) for w in caught if "fastegnn_amd" in str(w.message) or "fastegnn_amd" in str(w.filename)]
    assert m._wide_ordered.ws_bytes() > 0


# ---- the mode against the oracle -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("case,hidden,C_,flags", [("wide_det_h128", 128, 3, dict(gravity=[0, -1, 0])),
                                                 ("wide_det_h256", 256, 3, dict(gravity=[0, -1, 0])),
                                                 ("wide_det_h160_att", 160, 3, dict(attention=True, act="gelu")),
                                                 ("wide_det_ceilings", 64, 70, dict(gravity=[0, -1, 0]))])
def test_ordered_mode_vs_oracle(case, hidden, C_, flags):
    """the ordered path under the wide path's rule (tests/helpers.py, the r"wide_" entry).  The ratio of every tensor's error to the
    PLAIN rule (2 x the fp32 reference's own error + 1e-6) is printed: a measurement, recorded in DESIGN.md section 14."""
    cfg = R.Config(2, 0, 2, hidden, C_, n_layers=2, **flags)
    inp = _batch([150, 60], 5, C_, seed=hidden + C_) if C_ > 64 else _batch([300, 141, 77], 6, C_, seed=hidden)
    p, m = _models(cfg, hidden)
    m.deterministic = True
    assert m._wide
    tgt = inp["node_loc"] + 0.5
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        loc, vloc, got = _run_module(m, inp, tgt)
    assert not [str(w.message) for w in caught if "fastegnn_amd" in str(w.message) or "fastegnn_amd" in str(w.filename)]
    res = _oracle_results(cfg, p, inp, tgt)
    _, _, g32 = res[torch.float32]
    _, _, g64 = res[torch.float64]
    ratios = {k: rel_err(got[k], g64[k]) / (2.0 * rel_err(g32[k], g64[k]) + 1e-6) for k in g64}
    worst = max(ratios, key=ratios.get)
    print(f"\n[{case}] worst ratio to the plain rule: {ratios[worst]:.3f} ({worst})")
    _compare_vs_oracle(case, cfg, p, inp, tgt, loc, vloc, got)
