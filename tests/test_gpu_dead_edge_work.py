"""-m gpu: edge-stage work of the first and last layer that no result reads (include/fastegnn_hip.h).

  * last layer (h_out / HvT_out and g_h_out / g_HvT_out null): the layer calls build no aggm and neither fill nor read the zero rows of g_h;
  * first layer: g_x / g_Z null when node_loc / loc_mean need no gradient (g_vel null in every layer when node_vel needs none) -- no coordinate
    adjoint in the edge stage, no g_x carried through the virtual stage;
  * the column scatter of every layer goes into a Q block [N,64] + x block [N,4] (two 128-byte lines per edge).

FASTEGNN_KEEP_DEAD_EDGE_WORK=1 (read per call by the model and by the library) runs the unspecialised stages with every pointer set: every
comparison here is the default path against that switch in one process -- loc, vloc, every parameter gradient and the wanted input gradients,
the same set of Nones on both sides -- under the rule of tests/test_gpu_last_layer_skip.py: four times the largest difference between two KEEP
runs of the shape, at least 1e-6, never above 1e-5.  The virtual nodes start off the centroid (that module's docstring).  Which path ran is
read from the library's path counters (fastegnn_path_counts).

The null g_x / g_Z convention and the split scatter rows belong to the atomic scatter; graphs of at most 512 edges take the order-independent
(store + reduce) form by default, so the small cases set `deterministic = False` to reach them.

Measured on an MI355X (largest difference over the tensors of a case: two KEEP runs | default against KEEP): see profiles/dead_edge_work.txt
section 6."""
import ctypes as C
import os

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from oracle import fastegnn_ref as R
from tests import test_gpu_last_layer_skip as S
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

SWITCH = "FASTEGNN_KEEP_DEAD_EDGE_WORK"
INPUTS = ("node_loc", "node_vel", "loc_mean")


class _switch:
    def __init__(self, keep):
        self.keep = keep

    def __enter__(self):
        self.old = os.environ.get(SWITCH)
        os.environ[SWITCH] = "1" if self.keep else "0"

    def __exit__(self, *exc):
        if self.old is None:
            os.environ.pop(SWITCH, None)
        else:
            os.environ[SWITCH] = self.old


def _step(m, inp, tgt, keep, req=()):
    """one forward + backward with `req` of INPUTS requiring a gradient -> ({name: tensor or None}, the path counters of the step)"""
    with _switch(keep):
        for p in m.parameters():
            p.grad = None
        kw = dict(inp)
        for k in req:
            kw[k] = inp[k].clone().requires_grad_(True)
        K.path_counts()
        loc, vloc = m(**kw)
        S._loss(loc, vloc, tgt).backward()
        torch.cuda.synchronize()
        paths = K.path_counts()
        out = {"loc": loc.detach().clone(), "vloc": vloc.detach().clone()}
        for k in INPUTS:
            out["g." + k] = kw[k].grad.clone() if k in req and kw[k].grad is not None else None
            assert (out["g." + k] is not None) == (k in req), k      # asked for: there; not asked for: None
        out.update({"grad." + n: (p.grad.clone() if p.grad is not None else None) for n, p in m.named_parameters()})
    return out, paths


def _expected_paths(m, keep, req, det):
    """layer calls of one step per path"""
    if keep:
        return dict(no_aggm=0, zero_gaggm=0, no_gx=0, split_gqx=0)
    return dict(no_aggm=1, zero_gaggm=1, no_gx=0 if det or "node_loc" in req else 1, split_gqx=0 if det else m.n_layers)


def _compare(tag, m, inp, tgt, req=(), det=False):
    """KEEP twice (the shape's own run-to-run difference), then the default path against KEEP under four times that"""
    (k0, p0), (k1, _) = _step(m, inp, tgt, True, req), _step(m, inp, tgt, True, req)
    assert p0 == _expected_paths(m, True, req, det), p0
    noise = max(S._diffs(k0, k1).values())
    bound = min(S.CEIL, max(4.0 * noise, S.FLOOR))
    on, paths = _step(m, inp, tgt, False, req)
    assert paths == _expected_paths(m, False, req, det), paths          # the specialised paths ran
    d = S._diffs(on, k0)                                                # (asserts the same set of Nones)
    for k, v in on.items():
        if v is not None:
            assert torch.isfinite(v).all(), k
    worst = max(d.values())
    print(f"dead_edge_work[{tag}]: keep-vs-keep max {noise:.3e}, default-vs-keep max {worst:.3e} ({max(d, key=d.get)}; tensors {len(d)}), "
          f"bound {bound:.1e}")
    bad = {k: v for k, v in d.items() if v > bound}
    assert not bad, (bad, bound)
    return on, bound


def _atomic_model(C_, L, att=False, **extra):
    _, m = S._model(C_, L, att, **extra)
    m.deterministic = False        # the atomic scatter on a graph of <= 512 edges as well: the form the null g_x convention belongs to
    return m


# ---- 1. the ragged 60-node batch, inputs without requires_grad ----------------------------------------------------------------
@pytest.mark.parametrize("C_,L,att,bf16", [(3, 2, False, False), (3, 1, False, False), (3, 2, True, False), (16, 2, False, False),
                                          (3, 2, False, True)],
                         ids=["C3-L2", "C3-L1", "C3-L2-attention", "C16-L2", "C3-L2-bf16"])
def test_small_ragged_batch_default_matches_keep(C_, L, att, bf16):
    """L = 1: the only layer is first and last.
    C3-L2-bf16 FAILED in two of three visits to an MI355X, both times on 2.634e-5 at gcl_0.edge_mlp_virtual.0.weight against the 1e-5 ceiling: once its
    two KEEP runs were the pair that differed (default-vs-KEEP the same figure), once the default run against two agreeing KEEP runs (5.1e-7
    apart); 6.7e-7 | 6.7e-7 in the third.  One bf16 operand sits on a rounding tie that flips with the arrival order of the pools' atomics, in the
    baseline as in the change (DESIGN.md sections 6 and 20); the bound is not widened."""
    m = _atomic_model(C_, L, att, **({"mlp_dtype": torch.bfloat16} if bf16 else {}))
    inp = {k: v.cuda() for k, v in S._small(C_).items()}
    _compare(f"C{C_}-L{L}-att{int(att)}-bf{int(bf16)}", m, inp, inp["node_loc"] + 0.5)


def test_small_ragged_batch_deterministic_form_keeps_the_last_layer_part():
    """the default of a small graph (store + reduce): the last layer's part runs, the null g_x convention does not"""
    _, m = S._model(3, 2)
    inp = {k: v.cuda() for k, v in S._small(3).items()}
    _compare("C3-L2-det", m, inp, inp["node_loc"] + 0.5, det=True)


# ---- 2. input gradients ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("req", [("node_loc",), ("node_vel",), ("loc_mean",), INPUTS], ids=["node_loc", "node_vel", "loc_mean", "all"])
def test_input_gradients_asked_for_are_there_the_others_none(req):
    """only node_loc: g_x wanted (no null g_x), g_Z null; only node_vel: both null, g_vel set; only loc_mean: g_Z wanted, g_x not"""
    m = _atomic_model(3, 2)
    inp = {k: v.cuda() for k, v in S._small(3).items()}
    _compare("req-" + "+".join(req), m, inp, inp["node_loc"] + 0.5, req)


# ---- 3. edge walks ---------------------------------------------------------------------------------------------------------
def _walk_case(rows, cols, N=37, C_=3, seed=11):
    g = torch.Generator().manual_seed(seed)
    ei = torch.tensor([rows, cols], dtype=torch.long).view(2, -1)
    loc = torch.randn(N, 3, generator=g) * 2.0
    vstart = loc.mean(0).view(1, 3, 1) + 0.5 * torch.randn(1, 3, C_, generator=g)
    return dict(node_feat=torch.rand(N, 2, generator=g), node_loc=loc, node_vel=torch.randn(N, 3, generator=g) * 0.3, edge_index=ei,
                data_batch=torch.zeros(N, dtype=torch.long), loc_mean=vstart, edge_attr=torch.rand(ei.size(1), 2, generator=g))


_N = 37
_WALKS = {
    # one partial tile: the nvalid < 16 atomic path; columns 0 and N - 1 (the last Q row borders the x block of the split layout)
    "five-edges": ([5, 5, 9, 9, 30], [0, _N - 1, 3, 0, _N - 1]),
    # one row of 40 edges over three tiles, rows without edges before the first and after the last row that has any
    "row-of-40": ([10] * 40, [c for c in range(_N) if c != 10] + [0, _N - 1, 1, 2]),
    # 32 edges whose row boundary falls on the tile boundary
    "boundary-on-tile": ([3] * 16 + [20] * 16, [0, _N - 1] + list(range(4, 18)) + [_N - 1, 0] + list(range(21, 35))),
    "no-edges": ([], []),
}


@pytest.mark.parametrize("case", list(_WALKS))
def test_edge_walks_default_matches_keep(case):
    rows, cols = _WALKS[case]
    assert len(rows) == len(cols) and (not rows or (0 in cols and _N - 1 in cols))
    m = _atomic_model(3, 2)
    inp = {k: v.cuda() for k, v in _walk_case(rows, cols).items()}
    _compare("walk-" + case, m, inp, inp["node_loc"] + 0.5)


# ---- 4. the phased backward ------------------------------------------------------------------------------------------------
def test_phased_backward_default_matches_keep():
    """virt_bwd_cs_kernel<.., GX = false> (layer 0, with NODE = true) and <.., NODE = false> (layer 1) at the smallest size where the phased
    form is the default: a radius graph, C = 16, L = 2."""
    torch.manual_seed(43)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, 16, device="cuda", n_layers=2, gravity=[0, -1, 0])
    frame, tgt = S._radius_frame(S.N_PHASED, 16, 43)
    lib = K.lib()
    lib.fastegnn_spin_timeouts(1)
    lib.fastegnn_profile_enable(1)
    K.profile_collect()
    try:
        _compare("phased", m, frame, tgt)
        torch.cuda.synchronize()
        prof = K.profile_collect()
    finally:
        lib.fastegnn_profile_enable(0)
    # three steps of two layers, every one of them through the phased kernel (no Gv stage); the stage ids keep their launch counts
    assert prof.get("virt_bwd_kernel", (0, 0))[1] == 6 and "virt_bwd_gv_kernel" not in prof, prof
    assert prof.get("edge_bwd_kernel", (0, 0))[1] == 6 and prof.get("virt_bwd_node_kernel", (0, 0))[1] == 6, prof
    assert lib.fastegnn_spin_timeouts(1) == 0


# ---- 5. captured ------------------------------------------------------------------------------------------------------------
def test_captured_graph_replays_match_eager():
    """the default step captured with torch.cuda.graph and replayed three times, against eager, under the shape's bound"""
    m = _atomic_model(3, 2)
    inp = {k: v.cuda() for k, v in S._small(3).items()}
    tgt = inp["node_loc"] + 0.5
    eager, bound = _compare("capture", m, inp, tgt)
    with _switch(False):
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):   # warm-up on the side stream (allocator, lazy state)
                for p in m.parameters():
                    p.grad = None
                loc, vloc = m(**inp)
                S._loss(loc, vloc, tgt).backward()
        torch.cuda.current_stream().wait_stream(s)
        for p in m.parameters():
            p.grad = None
        K.path_counts()
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loc, vloc = m(**inp)
            S._loss(loc, vloc, tgt).backward()
        assert K.path_counts() == _expected_paths(m, False, (), False)
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    got = {"loc": loc.detach(), "vloc": vloc.detach()}
    got.update({"grad." + n: p.grad for n, p in m.named_parameters()})
    for k, v in got.items():
        assert (v is None) == (eager[k] is None), k
        if v is not None:
            assert rel_err(v, eager[k]) <= bound, (k, rel_err(v, eager[k]), bound)


# ---- 6. the oracle ------------------------------------------------------------------------------------------------------------
def test_small_shape_vs_oracle():
    """the default path against the CPU oracle with the suite's calibrated tolerances, unchanged"""
    from tests import test_gpu_properties as P
    assert os.environ.get(SWITCH, "0") in ("", "0")
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=2, gravity=[0, -1, 0])
    K.path_counts()
    P._check_vs_oracle(cfg, S._small(3), seed=7, case="dead_edge_work_small")
    paths = K.path_counts()
    assert paths["no_aggm"] == 1 and paths["zero_gaggm"] == 1 and paths["no_gx"] == 0, paths      # (<= 512 edges: store + reduce)


def test_small_shape_vs_oracle_atomic_scatter(monkeypatch):
    """the same comparison with the atomic scatter (FASTEGNN_DETERMINISTIC=0 when the checker builds its model): the null g_x / g_Z first layer
    and the split scatter rows against a reference that shares no code with them"""
    from tests import test_gpu_properties as P
    assert os.environ.get(SWITCH, "0") in ("", "0")
    monkeypatch.setenv("FASTEGNN_DETERMINISTIC", "0")
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=2, gravity=[0, -1, 0])
    K.path_counts()
    P._check_vs_oracle(cfg, S._small(3), seed=7, case="dead_edge_work_small_atomic")
    assert K.path_counts() == dict(no_aggm=1, zero_gaggm=1, no_gx=1, split_gqx=2)


# ---- 7. argument checks ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("flag", [K.F_DETERMINISTIC, K.F_RF, K.F_EGNN], ids=["deterministic", "fastrf", "egnn"])
def test_null_g_x_is_rejected_before_any_launch(flag):
    """a null g_x (or g_Z) under FASTEGNN_F_DETERMINISTIC or the FastRF wiring, a null g_x under the EGNN wiring (which has no Z), is
    FASTEGNN_E_INVALID; no kernel is launched (every other pointer of the descriptor is null: a launch could not get past its own argument
    checks either)"""
    from fastegnn_amd.model import SortedGraph, _new_layer, _stream
    m = _atomic_model(3, 1)
    inp = {k: v.cuda() for k, v in S._small(3).items()}
    m(**inp)   # builds the spec
    graph = SortedGraph(inp["edge_index"], 60)
    lib, st = K.lib(), _stream(inp["node_loc"].device)
    buf = torch.zeros(64 * 64, device="cuda")
    for null in ("g_x",) if flag == K.F_EGNN else ("g_x", "g_Z"):
        L = _new_layer(m._spec, 60, 2, graph)
        L.flags |= flag
        L.params = 1   # any non-null table: the checks come before anything is read
        L.wg_slab = buf.data_ptr()
        setattr(L, "g_Z" if null == "g_x" else "g_x", buf.data_ptr())
        with _switch(False):
            assert lib.fastegnn_layer_backward(C.byref(L), st) == -1, null   # FASTEGNN_E_INVALID
        assert b"not wanted" in lib.fastegnn_last_error(), lib.fastegnn_last_error()
    torch.cuda.synchronize()
