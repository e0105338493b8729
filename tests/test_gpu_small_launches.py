"""The small launches around the fused kernels: the per-graph stages in their four-wave / LDS-staged forms, the ordered
per-graph coordinate sums (block partials + a fixed-order combine, stand-alone and folded into graph_pre_fwd_kernel), the
zeroing of the virtual stage's accumulators folded into the launch in front of it, and the streamed embedding gradient.

Per-graph stages.  Every stage of stage_harness.GRAPH_LEVEL through stage_harness (make_case / run_stage / reference / compare:
the harness's own rule against the fp64 stage oracle, guard bands around every buffer).  Graph size lists and what each is for:
  (1,)                      one row, one tile, one node: every clamp of the tile loads
  (0, 3, 0, 2, 0)           empty graphs first, between and last: node ranges of length zero in the combine
  (64, 1, 63)               a graph that ends on a lane boundary of a block, a one-node graph, a block shared by three graphs
  (65,)                     one node past a wave of the block walk
  (100, 157)                a graph boundary inside the first block (256 nodes), one node past it
  (1,) * 257 + (0,) * 43    more graphs than a block has nodes; with C = 16 it is 4 800 rows = 300 tiles, more than the 256
                            workgroups of graph_post_*: the tile loop takes a second step
  (5000,)                   head-less graph: 19 whole blocks and a tail
  (16 * 4096 + 1,)          256 whole blocks and a tail: every thread of the combine holds a partial and the tree above them has
                            its lane, wave and workgroup level
Every list runs at C = 3 with and without `residual`; C = 1, 16, 17, 64 run at (100, 157) and (64, 1, 63), also with and
without.  The per-graph stages do not see N except through xsum, so the widths are not repeated at the large lists (the fp64
reference of graph_post_* at 65 537 nodes x 64 channels would take minutes).  graph_xsum does not see C: C = 3 only.
One case in bf16 operand mode and one on the generic-activation (_act) build.

xsum.  Two runs give the same bits; the staged entry point and the form folded into fastegnn_layer_forward (node ranges from
gptr, and searched in `batch` when the layer carries no gptr) give the same bits; the fp64 agreement is the stage test above.
The folded layer call also has to zero poolV / poolX (forward) and g_Bc / g_Zp (backward) itself: the buffers start from the
harness's NaN pattern, so a missing fill shows as a non-finite output.

Embedding gradient (wgrad_small_kernel).  The shapes of test_gpu_small_kernels.py::test_embed_forward_and_backward plus
N = 70 001 (274 rows per workgroup: three steps of 128 rows, the last one ragged) under that test's bound (grad_check).  Two runs
are bitwise equal in dW / db where ONE workgroup runs (N <= 256: a single atomic per element onto the start value); with more
workgroups the partials are the same bits in every run and only the order of the <= 256 float atomics that add them differs --
that order is not fixed, so only the single-workgroup sizes are compared bit for bit."""
import pytest
import torch

from fastegnn_amd import _lib as K
from tests import stage_harness as S
from tests.helpers import grad_check
from tests.stage_harness import BandedPool
from tests.test_gpu_small_kernels import _put, _rnd, _st

pytestmark = pytest.mark.gpu
H = S.H

BIG = (16 * 4096 + 1,)
SIZES = [(1,), (0, 3, 0, 2, 0), (64, 1, 63), (65,), (100, 157), (1,) * 257 + (0,) * 43, (5000,), BIG]
WIDTH_SIZES = [(100, 157), (64, 1, 63)]
_RUNNERS = {}


def _runner(act=False):
    if act not in _RUNNERS:
        _RUNNERS[act] = S.HipRunner(act, False)
    return _RUNNERS[act]


def _sid(sizes):
    return "x".join(map(str, sizes)) if len(sizes) < 8 else f"{len(sizes)}graphs_{sum(sizes)}nodes"


def _stage_params():
    out = []
    for stage in S.GRAPH_LEVEL:
        keys = [(sz, 3, fl) for sz in SIZES for fl in ((), ("noresidual",))]
        if stage != "graph_xsum":
            keys += [(sz, C, fl) for C in (1, 16, 17, 64) for sz in WIDTH_SIZES for fl in ((), ("noresidual",))]
            keys += [((1,) * 257 + (0,) * 43, 16, ())]
        keys += [((100, 157), 3, ("bf16",))]
        for sz, C, fl in keys:
            out.append(pytest.param(stage, sz, C, fl, False, id=f"{stage}-{_sid(sz)}-c{C}-{'+'.join(fl) or 'residual'}"))
        out.append(pytest.param(stage, (100, 157), 3, (), True, id=f"{stage}-100x157-c3-residual-act"))
    return out


@pytest.mark.parametrize("stage,sizes,C,flags,act", _stage_params())
def test_graph_stage_against_fp64(stage, sizes, C, flags, act):
    rn = _runner(act)
    key = (sizes, C, 0, 0, flags, "none")
    case = S.make_case(*key)
    ref32, truth = S.reference(stage, key + (0,), (), rn.pq_scale(case))
    bad = []
    for batch in ((False, True) if stage in S.BACKWARD else (False,)):
        got = S.run_stage(rn, stage, case, batch=batch)
        bad += S.compare(S.case_name(stage, case, f"batch={int(batch)}", rn.name), got, ref32, truth, sizes=case.sizes, bf16=case.cfg.bf16)
    assert not bad, bad


@pytest.mark.parametrize("sizes", SIZES, ids=_sid)
def test_xsum_two_runs_same_bits(sizes):
    rn = _runner()
    case = S.make_case(sizes, 3, 0, 0, (), "none")
    a = S.run_stage(rn, "graph_xsum", case)["xsum"]
    b = S.run_stage(rn, "graph_xsum", case)["xsum"]
    assert torch.equal(a, b)
    assert torch.equal(a[:, 3], torch.tensor(sizes, dtype=torch.float64))


def _layer_buffers(rn, case, with_gptr):
    """every buffer of one whole-layer call on the case's operands; outputs and scratch start from the NaN pattern"""
    be, t, N, B, C = rn.backend(case), case.t, case.N, case.B, case.C
    b = {k: rn.put(t[k]) for k in ("h", "x", "vel", "Z", "HvT")}
    b["batch"] = rn.put_int(case.batch.to(torch.int32))
    if with_gptr:
        ptr = torch.zeros(B + 1, dtype=torch.int64)
        ptr[1:] = torch.cumsum(torch.tensor(case.sizes), 0)
        b["gptr"] = rn.put_int(ptr.to(torch.int32))
    b["wpack"] = rn.scratch((be.wpack_floats(C) + 3) // 4 * 4)
    for k, s in dict(P=(N, H), QX=(N, S.QX_LD), A=(N, H), svel=(N,), sgrav=(N,), xsum=(B, 4), Bc=(B, C, H), aggm=(N, H), aggx=(N, 3),
                     npre=(N, H), poolV=(B, C, H), poolX=(B, 3, C), h_out=(N, H), x_out=(N, 3), Z_out=(B, 3, C),
                     HvT_out=(B, C, H)).items():
        b[k] = rn.new(*s)
    b["QX_src"] = b["QX"]
    return b


@pytest.mark.parametrize("with_gptr", [True, False], ids=["gptr", "searched"])
@pytest.mark.parametrize("sizes", [(0, 3, 0, 2, 0), (64, 1, 63), (100, 157), (5000,), BIG], ids=_sid)
def test_folded_layer_call(sizes, with_gptr):
    """fastegnn_layer_forward / _backward on buffers that start from NaN: xsum and Bc are the staged entry points' to the bit,
    the pools and the virtual stage's accumulators were zeroed (every output finite), no guard band written"""
    rn = _runner()
    case = S.make_case(sizes, 3, 0, 0, (), "none")
    staged = S.run_stage(rn, "graph_xsum", case)["xsum"]
    staged_Bc = S.run_stage(rn, "graph_pre_forward", case)["Bc"]
    be, N, B, C = rn.backend(case), case.N, case.B, case.C
    rn.reset()
    spec = rn.spec(case, False)
    params = [rn.put(w) if w is not None else None for w in case.params]
    graph = be.build_graph(rn.put_int(case.edge_index), N, case.n_src, case.row_begin, csc=False)
    b = _layer_buffers(rn, case, with_gptr)
    be.stage("layer_forward", spec, N, B, graph, b, params)
    rn.check_bands("layer_forward")
    assert torch.equal(rn.get(b["xsum"]), staged)
    assert torch.equal(rn.get(b["Bc"]), staged_Bc)
    for k in ("poolV", "poolX", "h_out", "x_out", "Z_out", "HvT_out"):
        assert bool(torch.isfinite(b[k]).all()), k
    grads = [rn.put(g0) if g0 is not None else None for g0 in case.grads0]
    for k in ("g_h_out", "g_x_out", "g_Z_out", "g_HvT_out"):
        b[k] = rn.put(case.t[k])
    for k, s in dict(g_h=(N, H), g_x=(N, 3), g_Z=(B, 3, C), g_HvT=(B, C, H), g_vel=(N, 3), g_poolV=(B, C, H), g_poolX=(B, 3, C),
                     g_Bc=(B, C, H), g_Zp=(B, 3, C), g_xbar=(B * 4,), g_A=(N, H), g_P=(N, H), g_aggm=(N, H), g_aggx=(N, 3), g_svel=(N,),
                     g_sgrav=(N,), g_QXe=(1, S.QX_LD), g_QX_src=(N, S.QX_LD), g_xrow=(N, 3)).items():
        b[k] = rn.new(*s)
    b["g_vel"].zero_()                                   # (+= by the ABI)
    b["g_QX"] = b["g_QX_src"]
    b["wg_edge"] = rn.scratch(be.wg_edge_floats(0))
    b["wg_virt"] = rn.scratch(be.wg_virt_floats(N, C, spec.flags))
    b["wg_node"] = rn.scratch(be.wg_node_floats(N, B, C))
    b["wg_slab"] = rn.scratch(be.wg_slab_floats())
    for k in ("aggx", "poolX", "h_out", "x_out", "Z_out", "HvT_out"):
        b.pop(k)
    be.stage("layer_backward", spec, N, B, graph, b, params, grads)
    rn.check_bands("layer_backward")
    for k in ("g_Bc", "g_Zp", "g_h", "g_x", "g_Z", "g_HvT"):
        assert bool(torch.isfinite(b[k]).all()), k
    for g in grads:
        assert g is None or bool(torch.isfinite(g).all())
    rn.reset()


# ---------------------------------------------------------------- embedding_in
@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000, 70001])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 6, 7, 8])
def test_embed_forward_and_streamed_gradient(nf, N):
    g = torch.Generator().manual_seed(nf * 10007 + N)
    x, W, b, g_h = _rnd(g, N, nf), _rnd(g, H, nf), _rnd(g, H), _rnd(g, N, H)
    gW0, gb0 = _rnd(g, H, nf), _rnd(g, H)
    lib, pool, case, bad = K.lib(), BandedPool(), f"small_launches:embed:nf{nf}:N{N}", []
    d = {k: _put(pool, v) for k, v in dict(x=x, W=W, b=b, g_h=g_h).items()}
    h = pool._alloc(N * H).view(N, H)
    K.check(lib.fastegnn_embed_forward(K.ptr(d["x"]), N, nf, K.ptr(d["W"]), K.ptr(d["b"]), K.ptr(h), _st()), "fastegnn_embed_forward")
    grad_check(case, "h", h.cpu(), x @ W.T + b, x.double() @ W.double().T + b.double(), bad)
    truth = dict(gW=g_h.double().T @ x.double(), gb=g_h.double().sum(0))
    ref32 = dict(gW=g_h.T @ x, gb=g_h.sum(0))
    runs = []
    for _ in range(2):
        gW, gb = _put(pool, gW0), _put(pool, gb0)                      # both accumulate (+=): they start from a random value
        K.check(lib.fastegnn_embed_backward(K.ptr(d["x"]), K.ptr(d["g_h"]), N, nf, K.ptr(d["W"]), K.ptr(gW), K.ptr(gb), K.ptr(None), _st()),
                "fastegnn_embed_backward")
        grad_check(case, "gW", gW.cpu().double() - gW0.double(), ref32["gW"], truth["gW"], bad)
        grad_check(case, "gb", gb.cpu().double() - gb0.double(), ref32["gb"], truth["gb"], bad)
        runs.append((gW.cpu(), gb.cpu()))
    pool.check_bands(case)
    assert bool(torch.isfinite(h).all()) and not bad, bad
    if N <= 256:                                                       # one workgroup: one atomic per element
        assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])
