"""-m gpu: the last layer's node update (node_model, node_model_virtual) feeds h and Hv, which FastEGNN.forward does not return.  The model
leaves that layer's h_out / HvT_out and g_h_out / g_HvT_out null and the library then runs neither the update nor its adjoint
(include/fastegnn_hip.h).  FASTEGNN_KEEP_DEAD_NODE_UPDATE=1 (read per call) runs them as before: every comparison here is
skip ON against skip OFF in one process -- loc, vloc, every parameter gradient that is not None (the same set of Nones on both sides) and the
input gradients g_x, g_vel.

Both paths add the same terms; only sums that depend on the arrival order of atomics (pools, rank-1 gradient sums, the edge scatter) may
differ.  The bound on every tensor's max-norm relative difference is four times the largest such difference between two skip-OFF runs on
that shape, at least 1e-6, and never above 1e-5 (the project's output bar).

The virtual nodes of every input here start OFF the centroid of their graph, each channel somewhere else.  On the centroid (where the data
sets put them) the layer-0 gradients of coord_mlp_v_virtual are sum_n <Z - x_n, g_poolX> (...) with one g_poolX for all nodes of a graph:
a sum that cancels to almost nothing, whose fp32 value is the arrival order of its atomics -- measured on an MI355X, two skip-OFF runs of the
49 137-node frame differ by 1.1e-4 / 2.1e-4 of max|g| on its .0.weight / .2.weight there, and two runs of the parent commit's benchmark
by 2.7e-5 .. 9.5e-5 (profiles/last_layer_skip.txt): no comparison under a 1e-5 bar can look through that.  Off the centroid the sums have a value."""
import ctypes as C
import os

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from oracle import fastegnn_ref as R
from tests.helpers import rel_err

pytestmark = pytest.mark.gpu

SWITCH = "FASTEGNN_KEEP_DEAD_NODE_UPDATE"
FLOOR, CEIL = 1e-6, 1e-5


def _small(C_, seed=5):
    """two ragged graphs of 37 and 23 nodes (N = 60: no multiple of 16, the tile of nodes 32..47 straddles the graphs), ~300 random
    directed edges, node 3 isolated"""
    g = torch.Generator().manual_seed(seed)
    sizes, iso = [37, 23], 3
    rows, cols, batch, off = [], [], [], 0
    for b, n in enumerate(sizes):
        r = torch.randint(0, n, (n * 5,), generator=g) + off
        c = torch.randint(0, n, (n * 5,), generator=g) + off
        keep = (r != iso) & (c != iso)
        rows.append(r[keep]); cols.append(c[keep]); batch += [b] * n; off += n
    ei = torch.stack([torch.cat(rows), torch.cat(cols)])
    ei = ei[:, torch.randperm(ei.size(1), generator=g)]
    assert not (ei == iso).any() and 250 < ei.size(1) <= 300
    N, B = off, len(sizes)
    batch = torch.tensor(batch)
    loc = torch.randn(N, 3, generator=g) * 2.0
    cm = torch.zeros(B, 3).index_add_(0, batch, loc) / torch.bincount(batch, minlength=B).unsqueeze(1)
    vstart = cm.unsqueeze(-1).repeat(1, 1, C_) + 0.5 * torch.randn(B, 3, C_, generator=g)      # (off the centroid: module docstring)
    return dict(node_feat=torch.rand(N, 2, generator=g), node_loc=loc, node_vel=torch.randn(N, 3, generator=g) * 0.3,
                edge_index=ei, data_batch=batch, loc_mean=vstart,
                edge_attr=torch.rand(ei.size(1), 2, generator=g))


def _model(C_, L, attention=False, seed=7, **extra):
    cfg = R.Config(2, 0, 2, 64, C_, n_layers=L, gravity=[0, -1, 0], attention=attention)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, C_, device="cuda", n_layers=L, gravity=[0, -1, 0], attention=attention, **extra)
    m.load_state_dict(R.init_params(cfg, seed=seed, coord_gain=0.05), strict=True)
    return cfg, m.cuda()


def _loss(loc, vloc, tgt):
    return torch.nn.functional.mse_loss(loc, tgt) + 0.05 * vloc.pow(2).mean()


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


def _step(m, inp, tgt, keep):
    """one forward + backward -> {name: tensor or None}"""
    with _switch(keep):
        for p in m.parameters():
            p.grad = None
        kw = dict(inp, node_loc=inp["node_loc"].clone().requires_grad_(True), node_vel=inp["node_vel"].clone().requires_grad_(True))
        loc, vloc = m(**kw)
        # which path ran: the skipping forward gave the last layer neither npre nor poolV (null pointers in its descriptor), and its backward
        # will pass null g_h_out / g_HvT_out; with the switch every layer has them
        last = loc.grad_fn.saved[-1]
        assert loc.grad_fn.skip_last == (not keep) and ("npre" in last) == keep and ("poolV" in last) == keep, (keep, sorted(last))
        assert all("npre" in b and "poolV" in b for b in loc.grad_fn.saved[:-1])
        _loss(loc, vloc, tgt).backward()
        out = {"loc": loc.detach().clone(), "vloc": vloc.detach().clone(), "g_x": kw["node_loc"].grad.clone(),
               "g_vel": kw["node_vel"].grad.clone()}
        out.update({"grad." + n: (p.grad.clone() if p.grad is not None else None) for n, p in m.named_parameters()})
    return out


def _diffs(a, b):
    assert a.keys() == b.keys()
    assert {k for k, v in a.items() if v is None} == {k for k, v in b.items() if v is None}      # the same set of Nones
    return {k: rel_err(a[k], b[k]) for k in a if a[k] is not None}


def _baseline(m, inp, tgt):
    """skip OFF twice -> (the first run, the bound of the shape: four times the largest difference between the two, floor and ceiling)"""
    off0, off1 = _step(m, inp, tgt, True), _step(m, inp, tgt, True)
    noise = max(_diffs(off0, off1).values())
    return off0, noise, min(CEIL, max(4.0 * noise, FLOOR))


def _compare(tag, m, inp, tgt):
    """skip OFF twice (the shape's own run-to-run difference), then skip ON against skip OFF under four times that"""
    off0, worst_noise, bound = _baseline(m, inp, tgt)
    on = _step(m, inp, tgt, False)
    nones = sorted(k for k, v in on.items() if v is None)
    L = m.n_layers - 1
    assert nones == sorted(k for k in on if k.startswith((f"grad.gcl_{L}.node_mlp.", f"grad.gcl_{L}.node_mlp_virtual."))), nones
    d = _diffs(on, off0)
    for k in on:
        if on[k] is not None:
            assert torch.isfinite(on[k]).all(), k
    worst = max(d.values())
    print(f"last_layer_skip[{tag}]: off-vs-off max {worst_noise:.3e}, on-vs-off max {worst:.3e} "
          f"({max(d, key=d.get)}; tensors {len(d)}, None {len(nones)})")
    bad = {k: v for k, v in d.items() if v > bound}
    assert not bad, (bad, bound)
    return on


# Measured on an MI355X (largest difference over the tensors of a case: two skip-off runs | skip on against skip off): C3-L2 8.5e-7 | 8.5e-7,
# C3-L1 3.3e-6 | 2.9e-6, C3-L2-attention 1.1e-6 | 1.1e-6, C16-L2 1.6e-6 | 3.7e-6, C5-L2 7.1e-7 | 5.7e-7, C3-L2-bf16 3.4e-7 | 3.4e-7 -- mostly on
# gcl_0.coord_mlp_r.0.weight.  Not zero: the edge backward of graphs of <= 512 edges is order-independent, the LDS pools and rank-1 gradient
# sums of the virtual stage are not.  _compare prints the figures of a run.
@pytest.mark.parametrize("C_,L,att,bf16", [(3, 2, False, False), (3, 1, False, False), (3, 2, True, False), (16, 2, False, False),
                                          (5, 2, False, False), (3, 2, False, True)],
                         ids=["C3-L2", "C3-L1", "C3-L2-attention", "C16-L2", "C5-L2", "C3-L2-bf16"])
def test_small_ragged_batch_skip_on_matches_skip_off(C_, L, att, bf16):
    """tile-major backward, PAIR forward (fp32 operands) / one wave per tile (bf16 operands); L = 1: the only layer is the last one"""
    _, m = _model(C_, L, att, **({"mlp_dtype": torch.bfloat16} if bf16 else {}))
    inp = {k: v.cuda() for k, v in _small(C_).items()}
    _compare(f"C{C_}-L{L}-att{int(att)}-bf{int(bf16)}", m, inp, inp["node_loc"] + 0.5)


# the phased backward runs from 256 workgroups x 12 tiles (virt_cs_applies, csrc/virt_bwd.hip: grid = tiles / VBS_MIN_TILES >= 256):
# 3 072 tiles, the last of them partial
N_PHASED = 3071 * 16 + 1


def _radius_frame(N, C_, seed, radius=0.035):
    """N points uniform in a box of the density of 100 000 points in [0, 0.965]^3 (mean degree ~19 at r = 0.035), one graph;
    edge_attr = [dist, dist], target = loc + 20 vel; the virtual nodes around the centroid, not on it (module docstring)"""
    from fastegnn_amd.graphs import radius_graph
    g = torch.Generator().manual_seed(seed)
    loc = (torch.rand(N, 3, generator=g) * (0.965 * (N / 100000.0) ** (1.0 / 3.0))).cuda()
    vel = (torch.randn(N, 3, generator=g) * 0.003).cuda()
    ei, dist = radius_graph(loc, radius)
    vstart = loc.mean(0).view(1, 3, 1) + (0.1 * torch.randn(1, 3, C_, generator=g)).cuda()
    frame = dict(node_feat=torch.stack([vel.norm(dim=1), torch.ones(N, device="cuda")], 1), node_loc=loc, node_vel=vel, edge_index=ei,
                 data_batch=torch.zeros(N, dtype=torch.long, device="cuda"), loc_mean=vstart, edge_attr=torch.stack([dist, dist], 1))
    return frame, loc + 20.0 * vel


def test_phased_backward_skip_on_matches_skip_off():
    """virt_bwd_cs_kernel<.., NODE = false> at the smallest size where the phased form is the default: a radius graph, C = 16, L = 2.
    (With FASTEGNN_VIRT_CS=0 or FASTEGNN_VIRT_CS_MIN_GRID in the environment the kernel assertion at the end fails: this case is about that kernel.)"""
    torch.manual_seed(43)
    m = fastegnn_amd.FastEGNN(2, 0, 2, 64, 16, device="cuda", n_layers=2, gravity=[0, -1, 0])
    frame, tgt = _radius_frame(N_PHASED, 16, 43)
    lib = K.lib()
    lib.fastegnn_spin_timeouts(1)
    lib.fastegnn_profile_enable(1)
    K.profile_collect()
    try:
        # Measured on an MI355X: 4.8e-6 between two skip-off runs, 3.4e-6 skip on against skip off (both on gcl_0.coord_mlp_r.0.weight: the atomic
        # edge scatter arrives in another order every run) -- the bound in force is the ceiling, 1e-5
        _compare("phased", m, frame, tgt)
        torch.cuda.synchronize()
        prof = K.profile_collect()
    finally:
        lib.fastegnn_profile_enable(0)
    # three steps of two layers, every one of them through the phased kernel (no Gv stage)
    assert prof.get("virt_bwd_kernel", (0, 0))[1] == 6 and "virt_bwd_gv_kernel" not in prof, prof
    assert lib.fastegnn_spin_timeouts(1) == 0


def test_captured_graph_replays_match_eager():
    """the skipping step captured with torch.cuda.graph and replayed three times"""
    _, m = _model(3, 2)
    inp = {k: v.cuda() for k, v in _small(3).items()}
    tgt = inp["node_loc"] + 0.5
    _, _, bound = _baseline(m, inp, tgt)
    eager = _step(m, inp, tgt, False)
    with _switch(False):
        x, v = inp["node_loc"].clone().requires_grad_(True), inp["node_vel"].clone().requires_grad_(True)
        s = torch.cuda.Stream()
        s.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(s):
            for _ in range(2):   # warm-up on the side stream (allocator, lazy state)
                for p in m.parameters():
                    p.grad = None
                x.grad = v.grad = None
                loc, vloc = m(**dict(inp, node_loc=x, node_vel=v))
                _loss(loc, vloc, tgt).backward()
        torch.cuda.current_stream().wait_stream(s)
        for p in m.parameters():
            p.grad = None
        x.grad = v.grad = None
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph):
            loc, vloc = m(**dict(inp, node_loc=x, node_vel=v))
            _loss(loc, vloc, tgt).backward()
        for _ in range(3):
            graph.replay()
        torch.cuda.synchronize()
    got = {"loc": loc.detach(), "vloc": vloc.detach(), "g_x": x.grad, "g_vel": v.grad}
    got.update({"grad." + n: p.grad for n, p in m.named_parameters()})
    for k, v in got.items():
        assert (v is None) == (eager[k] is None), k
        if v is not None:
            assert rel_err(v, eager[k]) <= bound, (k, rel_err(v, eager[k]), bound)      # (the same bound as above: 4 x off-vs-off of this shape)


def test_small_shape_vs_oracle():
    """the skipping path (the default) against the CPU oracle with the suite's calibrated tolerances, unchanged"""
    from tests import test_gpu_properties as P
    assert os.environ.get(SWITCH, "0") in ("", "0")
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=2, gravity=[0, -1, 0])
    P._check_vs_oracle(cfg, _small(3), seed=7, case="last_layer_skip_small")


def test_layer_entry_points_with_all_four_pointers_match_the_switch():
    """fastegnn_layer_forward / fastegnn_layer_backward called directly with h_out, HvT_out, g_h_out, g_HvT_out non-null on every layer: what
    the model does with the switch set, within the shape's own run-to-run bound -- the library's non-null behaviour is what it was"""
    from fastegnn_amd.model import H, _PtrTable, _carve, _fill, _new_layer, _stream
    _, m = _model(3, 2)
    inp = {k: v.cuda() for k, v in _small(3).items()}
    tgt = inp["node_loc"] + 0.5
    ref, _, bound = _baseline(m, inp, tgt)
    spec, lib, dev = m._spec, K.lib(), inp["node_loc"].device
    st = _stream(dev)
    f32 = dict(dtype=torch.float32, device=dev)
    params = [p.detach() for p in m._plist]
    N, B, Cn = 60, 2, 3
    graph = m.sorted_graph(inp["edge_index"], N)
    assert bool(spec.flags & K.F_DETERMINISTIC) == (graph.cscptr is not None) or m._spec_det is not None
    if graph.cscptr is not None and not spec.flags & K.F_DETERMINISTIC:
        spec = m._spec_det
    batch32, gptr = torch.empty(N, dtype=torch.int32, device=dev), torch.empty(B + 1, dtype=torch.int32, device=dev)
    K.check(lib.fastegnn_build_batch(K.ptr(inp["data_batch"]), N, B, K.ptr(batch32), K.ptr(gptr), st), "build_batch")
    ea = graph.permute(inp["edge_attr"])
    h = torch.empty(N, H, **f32)
    K.check(lib.fastegnn_embed_forward(K.ptr(inp["node_feat"]), N, spec.nf, K.ptr(params[1]), K.ptr(params[2]), K.ptr(h), st), "embed")
    HvT = torch.empty(B, Cn, H, **f32)
    K.check(lib.fastegnn_virtual_init(K.ptr(params[0]), B, Cn, K.ptr(HvT), st), "virtual_init")
    x, Z, saved = inp["node_loc"], inp["loc_mean"].contiguous(), []
    nwp = (lib.fastegnn_wpack_floats(Cn) + 3) // 4 * 4
    for i in range(spec.n_layers):
        tab = _PtrTable([params[s] if s is not None else None for s in spec.layer_slots[i]])
        b = dict(h=h, x=x, Z=Z, HvT=HvT, wpack=torch.empty(nwp, **f32))
        b.update(_carve(dev, dict(P=(N, H), QX=(N, K.QX_LD), A=(N, H), svel=(N,), sgrav=(N,), xsum=(B, 4), Bc=(B, Cn, H), aggm=(N, H),
                                  npre=(N, H), poolV=(B, Cn, H), aggx=(N, 3), poolX=(B, 3, Cn), h_out=(N, H), x_out=(N, 3),
                                  Z_out=(B, 3, Cn), HvT_out=(B, Cn, H))))
        Lf = _new_layer(spec, N, B, graph)
        _fill(Lf, batch=batch32, gptr=gptr, vel=inp["node_vel"], params=tab.addr(), ea_sorted=ea, **b)
        Lf.QX_src = b["QX"].data_ptr()
        assert Lf.h_out and Lf.HvT_out
        K.check(lib.fastegnn_layer_forward(C.byref(Lf), st), "layer_forward")
        saved.append((b, tab))
        h, x, Z, HvT = b["h_out"], b["x_out"], b["Z_out"], b["HvT_out"]
    # (not bit for bit: the pools and rank-1 sums of two runs of ONE path already differ in the order of their atomics -- the shape's bound)
    assert rel_err(x, ref["loc"]) <= bound and rel_err(Z, ref["vloc"]) <= bound
    loc, vloc = x.clone().requires_grad_(True), Z.clone().requires_grad_(True)
    _loss(loc, vloc, tgt).backward()
    grads = [torch.zeros_like(p) for p in params]
    g_h, g_x, g_Z, g_HvT = torch.zeros(N, H, **f32), loc.grad.contiguous(), vloc.grad.contiguous(), torch.zeros(B, Cn, H, **f32)
    g_vel, E = torch.zeros(N, 3, **f32), graph.E
    scratch = _carve(dev, dict(
        g_poolV=(B, Cn, H), g_poolX=(B, 3, Cn), g_Bc=(B, Cn, H), g_Zp=(B, 3, Cn), g_xbar=(B, 4), g_A=(N, H), g_P=(N, H), g_aggm=(N, H),
        g_aggx=(N, 3), g_svel=(N,), g_sgrav=(N,), g_QXe=(max(E, 1) if spec.flags & K.F_DETERMINISTIC else 1, K.QX_LD),
        g_QX_src=(N, K.QX_LD), g_xrow=(N, 3), wg_edge=(lib.fastegnn_wg_edge_floats(E),),
        wg_virt=(lib.fastegnn_wg_virt_floats_for(N, Cn, spec.flags),), wg_node=(lib.fastegnn_wg_node_floats(N, B, Cn),),
        wg_slab=(lib.fastegnn_wg_slab_floats(),)))
    for i in reversed(range(spec.n_layers)):
        b, tab = saved[i]
        b = {k: v for k, v in b.items() if k not in ("aggx", "poolX", "h_out", "x_out", "Z_out", "HvT_out")}
        gtab = _PtrTable([grads[s] if s is not None else None for s in spec.layer_slots[i]])
        out = dict(g_h=torch.empty(N, H, **f32), g_x=torch.empty(N, 3, **f32), g_Z=torch.empty(B, 3, Cn, **f32),
                   g_HvT=torch.empty(B, Cn, H, **f32))
        Lb = _new_layer(spec, N, B, graph)
        _fill(Lb, batch=batch32, gptr=gptr, vel=inp["node_vel"], params=tab.addr(), grads=gtab.addr(), g_h_out=g_h, g_x_out=g_x,
              g_Z_out=g_Z, g_HvT_out=g_HvT, g_vel=g_vel, ea_sorted=ea, **b, **out, **scratch)
        Lb.QX_src = b["QX"].data_ptr()
        Lb.g_QX = scratch["g_QX_src"].data_ptr()
        assert Lb.g_h_out and Lb.g_HvT_out
        K.check(lib.fastegnn_layer_backward(C.byref(Lb), st), "layer_backward")
        g_h, g_x, g_Z, g_HvT = out["g_h"], out["g_x"], out["g_Z"], out["g_HvT"]
    torch.cuda.synchronize()
    assert rel_err(g_x, ref["g_x"]) <= bound and rel_err(g_vel, ref["g_vel"]) <= bound
    for name, g in zip(spec.names, grads):
        if name in ("virtual_node_feat", "embedding_in.weight", "embedding_in.bias"):
            continue   # (their gradients come from the embedding / virtual-init adjoints behind the layers)
        r = ref["grad." + name]
        if r is None:      # the last layer's node update: the library wrote its exact zeros, the model hands out None
            assert not g.any(), name
        else:
            assert rel_err(g, r) <= bound, (name, rel_err(g, r), bound)


def test_one_null_one_non_null_is_rejected_before_any_launch():
    """a plain argument check of the two entry points: exactly one pointer of a pair null is FASTEGNN_E_INVALID (no kernel is launched)"""
    from fastegnn_amd.model import SortedGraph, _new_layer, _stream
    _, m = _model(3, 1)
    inp = {k: v.cuda() for k, v in _small(3).items()}
    m(**inp)   # builds the spec
    graph = SortedGraph(inp["edge_index"], 60)
    lib, st = K.lib(), _stream(inp["node_loc"].device)
    buf = torch.zeros(64 * 64, device="cuda")
    for stage, field in ((lib.fastegnn_virt_forward, "HvT_out"), (lib.fastegnn_graph_post_forward, "h_out"),
                         (lib.fastegnn_virt_backward, "g_HvT_out"), (lib.fastegnn_graph_post_backward, "g_h_out")):
        L = _new_layer(m._spec, 60, 2, graph)
        L.params = 1   # any non-null table: the pointer-pair check comes before anything is read
        setattr(L, field, buf.data_ptr())
        assert stage(C.byref(L), st) == -1, field   # FASTEGNN_E_INVALID
        assert "null" in lib.fastegnn_last_error().decode()
