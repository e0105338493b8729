"""-m gpu: forward-only execution of the fused models (fastegnn_amd.model._forward_only, fastegnn_amd.egnn._egnn_forward_only; DESIGN.md
section 16): a forward that can have no backward runs the same C-ABI calls on ONE reused set of stage buffers.

* memory: the peak of a no_grad forward does not grow by a stage set per layer any more;
* same function: its outputs hold the outputs rule of tests/helpers.py against the fp32 oracle (1e-5 of the fp32 reference, the
  displacement by grad_check through the fp64 oracle), as the grad-mode forward is held;
* what a call returned is never overwritten by a later call; the autograd path is what it was; the path is capturable."""
import copy

import pytest
import torch

import fastegnn_amd
from fastegnn_amd.model import _padded, inference_plan
from fastegnn_amd.train import mse_mmd_eval
from oracle import fastegnn_ref as R
from tests import test_gpu_properties as P
from tests.gpu_util import model_from_golden
from tests.helpers import OUT_TOL, Golden, check_parity, grad_check, rel_err
from tests.test_gpu_evaluate import _sample

pytestmark = pytest.mark.gpu


# ----------------------------------------------------------------------------------------------------------------------
# 1. memory
# ----------------------------------------------------------------------------------------------------------------------
N_MEM, DEG_MEM, C_MEM = 20000, 6, 3


def _mem_inputs():
    g = torch.Generator().manual_seed(1)
    N, E = N_MEM, N_MEM * DEG_MEM
    loc = torch.rand(N, 3, generator=g) * 3.0
    return dict(loc=loc.cuda(), vel=(torch.randn(N, 3, generator=g) * 0.01).cuda(), feat=torch.rand(N, 2, generator=g).cuda(),
                ei=torch.randint(0, N, (2, E), generator=g).cuda(), ea=torch.rand(E, 2, generator=g).cuda(),
                batch=torch.zeros(N, dtype=torch.long, device="cuda"), mean=loc.mean(0).view(1, 3, 1).repeat(1, 1, C_MEM).cuda())


def _peak_of_a_no_grad_forward(kind, L, d):
    """max_memory_allocated() delta of one no_grad forward, the graph prebuilt and one warm-up call first"""
    torch.manual_seed(2)
    if kind == "egnn":
        m = fastegnn_amd.EGNN(n_layers=L, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
        call = lambda: m(x=d["loc"], h=d["feat"], edge_index=d["ei"], edge_fea=d["ea"], v=d["vel"])   # noqa: E731 (its graph: cached by the warm-up)
    else:
        cls = fastegnn_amd.FastEGNN if kind == "fastegnn" else fastegnn_amd.FastRF
        m = cls(2, 0, 2, 64, C_MEM, device="cuda", n_layers=L)
        graph = m.sorted_graph(d["ei"], N_MEM)
        call = lambda: m(d["feat"], d["loc"], d["vel"], graph, d["batch"], d["mean"], edge_attr=d["ea"])   # noqa: E731
    with torch.no_grad():
        out = call()
        del out
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()
        out = call()
        torch.cuda.synchronize()
        peak = torch.cuda.max_memory_allocated() - base
        del out
    return peak


@pytest.mark.parametrize("kind", ["fastegnn", "fastrf", "egnn"])
def test_peak_memory_of_a_no_grad_forward_does_not_grow_with_the_layers(kind):
    """FastEGNN(2, 0, 2, 64, C = 3) on 20 000 nodes and 120 000 edges, one graph, fp32: four layers may take at most half a stage set
    more than one layer.  (A forward that keeps a set per layer takes three sets more.)
    Measured on an MI355X, four layers minus one layer, against the bound of 12.55 MiB (12.51 for EGNN): FastEGNN 10.00 MiB (the second
    ping-pong set and the npre / poolV a single dead layer does not have), FastRF 0.00, EGNN 6.08; the forward that kept a set per layer
    (the commit before this mode): 95.83 / 95.83 / 95.81 MiB."""
    B, C = (1, 0) if kind == "egnn" else (1, C_MEM)
    shapes, _ = inference_plan(N_MEM, B, C, 4, kind)
    stage_bytes = 4 * sum(_padded(s) for k, s in shapes.items() if "@" not in k)
    assert stage_bytes > 4 * 320 * N_MEM
    d = _mem_inputs()
    p1, p4 = _peak_of_a_no_grad_forward(kind, 1, d), _peak_of_a_no_grad_forward(kind, 4, d)
    print(f"no_grad peak [{kind}]: 1 layer {p1 / 2 ** 20:.2f} MiB, 4 layers {p4 / 2 ** 20:.2f} MiB, one stage set {stage_bytes / 2 ** 20:.2f} MiB")
    assert p4 - p1 <= 0.5 * stage_bytes, (p1, p4, stage_bytes)


# ----------------------------------------------------------------------------------------------------------------------
# 2. the same function
# ----------------------------------------------------------------------------------------------------------------------
SIZES = [300, 141, 77, 40]      # the last graph has no edges
FLAG_GOLDENS = ["ragged3_allflags", "ragged3_attention", "ragged3_default_init", "ragged3_gravity", "ragged3_nodeattr",
                "ragged3_noresidual", "ragged3_normalize", "ragged3_tanh"]
_INPUTS = {}


def _ragged_inputs(cfg, seed=11):
    """three ragged graphs with random endpoints (self loops, repeated edges, isolated nodes) and a fourth one without edges; made once
    per (feature widths, C) and never changed"""
    key = (cfg.node_feat_nf, cfg.node_attr_nf, cfg.edge_attr_nf, cfg.virtual_channels, seed)
    if key not in _INPUTS:
        inp = P._batch(SIZES, 2, cfg.virtual_channels, seed=seed, nf=cfg.node_feat_nf, ea=cfg.edge_attr_nf)
        first = sum(SIZES[:3])
        keep = inp["edge_index"][0] < first
        inp["edge_index"], inp["edge_attr"] = inp["edge_index"][:, keep].contiguous(), inp["edge_attr"][keep].contiguous()
        ei = inp["edge_index"]
        assert (ei[0] == ei[1]).any() and ei.size(1) > torch.unique(ei, dim=1).size(1)              # self loops, repeated edges
        touched = torch.zeros(sum(SIZES), dtype=torch.bool)
        touched[ei.reshape(-1)] = True
        assert (~touched[:first]).any() and not touched[first:].any()                                   # isolated nodes; the empty graph
        if cfg.node_attr_nf:
            inp["node_attr"] = torch.rand(sum(SIZES), cfg.node_attr_nf, generator=torch.Generator().manual_seed(seed + 1))
        _INPUTS[key] = inp
    return _INPUTS[key]


def _check_outputs(case, cfg, p, inp, loc, vloc):
    """the outputs rule: 1e-5 of the fp32 oracle, and the displacement through the fp64 oracle (tests/helpers.py)"""
    l32, v32 = R.forward(p, cfg, **inp)
    p64 = {k: v.double() for k, v in p.items()}
    l64, _ = R.forward(p64, cfg, **{k: (v.double() if v.is_floating_point() else v) for k, v in inp.items()})
    bad = []
    for name, got, ref in (("loc", loc, l32), ("vloc", vloc, v32)):
        assert torch.isfinite(got).all(), (case, name)
        if rel_err(got, ref) >= OUT_TOL:
            bad.append(f"{name} {rel_err(got, ref):.2e}")
    x0 = inp["node_loc"].double()
    grad_check(case, "displacement", loc.detach().cpu().double() - x0, l32.double() - x0, l64 - x0, bad)
    assert not bad, (case, bad)


@pytest.mark.parametrize("L", [1, 2, 3, 4])
@pytest.mark.parametrize("name", FLAG_GOLDENS)
def test_no_grad_outputs_hold_the_outputs_rule(name, L):
    """both ping-pong parities and the single layer, under every flag set of the ragged3_* goldens"""
    cfg = copy.copy(Golden(name).cfg)
    cfg.n_layers = L
    p, m = P._models(cfg, seed=20 + L)
    inp = _ragged_inputs(cfg)
    with torch.no_grad():
        p = {k: v.detach() for k, v in p.items()}
        loc, vloc = m(**{k: v.cuda() for k, v in inp.items()})
        assert loc.grad_fn is None and not loc.requires_grad
        _check_outputs(f"no_grad_{name}_L{L}", cfg, p, inp, loc, vloc)


def test_frozen_parameters_take_the_forward_only_path_in_grad_mode_too():
    cfg = copy.copy(Golden("ragged3_gravity").cfg)
    cfg.n_layers = 3
    p, m = P._models(cfg, seed=23)
    inp = _ragged_inputs(cfg)
    for q in m.parameters():
        q.requires_grad_(False)
    loc, vloc = m(**{k: v.cuda() for k, v in inp.items()})
    assert loc.grad_fn is None
    with torch.no_grad():
        _check_outputs("frozen", cfg, {k: v.detach() for k, v in p.items()}, inp, loc, vloc)


@pytest.mark.parametrize("name", ["ragged3_allflags", "c16_two_graphs", "nbody5_cfg1"])
def test_fastegnn_goldens_under_no_grad(name):
    g = Golden(name)
    m = model_from_golden(g, device="cuda")
    kw, _, _ = g.model_kwargs(device="cuda")
    with torch.no_grad():
        loc, vloc = m(**kw)
    msgs = check_parity(g, loc, vloc)
    assert not msgs, msgs


def test_fastrf_golden_under_no_grad():
    g = Golden("fastrf_allflags")
    m = model_from_golden(g, cls=fastegnn_amd.FastRF)
    kw, _, _ = g.model_kwargs(device="cuda")
    with torch.no_grad():
        loc, vloc = m(**kw)
    assert rel_err(loc, g.out["loc"]) < OUT_TOL and rel_err(vloc, g.out["vloc"]) < OUT_TOL      # tests/test_gpu_fastrf.py's rule


def test_egnn_golden_under_no_grad():
    from tests.test_egnn_oracle_cpu import load_egnn
    from tests.test_gpu_egnn import _egnn_of_golden
    g = load_egnn("egnn_with_v")
    m = _egnn_of_golden(g)
    m.load_state_dict(g["p"], strict=True)
    m = m.cuda()
    i = {k: v.cuda() for k, v in g["in"].items()}
    with torch.no_grad():
        out = m(x=i["x"], h=i["h"], edge_index=i["edge_index"], edge_fea=i["edge_fea"], v=i["v"])
    assert len(out) == 3 and out[1] is i["v"]
    assert rel_err(out[0], g["out"]["x"]) < 1e-5 and rel_err(out[-1], g["out"]["h"]) < 2e-5           # tests/test_gpu_egnn.py's rule


# ----------------------------------------------------------------------------------------------------------------------
# 3. / 4. results are never overwritten; the autograd path is what it was
# ----------------------------------------------------------------------------------------------------------------------
def _two_input_sets(cfg):
    """two batches of the ragged shape with different edge lists"""
    return _ragged_inputs(cfg, seed=11), _ragged_inputs(cfg, seed=12)


def _same_graph_other_values(a, seed):
    """the batch `a` with every floating-point input drawn again (what a captured graph is replayed on: same shapes, same edge list)"""
    g = torch.Generator().manual_seed(seed)
    b = dict(a)
    b["node_loc"] = a["node_loc"] + 0.2 * torch.randn(a["node_loc"].shape, generator=g)
    b["node_vel"] = torch.randn(a["node_vel"].shape, generator=g) * 0.3
    b["node_feat"] = torch.rand(a["node_feat"].shape, generator=g)
    b["edge_attr"] = torch.rand(a["edge_attr"].shape, generator=g)
    b["loc_mean"] = a["loc_mean"] + 0.1 * torch.randn(a["loc_mean"].shape, generator=g)
    return b


def test_a_later_call_never_overwrites_a_result():
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=3, gravity=[0, -1, 0])
    p, m = P._models(cfg, seed=31)
    a, b = _two_input_sets(cfg)
    da, db = {k: v.cuda() for k, v in a.items()}, {k: v.cuda() for k, v in b.items()}
    with torch.no_grad():
        out_a = m(**da)
        keep = [t.clone() for t in out_a]
    tgt = b["node_loc"] + 0.5
    loc, vloc, got = P._run_module(m, b, tgt)                       # a full training forward and backward in between
    with torch.no_grad():
        out_b = m(**db)
        out_b2 = m(**db)
    torch.cuda.synchronize()
    assert all(torch.equal(t, k) for t, k in zip(out_a, keep))      # bitwise
    ptrs = {t.data_ptr() for t in (*out_a, *out_b, *out_b2)}
    assert len(ptrs) == 6                                           # six live results, six allocations
    P._compare_vs_oracle("inference_interleaved", cfg, p, b, tgt, loc, vloc, got)     # the existing gradient rule
    with torch.no_grad():
        _check_outputs("inference_after_training", cfg, {k: v.detach() for k, v in p.items()}, b, *out_b)


def test_grad_path_saves_what_it_saved_and_survives_an_interleaved_no_grad_call():
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=3, gravity=[0, -1, 0])
    p, m = P._models(cfg, seed=32)
    a, b = _two_input_sets(cfg)
    kw = {k: v.cuda() for k, v in b.items()}
    tgt = b["node_loc"] + 0.5
    loc, vloc = m(**kw)
    saved = loc.grad_fn.saved
    assert len(saved) == cfg.n_layers
    full = {"h", "x", "Z", "HvT", "wpack", "P", "QX", "A", "svel", "sgrav", "xsum", "Bc", "aggm", "npre", "poolV"}
    assert all(set(s) == full for s in saved[:-1]) and set(saved[-1]) == full - {"npre", "poolV"}       # (the last layer's dead node update)
    assert len({s["P"].data_ptr() for s in saved}) == cfg.n_layers                                    # a stage set per layer, as before
    with torch.no_grad():
        other = m(**{k: v.cuda() for k, v in a.items()})                                              # ... between forward and backward
    P._loss(loc, vloc, tgt.cuda()).backward()
    got = {k: (v.grad.cpu() if v.grad is not None else torch.zeros_like(v).cpu()) for k, v in m.named_parameters()}
    P._compare_vs_oracle("inference_grad_path", cfg, p, b, tgt, loc, vloc, got)
    with torch.no_grad():
        _check_outputs("inference_between", cfg, {k: v.detach() for k, v in p.items()}, a, *other)


# ----------------------------------------------------------------------------------------------------------------------
# 5. capture
# ----------------------------------------------------------------------------------------------------------------------
def test_captured_no_grad_forward_and_eval_loss_replay():
    """the recipe of the repository's replay tests: an eager pass, the capture on a side stream, replays on two input sets copied into static
    tensors.  The outputs of a replay hold the outputs rule.  The accumulator is compared bit for bit with the eager sum over the outputs the
    replays produced: the loss kernel is order-fixed, while two forwards of one input are not the same bits (the virtual pools are summed with
    atomics in arrival order), so an eager forward is compared by the outputs rule and its sum by the loss bound."""
    from tests.test_gpu_evaluate import _bounds
    cfg = R.Config(2, 0, 2, 64, 3, n_layers=3, gravity=[0, -1, 0])
    p, m = P._models(cfg, seed=41)
    a = _ragged_inputs(cfg)
    b = _same_graph_other_values(a, 42)
    sigma, weight, S = 1.5, 0.7, 9
    samp, cnt = _sample(SIZES, S, torch.Generator().manual_seed(5))
    samp, cnt = samp.cuda(), cnt.cuda()
    static = {k: v.cuda().clone() for k, v in a.items()}
    tgts = [(s["node_loc"] + 0.3 * s["node_vel"]).cuda() for s in (a, b)]
    tgt = tgts[0].clone()
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    floats = [k for k, v in a.items() if v.is_floating_point()]

    def load(src, t):
        for k in floats:
            static[k].copy_(src[k])
        tgt.copy_(t)

    def step():
        loc, vloc = m(**static)
        mse_mmd_eval(loc, vloc, tgt, acc, sigma, weight, samp, cnt)
        return loc, vloc

    with torch.no_grad():
        eager = []
        for src, t in zip((a, b), tgts):                            # the eager pass (also loads the kernels, allocates the guard's words)
            load(src, t)
            eager.append(tuple(o.clone() for o in step()))
        eager_acc = acc.clone()
        stream = torch.cuda.Stream()
        stream.wait_stream(torch.cuda.current_stream())
        with torch.cuda.stream(stream):
            step()                                                  # warm-up on the side stream (allocator)
        torch.cuda.current_stream().wait_stream(stream)
        graph = torch.cuda.CUDAGraph()
        with torch.cuda.graph(graph, stream=stream):
            loc, vloc = step()
        acc.zero_()
        outs = []
        for src, t in zip((a, b), tgts):
            load(src, t)
            graph.replay()
            outs.append((loc.clone(), vloc.clone()))
        torch.cuda.synchronize()
        replay_acc = acc.clone()
        # the eager sum over the replays' own outputs: bit for bit
        acc.zero_()
        for (l, v), t in zip(outs, tgts):
            mse_mmd_eval(l, v, t, acc, sigma, weight, samp, cnt)
        assert torch.equal(acc, replay_acc), (acc.tolist(), replay_acc.tolist())
        assert float(replay_acc[2]) == 8.0
        # against the fully eager pass: outputs rule, and the sum within the loss bound of its two batches
        pd = {k: v.detach() for k, v in p.items()}
        tol = [0.0]
        for i, (src, t) in enumerate(zip((a, b), tgts)):
            _check_outputs(f"inference_replay{i}", cfg, pd, src, *outs[i])
            assert rel_err(outs[i][0], eager[i][0]) < OUT_TOL and rel_err(outs[i][1], eager[i][1]) < OUT_TOL
            _, _, b_mse, _ = _bounds(eager[i][0].cpu(), eager[i][1].cpu(), t.cpu(), samp.cpu(), cnt.cpu(), sigma, weight)
            e = 2 * OUT_TOL * float(eager[i][0].abs().max())       # two forwards inside the output bar move a mean of squares by 2 e sqrt(mse) + e^2
            mse = float((eager[i][0] - t).pow(2).mean())
            tol[0] += b_mse + len(SIZES) * (2 * e * mse ** 0.5 + e * e)
        print(f"replayed acc {replay_acc.tolist()} eager {eager_acc.tolist()}")
        assert abs(float(replay_acc[0] - eager_acc[0])) <= tol[0] and float(replay_acc[2]) == float(eager_acc[2])
