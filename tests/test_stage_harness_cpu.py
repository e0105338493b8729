"""CPU: the two things the stage-level GPU tests (tests/test_gpu_stages.py) rest on.

1. The references are the reference.  The stages of tests/cpu_stage_backend.py, chained in fp64 into one layer, equal
   autograd through the op-for-op oracle (oracle.fastegnn_ref.layer_forward, which holds the reference's detach of the norm
   under normalize=True) on the same operands to 1e-10 -- outputs, input gradients (edge_attr and node_attr included) and
   every parameter gradient, for every flag set of the stage matrix.
2. The comparison has teeth.  An fp32 CpuOracleBackend with ONE wrong term, pushed through stage_harness.compare in the
   place of a HIP result, is reported on at least one case of the matrix -- for each of the eleven mutants below -- and the
   unmutated fp32 backend on none.

The same two things for the sibling wirings (FastRF, the EGNN baseline) and the seven non-SiLU activation kinds of
tests/test_gpu_stage_wirings.py: chain tests against oracle.fastrf_ref / oracle.egnn_ref / oracle.fastegnn_ref with Config.act, eleven
more mutants, and the seeds at which the kinked activations run (no pre-activation within 1e-5 of 0)."""
import pytest
import torch

from oracle import factored as F
from oracle import fastegnn_ref as R
from tests import stage_harness as S
from tests.cpu_stage_backend import CpuOracleBackend
from tests.helpers import rel_err

H = 64
FLAG_SETS = sorted({k[4] for k in S.MATRIX if "bf16" not in k[4]})      # (the bf16 mirror has no autograd counterpart: its rounding
#                                                                          of operands is not what oracle.fastegnn_ref computes)


def _chain(case):
    """one layer through the eleven stage statements in fp64: outputs, input gradients, parameter gradients"""
    dt = torch.float64
    cfg, t, N, B, C = case.cfg, case.t, case.N, case.B, case.C
    be = CpuOracleBackend(None, 1, cfg, dtype=dt)
    graph = be.build_graph(case.edge_index, N, N, 0)
    z = lambda *s: torch.zeros(*s, dtype=dt)      # noqa: E731
    b = dict(batch=case.batch, h=t["h"], x=t["x"], vel=t["vel"], Z=t["Z"], HvT=t["HvT"], node_attr=t.get("node_attr"),
             ea_sorted=graph.permute(t.get("ea")),
             P=z(N, H), QX=z(N, 68), A=z(N, H), svel=z(N), sgrav=z(N), xsum=z(B, 4), Bc=z(B, C, H), aggm=z(N, H), aggx=z(N, 3),
             poolV=z(B, C, H), poolX=z(B, 3, C), h_out=z(N, H), x_out=z(N, 3), Z_out=z(B, 3, C), HvT_out=z(B, C, H))
    b["QX_src"] = b["QX"]
    for st in S.FORWARD:
        be.stage(st, None, N, B, graph, b, case.params)
    grads = [torch.zeros_like(w) if w is not None else None for w in case.params]
    b.update(g_h_out=t["g_h_out"], g_x_out=t["g_x_out"], g_Z_out=t["g_Z_out"], g_HvT_out=t["g_HvT_out"],
             g_h=z(N, H), g_x=z(N, 3), g_Z=z(B, 3, C), g_HvT=z(B, C, H), g_vel=z(N, 3), g_poolV=z(B, C, H), g_poolX=z(B, 3, C),
             g_Bc=z(B, C, H), g_Zp=z(B, 3, C), g_xbar=z(B, 4), g_A=z(N, H), g_P=z(N, H), g_aggm=z(N, H), g_aggx=z(N, 3),
             g_svel=z(N), g_sgrav=z(N), g_QX_src=z(N, 68), g_xrow=z(N, 3),
             g_ea_sorted=z(max(graph.E, 1), cfg.edge_attr_nf) if cfg.edge_attr_nf else None,
             g_node_attr=z(N, cfg.node_attr_nf) if cfg.node_attr_nf else None)
    b["g_QX"] = b["g_QX_src"]
    for st in ("graph_post_backward", "virt_backward", "graph_pre_backward", "edge_backward", "edge_col_reduce", "node_pre_backward"):
        be.stage(st, None, N, B, graph, b, case.params, grads)
    return b, grads, graph


@pytest.mark.parametrize("flags", FLAG_SETS, ids=lambda f: "+".join(f) or "plain")
@pytest.mark.parametrize("kind", ["random", "one_col"])
def test_chained_fp64_stages_equal_autograd_of_the_oracle(flags, kind):
    from fastegnn_amd._lib import PARAM_SLOTS
    case = S.make_case(S.S_RAGGED, 3, 2, 1, flags, kind)
    cfg, t = case.cfg, case.t
    b, grads, graph = _chain(case)
    p = {f"gcl_0.{s}": w.clone().requires_grad_(True) for s, w in zip(PARAM_SLOTS, case.params) if w is not None}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("h", "x", "vel", "Z", "node_attr", "ea")}
    Hv = t["HvT"].transpose(1, 2).clone().requires_grad_(True)
    grav = torch.tensor(list(cfg.gravity), dtype=torch.float64) if cfg.gravity is not None else None
    h1, x1, Hv1, Z1 = R.layer_forward(p, "gcl_0", cfg, leaf["h"], case.edge_index, leaf["x"], leaf["vel"], leaf["Z"], Hv, case.batch,
                                      edge_attr=leaf["ea"], node_attr=leaf["node_attr"], gravity=grav)
    ((h1 * t["g_h_out"]).sum() + (x1 * t["g_x_out"]).sum() + (Z1 * t["g_Z_out"]).sum()
     + (Hv1.transpose(1, 2) * t["g_HvT_out"]).sum()).backward()
    pairs = [("h_out", b["h_out"], h1), ("x_out", b["x_out"], x1), ("Z_out", b["Z_out"], Z1), ("HvT_out", b["HvT_out"], Hv1.transpose(1, 2)),
             ("g_h", b["g_h"], leaf["h"].grad), ("g_x", b["g_x"], leaf["x"].grad), ("g_vel", b["g_vel"], leaf["vel"].grad),
             ("g_Z", b["g_Z"], leaf["Z"].grad), ("g_HvT", b["g_HvT"], Hv.grad.transpose(1, 2)),
             ("g_node_attr", b["g_node_attr"], leaf["node_attr"].grad),
             ("g_ea_sorted", b["g_ea_sorted"][:graph.E], leaf["ea"].grad[graph.perm])]
    for s, g in zip(PARAM_SLOTS, grads):
        if g is not None:
            pairs.append(("grad." + s, g, p["gcl_0." + s].grad))
    bad = [(k, rel_err(a, r.detach())) for k, a, r in pairs if rel_err(a, r.detach()) > 1e-10]
    assert not bad, bad
    assert all(float(r.detach().abs().max()) > 0 for _, _, r in pairs)          # every compared quantity is live


def test_autograd_through_the_factored_edge_stage_is_not_the_reference_under_normalize():
    """why the hand-written backward stages are the truth: autograd through F.edge_fwd differentiates the norm the reference
    detaches -- g_P agrees with the hand-written F.edge_bwd, the coordinate gradients do not (and do without normalize)"""
    for flags, differs in ((("normalize",), True), ((), False)):
        case = S.make_case(S.S_RAGGED, 3, 2, 0, flags, "random")
        cfg, t = case.cfg, case.t
        be = CpuOracleBackend(None, 1, cfg, dtype=torch.float64)
        w, _ = be._w(case.params)
        csr = be.build_graph(case.edge_index, case.N, case.N, 0).csr_as(torch.float64)
        ea = t["ea"][csr.perm]
        P, Q, x = (v.clone().requires_grad_(True) for v in (t["P"], t["QX_src"][:, :H], t["x"]))
        aggm, aggx = F.edge_fwd(w, cfg, csr, P, Q, x, ea)
        ((aggm * t["g_aggm"]).sum() + (aggx * t["g_aggx"]).sum()).backward()
        G = be._G([torch.zeros_like(v) if v is not None else None for v in case.params], case.params)
        g_P, g_Q, g_x = F.edge_bwd(w, cfg, G, "L", csr, t["P"], t["QX_src"][:, :H], t["x"], ea, t["g_aggm"], t["g_aggx"])
        assert rel_err(g_P, P.grad) < 1e-12 and rel_err(g_Q, Q.grad) < 1e-12
        assert (rel_err(g_x, x.grad) > 1e-3) == differs


# --------------------------------------------------------------------------
# mutants: CpuOracleBackend with one wrong term each
# --------------------------------------------------------------------------
class _Mutant(CpuOracleBackend):
    stage_name = None          # the stage the error lives in
    variant = ()               # a run_stage variant the error needs to show (e.g. accum)

    def _stage(self, name, N, B, graph, t, params, grads, flags):
        if name != self.stage_name:
            return super()._stage(name, N, B, graph, t, params, grads, flags)
        return self.wrong(name, N, B, graph, t, params, grads, flags)


class XbarDropped(_Mutant):                                     # 1
    stage_name = "node_pre_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, dict(t, g_xbar=torch.zeros_like(t["g_xbar"])), params, grads, flags)


class XbarOfOneNodeGraphs(_Mutant):                             # 2
    """(read literally -- "not divided by n_b for graphs of one node" -- the error is the identity, n_b being 1 there.  The nearest
    error that touches only the slice of a one-node graph: its centroid gradient is divided by the count of the graph BEFORE it,
    an off-by-one in the graph index of the division)"""
    stage_name = "graph_pre_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        cnt = t["xsum"][:, 3].clamp(min=1)
        for b in range(1, B):
            if cnt[b] == 1:
                t["g_xbar"][b, :3] *= cnt[b] / cnt[b - 1]


class ColSideSignFlipped(_Mutant):                              # 3
    stage_name = "edge_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        before = t["g_QX_src"][:, H:H + 3].clone()
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        from fastegnn_amd._lib import F_GQX_ACCUM
        base = before if flags & F_GQX_ACCUM else torch.zeros_like(before)
        t["g_QX_src"][:, H:H + 3] = base - (t["g_QX_src"][:, H:H + 3] - base)


class InvDegMissingOnAggx(_Mutant):                             # 4
    stage_name = "edge_forward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        if self.cfg.coords_agg == "mean":
            t["aggx"] *= graph.deg.clamp(min=1).to(t["aggx"].dtype).unsqueeze(1)


class GqxZeroedDespiteAccum(_Mutant):                           # 5
    stage_name, variant = "edge_backward", (("accum", True),)

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, 0)


class GvelWritten(_Mutant):                                     # 6
    stage_name = "node_pre_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        t["g_vel"].copy_(t["svel"].unsqueeze(1) * t["g_x_out"])


class GZpOmitted(_Mutant):                                      # 7
    stage_name = "graph_pre_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, dict(t, g_Zp=torch.zeros_like(t["g_Zp"])), params, grads, flags)


class ResidualDroppedFromGHvT(_Mutant):                         # 8
    stage_name = "graph_post_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        if self.cfg.residual and t.get("g_HvT_out") is not None:
            t["g_HvT"] -= t["g_HvT_out"]


class PoolVMissesLastPartialTile(_Mutant):                      # 9
    stage_name = "virt_forward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        rows = torch.arange(N // 16 * 16, N)
        rows = rows[t["batch"][rows] == B - 1]
        if t.get("poolV") is None or rows.numel() == 0:
            return
        cfg, dt = self.cfg, t["x"].dtype
        w, _ = self._w(params)
        grav = torch.tensor(list(cfg.gravity), dtype=dt) if cfg.gravity is not None else None
        sub = lambda k: t[k][rows] if t.get(k) is not None else None      # noqa: E731
        _, _, poolV, _ = F.virt_fwd(w, cfg, sub("h"), sub("A"), t["Bc"], sub("x"), sub("vel"), t["Z"], t["batch"][rows], sub("aggm"),
                                    sub("aggx"), sub("svel"), sub("sgrav") if grav is not None else None, grav, sub("node_attr"))
        t["poolV"][B - 1] -= poolV[B - 1]


class WeightGradientWritten(_Mutant):                           # 10
    stage_name = "node_pre_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        grads[1].zero_()                                        # edge_mlp.0.bias: '=' in the place of '+='
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)


class GsvelScaled(_Mutant):                                     # 11: sets the sensitivity
    stage_name = "virt_backward"

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        t["g_svel"] *= 1.0 + 1e-4


MUTANTS = [XbarDropped, XbarOfOneNodeGraphs, ColSideSignFlipped, InvDegMissingOnAggx, GqxZeroedDespiteAccum, GvelWritten, GZpOmitted,
           ResidualDroppedFromGHvT, PoolVMissesLastPartialTile, WeightGradientWritten, GsvelScaled]


def _cases(stage, need=()):
    for key, variant in S.stage_cases(stage):
        if sum(key[0]) > 100 or "bf16" in key[4]:      # (the small shapes decide; the bf16 rule is a hundred times wider by design)
            continue
        v = tuple(p for p in variant if p[0] != "det")
        if all(p in v for p in need):
            yield key, v


@pytest.mark.parametrize("mutant", MUTANTS, ids=lambda m: m.__name__)
def test_every_mutant_is_reported_and_the_clean_backend_is_not(mutant):
    reported = []
    for key, v in _cases(mutant.stage_name, mutant.variant):
        case = S.make_case(*key)
        ref32, truth = S.reference(mutant.stage_name, key + (0,), v, 1.0)
        name = S.case_name(mutant.stage_name, case, S.variant_id(key, v), "cpu32")
        assert not S.compare(name, ref32, ref32, truth, sizes=case.sizes)
        got = S.run_stage(S.CpuRunner(torch.float32, backend_cls=mutant), mutant.stage_name, case, **dict(v))
        bad = S.compare(name + "-" + mutant.__name__, got, ref32, truth, sizes=case.sizes)
        if bad:
            reported.append((S.variant_id(key, v), bad[:3]))
    assert reported, f"{mutant.__name__}: not reported on any case of the matrix"


def test_two_launch_form_catches_a_second_launch_that_zeroes_the_table():
    """mutant 5 again, in the form the sharded caller uses: two launches over disjoint row ranges, the second with GQX_ACCUM"""
    key = next(k for k in S.EDGE_ONLY if k[5] == "two_launch")
    case = S.make_case(*key)
    ref32, truth = S.reference("edge_backward", key + (0,), (), 1.0)
    got = S.run_stage(S.CpuRunner(torch.float32, backend_cls=GqxZeroedDespiteAccum), "edge_backward", case)
    assert not S.compare("stage:edge_backward:two:cpu32", ref32, ref32, truth, sizes=case.sizes)
    assert any(m.startswith("g_QX_src") for m in S.compare("stage:edge_backward:two:mutant", got, ref32, truth, sizes=case.sizes))


def test_unwritten_output_and_missing_output_are_reported():
    key = S.MATRIX[1]
    case = S.make_case(*key)
    ref32, truth = S.reference("edge_forward", key + (0,), (), 1.0)
    got = {k: v.clone() for k, v in ref32.items()}
    got["aggx"][7, 1] = float("nan")
    assert any("not finite" in m for m in S.compare("stage:x", got, ref32, truth))
    del got["aggm"]
    assert any("missing" in m for m in S.compare("stage:x", got, ref32, truth))


# --------------------------------------------------------------------------
# the sibling wirings and the activation kinds (tests/test_gpu_stage_wirings.py)
# --------------------------------------------------------------------------
def _chain_wired(case, params=None):
    """_chain for any wiring: the stages the wiring has, in the order fastegnn_layer_forward / _backward run them"""
    dt = torch.float64
    cfg, t, N, B, C = case.cfg, case.t, case.N, case.B, case.C
    egnn = case.wiring[0] == "egnn"
    params = case.params if params is None else params
    be = CpuOracleBackend(None, 1, cfg, dtype=dt)
    graph = be.build_graph(case.edge_index, N, N, 0)
    z = lambda *s: torch.zeros(*s, dtype=dt)      # noqa: E731
    b = dict(batch=case.batch, h=t["h"], x=t["x"], vel=t["vel"], Z=t["Z"], HvT=t["HvT"], node_attr=t.get("node_attr"),
             ea_sorted=graph.permute(t.get("ea")),
             P=z(N, H), QX=z(N, 68), A=z(N, H), svel=z(N), sgrav=z(N), xsum=z(B, 4), Bc=z(B, C, H), aggm=z(N, H), aggx=z(N, 3),
             poolV=z(B, C, H), poolX=z(B, 3, C), h_out=z(N, H), x_out=z(N, 3), Z_out=z(B, 3, C), HvT_out=z(B, C, H))
    b["QX_src"] = b["QX"]
    for st in (("node_pre_forward", "edge_forward", "virt_forward") if egnn else S.FORWARD):
        be.stage(st, None, N, B, graph, b, params)
    grads = [torch.zeros_like(w) if w is not None else None for w in params]
    b.update(g_h_out=t["g_h_out"], g_x_out=t["g_x_out"], g_Z_out=t["g_Z_out"], g_HvT_out=t["g_HvT_out"],
             g_h=z(N, H), g_x=z(N, 3), g_Z=z(B, 3, C), g_HvT=z(B, C, H), g_vel=z(N, 3), g_poolV=z(B, C, H), g_poolX=z(B, 3, C),
             g_Bc=z(B, C, H), g_Zp=z(B, 3, C), g_xbar=z(B, 4), g_A=z(N, H), g_P=z(N, H), g_aggm=z(N, H), g_aggx=z(N, 3),
             g_svel=z(N), g_sgrav=z(N), g_QX_src=z(N, 68), g_xrow=z(N, 3),
             g_ea_sorted=z(max(graph.E, 1), cfg.edge_attr_nf) if cfg.edge_attr_nf else None,
             g_node_attr=z(N, cfg.node_attr_nf) if cfg.node_attr_nf else None)
    b["g_QX"] = b["g_QX_src"]
    back = ("virt_backward", "edge_backward", "edge_col_reduce", "node_pre_backward")
    for st in (back if egnn else ("graph_post_backward", "virt_backward", "graph_pre_backward") + back[1:]):
        be.stage(st, None, N, B, graph, b, params, grads)
    return b, grads, graph


def _assert_pairs(pairs):
    bad = [(k, rel_err(a, r.detach())) for k, a, r in pairs if rel_err(a, r.detach()) > 1e-10]
    assert not bad, bad
    dead = [k for k, _, r in pairs if not float(r.detach().abs().max()) > 0]
    assert not dead, f"compared against nothing: {dead}"


def _fast_pairs(case, layer_forward, node_attr):
    """autograd through an op-for-op FastEGNN / FastRF layer against the chained stages"""
    from fastegnn_amd._lib import PARAM_SLOTS
    cfg, t = case.cfg, case.t
    b, grads, graph = _chain_wired(case)
    p = {f"gcl_0.{s}": w.clone().requires_grad_(True) for s, w in zip(PARAM_SLOTS, case.params) if w is not None}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("h", "x", "vel", "Z", "ea") + (("node_attr",) if node_attr else ())}
    Hv = t["HvT"].transpose(1, 2).clone().requires_grad_(True)
    grav = torch.tensor(list(cfg.gravity), dtype=torch.float64) if cfg.gravity is not None else None
    kw = dict(node_attr=leaf["node_attr"]) if node_attr else {}
    h1, x1, Hv1, Z1 = layer_forward(p, "gcl_0", cfg, leaf["h"], case.edge_index, leaf["x"], leaf["vel"], leaf["Z"], Hv, case.batch,
                                    edge_attr=leaf["ea"], gravity=grav, **kw)
    ((h1 * t["g_h_out"]).sum() + (x1 * t["g_x_out"]).sum() + (Z1 * t["g_Z_out"]).sum()
     + (Hv1.transpose(1, 2) * t["g_HvT_out"]).sum()).backward()
    pairs = [("h_out", b["h_out"], h1), ("x_out", b["x_out"], x1), ("Z_out", b["Z_out"], Z1), ("HvT_out", b["HvT_out"], Hv1.transpose(1, 2)),
             ("g_h", b["g_h"], leaf["h"].grad), ("g_x", b["g_x"], leaf["x"].grad), ("g_vel", b["g_vel"], leaf["vel"].grad),
             ("g_Z", b["g_Z"], leaf["Z"].grad), ("g_HvT", b["g_HvT"], Hv.grad.transpose(1, 2)),
             ("g_ea_sorted", b["g_ea_sorted"][:graph.E], leaf["ea"].grad[graph.perm])]
    if node_attr:
        pairs.append(("g_node_attr", b["g_node_attr"], leaf["node_attr"].grad))
    for s, g in zip(PARAM_SLOTS, grads):
        if g is not None:
            pairs.append(("grad." + s, g, p["gcl_0." + s].grad))
    return pairs


@pytest.mark.parametrize("kind", ["random", "one_col"])
@pytest.mark.parametrize("flags", [S.ALL_FLAGS, ()], ids=["allflags", "plain"])
def test_chained_fp64_rf_stages_equal_autograd_of_the_fastrf_oracle(flags, kind):
    from oracle import fastrf_ref as RF
    case = S.make_case(S.S_RAGGED, 3, 2, 0, flags, kind, 0, S.RF, S.SILU)
    pairs = _fast_pairs(case, RF.layer_forward, node_attr=False)
    assert torch.equal(dict((k, a) for k, a, _ in pairs)["h_out"], case.t["h"])        # the node features pass through
    _assert_pairs(pairs)


@pytest.mark.parametrize("kind", ["random", "one_col"])
@pytest.mark.parametrize("act", S.KINDS, ids=lambda a: a[0])
def test_chained_fp64_stages_equal_autograd_of_the_oracle_for_every_activation(act, kind):
    case = S.make_case(S.S_RAGGED, 3, 2, 1, S.ALL_FLAGS, kind, 0, S.FASTEGNN_WIRING, act)
    _assert_pairs(_fast_pairs(case, R.layer_forward, node_attr=True))


@pytest.mark.parametrize("kind", ["random", "one_col"])
@pytest.mark.parametrize("with_v,norm", [(True, False), (False, False), (True, True), (False, True)], ids=["v", "nov", "v+norm", "nov+norm"])
def test_chained_fp64_egnn_stages_equal_autograd_of_the_egnn_oracle(with_v, norm, kind):
    """N = 17, one graph.  The coordinate head is scaled until the clamp is engaged on some components and not on others; under norm the
    case carries its eight sub-epsilon and four coincident pairs (stage_harness._egnn_operand_edges)."""
    from fastegnn_amd._lib import PARAM_SLOTS
    from fastegnn_amd.egnn import _SLOT_OF
    from oracle import egnn_ref as E
    case = S.make_case((17,), 0, 7, 0, (), kind, 0, ("egnn", with_v, norm), S.SILU)
    t = case.t
    slot = PARAM_SLOTS.index("coord_mlp_r.2.weight")
    params = [w * 3000.0 if i == slot else w for i, w in enumerate(case.params)]
    b, grads, graph = _chain_wired(case, params)
    over = b["aggx"].abs() > F.CLAMP
    assert bool(over.any()) and not bool(over.all()), "the clamp is not engaged on some components and off on others"
    if norm:
        d = t["x"][graph.row] - t["x"][graph.col]
        r = (d * d).sum(1)
        assert int(((r > 0) & (r < F.NORM_EPS)).sum()) >= 4 and int((r == 0).sum()) >= 2 and bool((r >= F.NORM_EPS).any())
    p = {f"layers.0.{_SLOT_OF[s]}": w.clone().requires_grad_(True) for s, w in zip(PARAM_SLOTS, params) if w is not None}
    leaf = {k: t[k].clone().requires_grad_(True) for k in ("h", "x", "ea") + (("vel",) if with_v else ())}
    x1, h1 = E.layer_forward(p, "layers.0", leaf["x"], leaf["h"], case.edge_index, leaf["ea"], leaf.get("vel"), norm=norm)
    ((h1 * t["g_h_out"]).sum() + (x1 * t["g_x_out"]).sum()).backward()
    pairs = [("h_out", b["h_out"], h1), ("x_out", b["x_out"], x1), ("g_h", b["g_h"], leaf["h"].grad), ("g_x", b["g_x"], leaf["x"].grad),
             ("g_ea_sorted", b["g_ea_sorted"][:graph.E], leaf["ea"].grad[graph.perm])]
    if with_v:
        pairs.append(("g_vel", b["g_vel"], leaf["vel"].grad))
    else:
        assert not bool(b["g_vel"].any()) and not bool(b["svel"].any())       # no head: a zero scale, nothing reaches the velocity
    for s, g in zip(PARAM_SLOTS, grads):
        if g is not None:
            pairs.append(("grad." + s, g, p[f"layers.0.{_SLOT_OF[s]}"].grad))
    _assert_pairs(pairs)


def test_egnn_clamp_gate_includes_its_boundary_as_torch_clamp_does():
    """the virt stage of the EGNN wiring on the case's own aggx draw (x 100, eight components exactly +-100) against autograd through
    torch.clamp: the gradient passes on the boundary and inside, and nowhere else"""
    case = S.make_case((65,), 0, 0, 0, (), "deg32_33", 0, ("egnn", True, False), S.SILU)
    t = case.t
    a = t["aggx"]
    assert int((a.abs() == 100.0).sum()) == 8 and 0.2 < float((a.abs() > 100.0).double().mean()) < 0.45
    aggx = a.clone().requires_grad_(True)
    (torch.clamp(aggx, min=-100, max=100) * t["g_x_out"]).sum().backward()
    got = S.run_stage(S.CpuRunner(torch.float64), "virt_backward", case)["g_aggx"]
    assert torch.equal(got, aggx.grad)
    assert bool((got[a.abs() == 100.0] != 0).all()) and not bool(got[a.abs() > 100.0].any())


@pytest.mark.parametrize("n,ea,kind", [(65, 7, "random"), (65, 7, "subrange"), (681, 2, "hub"), (681, 2, "one_col")])
def test_egnn_norm_cases_carry_their_sub_epsilon_and_coincident_pairs(n, ea, kind):
    """eight connected pairs with 0 < r < 1e-12 (1..4 ulps apart in every component, far from the epsilon) and four with r = 0"""
    case = S.make_case((n,), 0, ea, 0, (), kind, 0, ("egnn", True, True), S.SILU)
    xs = case.t["QX_src"][:, H:H + 3]
    assert torch.equal(xs[case.row_begin:case.row_begin + case.N], case.t["x"]) and torch.equal(xs, xs.float().double())
    d = xs[case.edge_index[0]] - xs[case.edge_index[1]]
    r = (d * d).sum(1)
    sub = (r > 0) & (r < F.NORM_EPS)
    pairs = lambda m: len({frozenset((int(a), int(b))) for a, b in case.edge_index[:, m].T})      # noqa: E731
    assert pairs(sub) >= 8 and pairs(r == 0) >= 4        # (more where two moved nodes of one anchor are connected as well)
    assert float(r[sub].max()) < 2e-13 and bool((d[sub] != 0).all())


@pytest.mark.parametrize("kind", S.KINKED)
def test_committed_kink_seeds_keep_every_preactivation_away_from_zero(kind):
    """relu, leaky_relu and elu (alpha != 1) have a derivative that jumps at 0: at every committed (kind, shape, stage) seed the fp64
    reference evaluates no pre-activation with |z| < 1e-5, so no rounding of a correct kernel can take the other branch"""
    act = next(a for a in S.KINDS if a[0] == kind)
    for (k, i, stage), seed in S.KINK_SEEDS.items():
        if k == kind:
            m = S.min_abs_preactivation(stage, S.ACT_SHAPES[i] + (seed, S.FASTEGNN_WIRING, act))
            assert m >= S.KINK_BAND, (kind, i, stage, seed, m)
    assert {(k, i, st) for k in S.KINKED for i in range(len(S.ACT_SHAPES)) for st in S.STAGES} == set(S.KINK_SEEDS)
    assert act[0] != "elu" or act[1] != 1.0


# --------------------------------------------------------------------------
# mutants of the branches the new cases reach: one wrong term each
# --------------------------------------------------------------------------
class _patched:
    """oracle.factored with one module attribute replaced for the duration of a stage call"""

    def __init__(self, name, value):
        self.name, self.value = name, value

    def __enter__(self):
        self.prev = getattr(F, self.name)
        setattr(F, self.name, self.value)

    def __exit__(self, *a):
        setattr(F, self.name, self.prev)


_EGNN = lambda n, ea, kind, v=True, norm=False: ((n,), 0, ea, 0, (), kind, 0, ("egnn", v, norm), S.SILU)      # noqa: E731
_RF_KEYS = [k + (0, S.RF, S.SILU) for k in S.RF_MATRIX if sum(k[0]) <= 100 and "bf16" not in k[4]]
_ACT = lambda kind: [sh + (0, S.FASTEGNN_WIRING, next(a for a in S.KINDS if a[0] == kind)) for sh in S.ACT_SHAPES]      # noqa: E731


class ClampGradientPassedOutside(_Mutant):                      # 1
    stage_name, keys = "virt_backward", [_EGNN(17, 0, "none"), _EGNN(65, 0, "deg32_33")]

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        t["g_aggx"].copy_(t["g_x_out"])


class ClampBoundaryTreatedAsOutside(_Mutant):                   # 2
    stage_name, keys = "virt_backward", [_EGNN(17, 0, "none"), _EGNN(65, 0, "deg32_33")]

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        t["g_aggx"][t["aggx"].abs() >= 100.0] = 0.0


class RadialColumnAt2H(_Mutant):                                # 3
    stage_name, keys = "edge_forward", [_EGNN(17, 7, "random"), _EGNN(65, 0, "deg32_33")]

    def _w(self, params):
        w, p = CpuOracleBackend._w(self, params)
        w.w_r = p["L.edge_mlp.0.weight"][:, 2 * H]
        return w, p

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)


class CoordHeadBiasGradientDropped(_Mutant):                    # 4
    stage_name, keys = "edge_backward", [_EGNN(17, 7, "random"), _EGNN(65, 0, "deg32_33")]

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        from fastegnn_amd._lib import PARAM_SLOTS
        g = grads[PARAM_SLOTS.index("coord_mlp_r.2.bias")]
        before = g.clone()
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        g.copy_(before)


class NormDerivativeAboveEpsilon(_Mutant):                      # 5
    stage_name, keys = "edge_backward", [_EGNN(17, 7, "random", norm=True), _EGNN(65, 7, "random", norm=True)]

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        real = F._edge_recompute

        def recompute(*a, **k):
            out = real(*a, **k)
            out["drf"] = torch.full_like(out["r"], 1.0 / F.NORM_EPS)
            return out
        with _patched("_edge_recompute", recompute):
            CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)


class RfVelocityHeadFedH(_Mutant):                              # 6
    stage_name, keys = "node_pre_forward", _RF_KEYS

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        vel = torch.zeros_like(t["vel"])
        vel[:, 0] = t["h"][:, 0]                                # the head's scalar input taken from h (its first feature) in the place of |vel|
        CpuOracleBackend._stage(self, name, N, B, graph, dict(t, vel=vel), params, grads, flags)


class RfNodeModelAdjointRun(_Mutant):                           # 7
    """FastRF has no node_mlp (its slots are null: no kernel can write them), so "node_mlp's gradient moved" shows on the operand side: the
    adjoint of a node model that does not exist hands g_h_out on to the pooled messages"""
    stage_name, keys = "virt_backward", _RF_KEYS

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        t["g_aggm"].copy_(t["g_h_out"])


class SiluDerivativeForGelu(_Mutant):                           # 8
    stage_name, keys = "edge_backward", _ACT("gelu")

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        real = F.act_pair
        with _patched("act_pair", lambda cfg: (real(cfg)[0], F.dsilu)):
            CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)


class SigmoidOfZeroLeaksIntoBiasGradient(_Mutant):              # 9
    """act(0) = 0.5 once per padding row of the last 16-row tile of edges, into edge_mlp.2.bias's gradient"""
    stage_name, keys = "edge_backward", _ACT("sigmoid")

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        from fastegnn_amd._lib import PARAM_SLOTS
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        grads[PARAM_SLOTS.index("edge_mlp.2.bias")] += 0.5 * (-graph.E % 16)


class SigmoidOfZeroLeaksIntoPoolV(_Mutant):                     # 10
    """the same leak into poolV of every graph whose node count is no multiple of 16"""
    stage_name, keys = "virt_forward", _ACT("sigmoid")

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)
        cnt = torch.bincount(t["batch"], minlength=B)
        t["poolV"] += (0.5 * (-cnt % 16)).to(t["poolV"].dtype).view(-1, 1, 1)


WIRING_MUTANTS = [ClampGradientPassedOutside, ClampBoundaryTreatedAsOutside, RadialColumnAt2H, CoordHeadBiasGradientDropped,
                  NormDerivativeAboveEpsilon, RfVelocityHeadFedH, RfNodeModelAdjointRun, SiluDerivativeForGelu,
                  SigmoidOfZeroLeaksIntoBiasGradient, SigmoidOfZeroLeaksIntoPoolV]


@pytest.mark.parametrize("mutant", WIRING_MUTANTS, ids=lambda m: m.__name__)
def test_every_wiring_mutant_is_reported_and_the_clean_backend_is_not(mutant):
    reported = []
    for key in mutant.keys:
        case = S.make_case(*key)
        ref32, truth = S.reference(mutant.stage_name, key, (), 1.0)
        name = S.case_name(mutant.stage_name, case, S.wiring_case_id(key, ()), "cpu32")
        assert not S.compare(name, ref32, ref32, truth, sizes=case.sizes)
        got = S.run_stage(S.CpuRunner(torch.float32, backend_cls=mutant), mutant.stage_name, case)
        bad = S.compare(name + "-" + mutant.__name__, got, ref32, truth, sizes=case.sizes)
        if bad:
            reported.append((S.wiring_case_id(key, ()), bad[:3]))
    assert reported, f"{mutant.__name__}: not reported on any of its cases"


def test_softplus_without_its_threshold_branch_is_reported():
    """mutant 11.  One row of P is scaled until a pre-activation passes beta z = 20, where torch.nn.Softplus is the identity.  log(1 + exp(beta z))
    without that branch is the same number to 1e-15 until exp overflows (fp32: beta z > 88.7) and infinite beyond: the row is scaled past that."""
    import dataclasses
    key = S.ACT_SHAPES[0] + (0, S.FASTEGNN_WIRING, ("softplus", 1.7))
    base = S.make_case(*key)
    t = dict(base.t)
    t["P"] = base.t["P"].clone()
    row = int(base.edge_index[0, 0])
    t["P"][row] *= 40.0
    case = dataclasses.replace(base, t=t)
    seen = {}

    def no_threshold(cfg):
        q = cfg.act_param

        def act(z):
            seen["max"] = max(seen.get("max", 0.0), float(z.max()) * q)
            return torch.log1p(torch.exp(z * q)) / q
        return act, lambda z: torch.sigmoid(z * q)

    class NoThreshold(_Mutant):
        stage_name = "edge_forward"

        def wrong(self, name, N, B, graph, t, params, grads, flags):
            with _patched("act_pair", no_threshold):
                CpuOracleBackend._stage(self, name, N, B, graph, t, params, grads, flags)

    ref32, truth = (S.run_stage(S.CpuRunner(dt), "edge_forward", case) for dt in (torch.float32, torch.float64))
    assert not S.compare("stage:edge_forward:softplus-threshold:cpu32", ref32, ref32, truth, sizes=case.sizes)
    got = S.run_stage(S.CpuRunner(torch.float32, backend_cls=NoThreshold), "edge_forward", case)
    assert seen["max"] > 88.7, seen
    assert S.compare("stage:edge_forward:softplus-threshold:mutant", got, ref32, truth, sizes=case.sizes)
