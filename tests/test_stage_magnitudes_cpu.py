"""CPU: what the magnitude cases of tests/test_gpu_stage_magnitudes.py rest on (stage_harness.make_case(..., magnitude=...)).

1. The cases are what they claim.  Every profile rescales the unit draw by exact powers of two, parameters and coordinates untouched, the
   QX_src rows and x consistent; g_far stays clear of fp32's subnormals and every 64-value item of it clear of 2^-113, below which the
   per-item split drops a product (csrc/common.h: vsplit2_scaled).
2. The truth scales.  For every per-graph backward profile the fp64 reference of the scaled case is 2^s_b times the fp64 reference of the
   unit case on every graph-local output, to fp64 rounding; for g_rows on the outputs that depend on their own row alone.
3. The slice-wise rule is not too tight for honest fp32.  The clean fp32 statement of oracle/factored.py in a SECOND association -- the nodes
   of every graph and the edges in another order, so that every sum over rows and over edges adds in another order -- passes every
   magnitude case under stage_harness.compare with the case's groups.
4. The slice-wise rule has teeth where the unit draw has none.  Three mutants emulate the quantisation of the scaled f16x2 split with one
   error of scale bookkeeping each; each passes the unit case of its shape and is reported under a profile.
5. f_ramp stays inside the documented range of the unscaled forward split: no quantity that becomes a matrix-core operand of a forward
   stage -- scaled inputs, pre-activations, activations -- reaches 2^15 or is non-finite in the fp64 evaluation."""
import dataclasses

import pytest
import torch

from oracle import factored as F
from tests import stage_harness as S
from tests.cpu_stage_backend import CpuOracleBackend
from tests.helpers import rel_err

H = 64
ALL_KEYS = sorted({k for st in S.STAGES for k in S.magnitude_keys(st)}, key=repr)
_id = lambda k: S.magnitude_case_id(k, ())      # noqa: E731


# --------------------------------------------------------------------------
# 1. well-formed
# --------------------------------------------------------------------------
@pytest.mark.parametrize("key", ALL_KEYS, ids=_id)
def test_magnitude_case_is_the_unit_draw_times_exact_powers_of_two(key):
    case, unit = S.make_case(*key), S.make_case(*key[:9])
    profile = key[9]
    assert case.key == key and case.name == unit.name + ":mag-" + profile and unit.magnitude == "unit" and unit.row_exp is None
    assert all(a is b for a, b in zip(case.params, unit.params)) and case.grads0 is unit.grads0 and case.edge_index is unit.edge_index
    scaled = set()
    for k, v in case.t.items():
        u = unit.t[k]
        if torch.equal(u, v):
            continue
        scaled.add(k)
        assert torch.equal(v, v.float().double()), k                       # exact in fp32
        live = u != 0
        assert torch.equal(v != 0, live), k
        e = torch.log2((v[live] / u[live]))
        assert torch.equal(e, e.round()) and bool((v[live] / u[live] > 0).all()), f"{k}: a factor that is no power of two"
        rows = {"g_ea0": None}.get(k, case.graph_exp if k in S.G_GRAPH + S.F_GRAPH else case.row_exp)
        if rows is not None:                                               # one factor per row: that of the row's graph / class
            want = torch.exp2(rows.double()).view(-1, *([1] * (u.dim() - 1)))
            cols = slice(0, H) if k == "QX_src" else slice(None)
            assert torch.equal(v.reshape(v.size(0), -1)[:, cols], (u * want).reshape(v.size(0), -1)[:, cols]), k
    if profile in S.BACKWARD_PROFILES:
        assert scaled == {k for k in S.G_NODE + S.G_GRAPH + S.G_EDGE if case.t[k].numel() and (k in S.G_NODE + S.G_EDGE or profile != "g_rows")}
    else:
        assert scaled == {k for k in S.F_NODE + S.F_GRAPH + ("QX_src",) if case.t[k].numel()}
    # the edge-level start value follows the row of its (sorted) edge
    E = case.edge_index.size(1)
    if profile in S.BACKWARD_PROFILES and E:
        want = torch.exp2(case.row_exp[S._sorted_rows(case)].double()).view(-1, 1)
        assert torch.equal(case.t["g_ea0"][:E], unit.t["g_ea0"][:E] * want)
    src = case.t["QX_src"]
    assert torch.equal(src[case.row_begin:case.row_begin + case.N, H:H + 3], case.t["x"]) and torch.equal(case.t["x"], unit.t["x"])
    assert not bool(src[:, H + 3:].any())
    if profile == "g_rows":
        i = torch.arange(case.N)
        assert bool((case.row_exp[(i % 16 == 0) | (i % 16 == 15)] == 20).all()) and bool((case.row_exp[i % 16 == 7] != 0).all())
        ends = torch.tensor(case.sizes).cumsum(0) - 1
        assert bool((case.row_exp[ends[torch.tensor(case.sizes) > 0]] == 20).all())
        assert {int(v) for v in case.row_exp.unique()} == {-20, 0, 20}
    else:
        assert torch.equal(case.row_exp, case.graph_exp[case.batch])
        assert case.graph_exp.tolist() == [S.MAG_GRAPH[profile][b % 3] for b in range(case.B)]


@pytest.mark.parametrize("key", [k for k in ALL_KEYS if k[9] == "g_far"], ids=_id)
def test_g_far_is_normal_fp32_and_clear_of_the_dropped_item_threshold(key):
    """No non-zero value is subnormal in fp32 (|v| >= 2^-126), and every ROW of every gradient operand -- an item of the per-item split is 64
    values of one row; a single N(0,1) value times 2^-100 can lie below 2^-113, an item's maximum cannot -- has its maximum at or above 2^-113,
    the threshold below which vsplit2_scaled drops the item's product.  The largest values stay far inside fp32 (2^30 x 5)."""
    case = S.make_case(*key)
    assert case.B >= 3 and sorted(set(case.graph_exp.tolist())) == [-100, 0, 30]
    for k in S.G_NODE + S.G_GRAPH + S.G_EDGE:
        v = case.t[k]
        if v.numel() == 0:
            continue
        nz = v[v != 0].abs()
        assert float(nz.min()) >= 2.0 ** -126 and float(nz.max()) < 2.0 ** 34, k
        if v.dim() >= 2 and v.size(-1) >= H:
            assert float(v.reshape(-1, v.size(-1))[:, :H].abs().amax(1).min()) >= 2.0 ** -113, k


# --------------------------------------------------------------------------
# 2. the truth scales
# --------------------------------------------------------------------------
def _graph_local(case, groups, out):
    """(name, slice of graph b) of every graph-local output: node- and edge-level buffers by the rows of the graph, per-graph buffers by
    the graph -- parameter gradients are sums over all graphs"""
    for k, v in out.items():
        if k.startswith("grad."):
            continue
        for b in range(case.B):
            if k in S.PER_GRAPH:
                yield k, b, v[b]
            else:
                idx = groups["edge" if k.startswith("g_ea_sorted") else "node"][b][1]
                yield k, b, v[idx]


@pytest.mark.parametrize("key", [k for k in ALL_KEYS if k[9] in ("g_ramp_up", "g_ramp_down", "g_far") and "bf16" not in k[4]], ids=_id)
def test_fp64_truth_of_a_backward_profile_is_the_unit_truth_times_the_graphs_factor(key):
    case, unit = S.make_case(*key), S.make_case(*key[:9])
    groups = S.groups_of(case)
    stages = [st for st in S.BACKWARD if key in S.magnitude_keys(st)]
    assert stages
    for st in stages:
        a = S.reference(st, key, (), 1.0)[1]
        u = S.reference(st, key[:9], (), 1.0)[1]
        assert set(a) == set(u)
        seen = 0
        for (k, b, va), (_, _, vu) in zip(_graph_local(case, groups, a), _graph_local(unit, groups, u)):
            want = vu * 2.0 ** int(case.graph_exp[b])
            if va.numel() == 0:
                continue
            assert rel_err(va, want) < 1e-12, (st, k, b, rel_err(va, want))
            seen += 1
        assert seen >= case.B


def test_fp64_truth_of_g_rows_scales_row_by_row_where_an_output_depends_on_its_own_row_alone():
    """node_pre_backward: g_h and g_vel of a row are functions of that row's upstream gradients (and start value) alone"""
    key = next(k for k in S.magnitude_keys("node_pre_backward") if k[9] == "g_rows")
    case = S.make_case(*key)
    a, u = S.reference("node_pre_backward", key, (), 1.0)[1], S.reference("node_pre_backward", key[:9], (), 1.0)[1]
    f = torch.exp2(case.row_exp.double()).view(-1, 1)
    for k in ("g_h", "g_vel"):
        for lab, idx in S.groups_of(case)["node"]:
            assert rel_err(a[k][idx], (u[k] * f)[idx]) < 1e-12, (k, lab)


# --------------------------------------------------------------------------
# 3. a second association of honest fp32 passes the slice-wise rule
# --------------------------------------------------------------------------
def _reordered(case, seed=5):
    """the same case with the nodes of every graph and the caller's edges in another order, and what takes its outputs back"""
    g = torch.Generator().manual_seed(seed)
    N, E = case.N, case.edge_index.size(1)
    p = torch.cat([off + torch.randperm(n, generator=g) for off, n in zip([sum(case.sizes[:b]) for b in range(case.B)], case.sizes)]) \
        if N else torch.zeros(0, dtype=torch.long)                          # new row j holds old row p[j]
    inv = torch.empty_like(p)
    inv[p] = torch.arange(N)
    eperm = torch.randperm(E, generator=g)
    ei = inv[case.edge_index][:, eperm]
    old_sorted = torch.sort(case.edge_index[0], stable=True).indices       # sorted position -> caller's edge (old numbering of edges)
    pos_old = torch.empty(E, dtype=torch.long)
    pos_old[old_sorted] = torch.arange(E)
    new_sorted = torch.sort(ei[0], stable=True).indices
    to_old = pos_old[eperm[new_sorted]]                                     # new sorted position -> old sorted position
    t = {}
    for k, v in case.t.items():
        if k == "ea":
            t[k] = v[eperm]
        elif k == "g_ea0":
            t[k] = v.clone()
            t[k][:E] = v[to_old]
        elif k in S.G_GRAPH + S.F_GRAPH + ("Z",):
            t[k] = v
        else:
            assert v.size(0) == N, k
            t[k] = v[p]
    new = dataclasses.replace(case, edge_index=ei.contiguous(), t=t, row_exp=None if case.row_exp is None else case.row_exp[p])

    def back(out):
        res = {}
        for k, v in out.items():
            if k.startswith("grad.") or k in S.PER_GRAPH or k == "xsum":
                res[k] = v
            elif k.startswith("g_ea_sorted"):
                res[k] = torch.empty_like(v)
                res[k][to_old] = v
            else:
                res[k] = v[inv]
        return res
    return new, back


@pytest.mark.parametrize("key", [k for k in ALL_KEYS if "bf16" not in k[4]], ids=_id)
def test_clean_fp32_in_a_second_association_passes_every_magnitude_case_slice_by_slice(key):
    case = S.make_case(*key)
    other, back = _reordered(case)
    differs = False
    for st in [st for st in S.STAGES if key in S.magnitude_keys(st)]:
        ref32, truth = S.reference(st, key, (), 1.0)
        name = S.case_name(st, case, "second-association", "cpu32")
        assert not S.compare(name, ref32, ref32, truth, sizes=case.sizes, groups=S.groups_of(case))
        got64 = back(S.run_stage(S.CpuRunner(torch.float64), st, other))
        worst = max(rel_err(got64[k], truth[k]) for k in truth)
        assert worst < 1e-10, (st, worst)                                   # the reordered case IS the case
        got = back(S.run_stage(S.CpuRunner(torch.float32), st, other))
        differs = differs or any(not torch.equal(got[k], ref32[k]) for k in truth)
        bad = S.compare(name, got, ref32, truth, sizes=case.sizes, groups=S.groups_of(case))
        assert not bad, (st, bad)
    assert differs, "the second association is the first: nothing was tested"


# --------------------------------------------------------------------------
# 4. mutants: the quantisation of the scaled f16x2 split with one error of scale bookkeeping
# --------------------------------------------------------------------------
F16_MAX = 65504.0


def _pow2_scale(m):
    """the power of two that puts m into [2^14, 2^15) (1 for m = 0)"""
    e = torch.floor(torch.log2(torch.where(m > 0, m, torch.ones_like(m))))
    return torch.where(m > 0, torch.exp2(14.0 - e), torch.ones_like(m))


def _split2(x, scale):
    """x through the 2-part fp16 split relative to `scale` (csrc/common.h): h = fp16(x S), l = fp16(x S - h), (h + l) / S; a value
    beyond fp16's range saturates at 65 504 / S"""
    y = (x.double() * scale.double()).clamp(-F16_MAX, F16_MAX)
    h = y.to(torch.float16).double()
    l = (y - h).to(torch.float16).double()
    return ((h + l) / scale.double()).to(x.dtype)


class _ScaleMutant(CpuOracleBackend):
    """the gradient operands of one stage (the 64-wide g_* inputs: an item is one row) through a wrong split, the stage itself clean"""
    stage_name = None
    operands = ()

    def _stage(self, name, N, B, graph, t, params, grads, flags):
        if name != self.stage_name:
            return super()._stage(name, N, B, graph, t, params, grads, flags)
        return self.wrong(name, N, B, graph, t, params, grads, flags)

    def quantised(self, t):
        q = dict(t)
        for k in self.operands:
            v = t[k].clone()
            v[:, :H] = self.split(t[k][:, :H])
            q[k] = v
        return q

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        CpuOracleBackend._stage(self, name, N, B, graph, self.quantised(t), params, grads, flags)


class ItemSplitWithTheNeighbourRowsScale(_ScaleMutant):         # (a)
    stage_name, operands, profile = "node_pre_backward", ("g_P", "g_A", "g_QX"), "g_rows"

    def split(self, v):
        m = v.abs().amax(1, keepdim=True)
        other = torch.arange(v.size(0)) ^ 1
        other = torch.where(other < v.size(0), other, torch.arange(v.size(0)))
        return _split2(v, _pow2_scale(m[other]))


class StreamScaleFixedByItsFirstTicket(_ScaleMutant):           # (b)
    """only the weight-gradient consumers take a scale per stream: the parameter gradients come from the operands split under the scale of
    the first 16 rows, everything else from the operands as they are"""
    stage_name, operands, profile = "node_pre_backward", ("g_P", "g_A", "g_QX"), "g_ramp_up"

    def split(self, v):
        return _split2(v, _pow2_scale(v[:16].abs().max()).expand(v.size(0), 1))

    def wrong(self, name, N, B, graph, t, params, grads, flags):
        aside = {k: (v.clone() if torch.is_tensor(v) and v.is_floating_point() else v) for k, v in self.quantised(t).items()}
        CpuOracleBackend._stage(self, name, N, B, graph, aside, params, grads, flags)                      # the parameter gradients
        CpuOracleBackend._stage(self, name, N, B, graph, t, params, [None if g is None else g.clone() for g in grads], flags)


class OperandsBelowFp16RangeOfTheTensorFlushed(_ScaleMutant):   # (c)
    stage_name, operands, profile = "node_pre_backward", ("g_P", "g_A", "g_QX"), "g_rows"

    def split(self, v):
        return torch.where(v.abs() < 2.0 ** -14 * v.abs().max(), torch.zeros_like(v), v)


SCALE_MUTANTS = [ItemSplitWithTheNeighbourRowsScale, StreamScaleFixedByItsFirstTicket, OperandsBelowFp16RangeOfTheTensorFlushed]
MUTANT_SHAPE = S.MAG_SHAPES[0][0] + (0, S.FASTEGNN_WIRING, S.SILU)


def test_the_split_emulation_is_exact_to_fp32_under_the_right_scale():
    """the quantiser of the mutants, with the item's OWN scale, is the identity to 2^-22 of the item's maximum (two 11-bit parts)"""
    v = S.make_case(*MUTANT_SHAPE, "g_rows").t["g_P"].float()
    m = v.abs().amax(1, keepdim=True)
    assert float(((_split2(v, _pow2_scale(m)) - v).abs() / m).max()) <= 2.0 ** -22


@pytest.mark.parametrize("mutant", SCALE_MUTANTS, ids=lambda m: m.__name__)
def test_scale_mutant_passes_the_unit_case_and_is_reported_under_its_profile(mutant):
    st = mutant.stage_name
    out = {}
    for profile in ("unit", mutant.profile):
        key = MUTANT_SHAPE + ((profile,) if profile != "unit" else ())
        case = S.make_case(*key)
        ref32, truth = S.reference(st, key, (), 1.0)
        name = S.case_name(st, case, mutant.__name__, "cpu32")
        assert not S.compare(name, ref32, ref32, truth, sizes=case.sizes, groups=S.groups_of(case))
        got = S.run_stage(S.CpuRunner(torch.float32, backend_cls=mutant), st, case)
        out[profile] = S.compare(name, got, ref32, truth, sizes=case.sizes, groups=S.groups_of(case))
    assert not out["unit"], f"{mutant.__name__} shows on the unit draw already: {out['unit'][:3]}"
    assert out[mutant.profile], f"{mutant.__name__}: not reported under {mutant.profile}"


# --------------------------------------------------------------------------
# 5. f_ramp inside the range of the unscaled forward split
# --------------------------------------------------------------------------
@pytest.mark.parametrize("key", [k for k in ALL_KEYS if k[9] == "f_ramp"], ids=_id)
def test_f_ramp_keeps_every_matrix_core_operand_of_the_forward_below_2_to_15(key):
    case = S.make_case(*key)
    for k in S.F_NODE + S.F_GRAPH + ("QX_src",):
        v = case.t[k]
        assert bool(torch.isfinite(v).all()) and (v.numel() == 0 or float(v.abs().max()) < 2.0 ** 15), k
    real = F.act_pair
    seen = {"max": 0.0, "n": 0, "finite": True}

    def note(v):
        if v.numel():
            seen["n"] += v.numel()
            seen["finite"] = seen["finite"] and bool(torch.isfinite(v).all())
            seen["max"] = max(seen["max"], float(v.detach().abs().max()))
        return v

    def recording(cfg):
        act, dact = real(cfg)
        return (lambda z: note(act(note(z)))), dact

    F.act_pair = recording
    try:
        for st in [st for st in S.FORWARD if key in S.magnitude_keys(st)]:
            out = S.run_stage(S.CpuRunner(torch.float64), st, case)
            for k, v in out.items():
                note(v[:, :H + 3] if k in S.MIXED_QX else v)              # (the pad column of QX belongs to nobody)
    finally:
        F.act_pair = real
    assert seen["n"] > 0 and seen["finite"] and seen["max"] < 2.0 ** 15, seen
