"""TEST INFRASTRUCTURE: one stage of the fused layer at a time, HIP against the CPU statement of the same stage.

The twelve stage entry points of include/fastegnn_hip.h (fastegnn_node_pre_forward ... fastegnn_node_pre_backward) and
tests/cpu_stage_backend.py::CpuOracleBackend.stage share one signature and one set of buffer names.  This module drives
both with the same operands:

  make_case   one layer's parameters, a graph and EVERY buffer a stage reads, each an independent N(0,1) draw (values an
              fp32 holds exactly), so that no term of a stage's output is small or zero by construction;
  run_stage   one stage on one backend (CpuRunner: fp32 or fp64; HipRunner: one of the four shipped libraries), every
              output returned as an fp64 CPU tensor.  On the HIP side every buffer the call can write sits between two
              64-float bands of a fixed NaN bit pattern that must be bit-identical afterwards, and the scratch arrays have
              exactly the sizes the ABI's size functions return;
  compare     every output through tests.helpers.grad_check: err(HIP, fp64) <= 2 x err(CPU fp32, fp64) + 1e-6, per graph
              slice for per-graph buffers, per unit for buffers of mixed units (Q | x), accumulators minus their start value.

Representation of P and Q.  The SiLU builds keep P and the Q columns of QX / QX_src in units of ln 2 (csrc/common.h,
FE_LOG2E_FOLD: what node_pre_forward stores is log2(e) x the pre-activation share; the generic-activation builds and the
bf16 operand mode store it plainly).  HipRunner.pq_scale measures which of the two a library does, through the library's own
node_pre_forward.  A case's draw of P / Q is what the LIBRARY holds; the CPU reference of that run takes draw / scale (in
fp64: exact to 1e-16), so the HIP kernels and the fp64 truth see the same operands to the last bit.  Outputs of
node_pre_forward are divided by the scale before they are compared.  Gradients are with respect to the true P / Q in
every build.

Wirings and activations.  make_case takes a wiring -- ("fastegnn",), ("rf",) or ("egnn", with_v, norm) -- and an activation
(Config.act, Config.act_param); the case then carries an oracle.factored.StageConfig, the parameter slots of that wiring's oracle,
and HipRunner builds fastegnn_amd.FastRF / fastegnn_amd.EGNN for its flags.  The EGNN wiring has six stages, one graph (B = 1, a zero
batch) and no virtual buffers; its cases carry an aggx that engages the +-100 clamp and, under norm, pairs below the normalisation's
epsilon.  Without the velocity head (with_v=False) nothing changes in what a stage writes: node_pre_forward stores a zero svel,
virt_backward writes g_svel = <g_x_out, vel> and node_pre_backward adds svel x g_x_out to g_vel without reading g_svel -- every one
of them is compared.  The tables of these cases are at the end of the file; MATRIX and stage_cases are what they were.

No GPU import at module level: the CPU tests use everything but HipRunner."""
from __future__ import annotations

import dataclasses
import functools
from typing import Dict, List, Optional, Tuple

import torch

from oracle import fastegnn_ref as R
from tests.cpu_stage_backend import CpuOracleBackend
from tests.helpers import grad_check, rel_err

H, QX_LD = 64, 68
LOG2E = 1.4426950408889634074
BAND = 64                      # floats of the guard band on each side of a device buffer
BAND_BITS = 0x7FC0BAD5         # a quiet NaN with a payload nothing computes

FLAGS = ("attention", "normalize", "tanh", "noresidual", "gravity", "coords_sum", "bf16")
ALL_FLAGS = ("attention", "normalize", "tanh", "noresidual", "gravity")
GRAVITY = (0.25, -1.0, 0.5)    # not an axis: a swapped component shows

FORWARD = ("node_pre_forward", "graph_xsum", "graph_pre_forward", "edge_forward", "virt_forward", "graph_post_forward")
BACKWARD = ("graph_post_backward", "virt_backward", "graph_pre_backward", "edge_backward", "node_pre_backward")
STAGES = FORWARD + BACKWARD
EGNN_STAGES = ("node_pre_forward", "edge_forward", "virt_forward", "virt_backward", "edge_backward", "node_pre_backward")
EDGE_STAGES = ("edge_forward", "edge_backward")
GRAPH_LEVEL = ("graph_xsum", "graph_pre_forward", "graph_post_forward", "graph_post_backward", "graph_pre_backward")

# buffers compared per graph slice (a 1-node graph is not hidden behind a 300-node one)
PER_GRAPH = ("Bc", "poolV", "poolX", "Z_out", "HvT_out", "g_Bc", "g_Zp", "g_HvT", "g_Z", "g_poolV", "g_poolX", "g_xbar")
MIXED_QX = ("QX", "g_QX_src", "g_QXe")


FASTEGNN_WIRING, SILU = ("fastegnn",), ("silu", 0.0)


def config(C: int, ea: int, na: int, flags: Tuple[str, ...], wiring: tuple = FASTEGNN_WIRING, act: tuple = SILU) -> R.Config:
    """wiring: ("fastegnn",) | ("rf",) | ("egnn", with_v, norm); act: (Config.act, Config.act_param)"""
    assert set(flags) <= set(FLAGS), flags
    if wiring != FASTEGNN_WIRING or act != SILU:
        from oracle.factored import StageConfig
        egnn = wiring[0] == "egnn"
        assert wiring[0] in ("fastegnn", "rf") or (egnn and C == 0 and na == 0 and not flags), (wiring, C, na, flags)
        return StageConfig(node_feat_nf=1, node_attr_nf=na, edge_attr_nf=ea, hidden_nf=H, virtual_channels=C, n_layers=1,
                           residual="noresidual" not in flags and not egnn, attention="attention" in flags,
                           normalize="normalize" in flags, tanh="tanh" in flags, gravity=list(GRAVITY) if "gravity" in flags else None,
                           coords_agg="sum" if "coords_sum" in flags else "mean", bf16="bf16" in flags, act=act[0], act_param=act[1],
                           wiring=wiring[0], with_v=bool(wiring[1]) if egnn else True, norm=bool(wiring[2]) if egnn else False)
    return R.Config(node_feat_nf=1, node_attr_nf=na, edge_attr_nf=ea, hidden_nf=H, virtual_channels=C, n_layers=1,
                    residual="noresidual" not in flags, attention="attention" in flags, normalize="normalize" in flags,
                    tanh="tanh" in flags, gravity=list(GRAVITY) if "gravity" in flags else None,
                    coords_agg="sum" if "coords_sum" in flags else "mean", bf16="bf16" in flags)


@dataclasses.dataclass
class Case:
    name: str
    cfg: R.Config
    flags: Tuple[str, ...]
    sizes: Tuple[int, ...]
    N: int
    B: int
    C: int
    n_src: int
    row_begin: int
    graph_kind: str
    params: List[Optional[torch.Tensor]]      # FASTEGNN_P_* order, fp64 tensors holding fp32 values
    grads0: List[Optional[torch.Tensor]]      # start values of the gradient accumulators
    edge_index: torch.Tensor                  # int64 [2,E]: rows in [row_begin, row_begin + N), cols in [0, n_src)
    batch: torch.Tensor                       # int64 [N]
    t: Dict[str, torch.Tensor]                # every other buffer, fp64 tensors holding fp32 values
    key: tuple = ()                           # the arguments of make_case
    wiring: tuple = ("fastegnn",)
    act: tuple = ("silu", 0.0)
    magnitude: str = "unit"                   # the magnitude profile (MAGNITUDES below)
    row_exp: Optional[torch.Tensor] = None    # int64 [N]: the power of two the profile put on each row; None for "unit"
    graph_exp: Optional[torch.Tensor] = None  # int64 [B]: the same per graph


# --------------------------------------------------------------------------
# graphs
# --------------------------------------------------------------------------
def _no_self(rows, cols, n_src, row_begin, g):
    """move a column that equals its row (in table numbering) to another table entry"""
    same = cols == rows + row_begin
    return torch.where(same, (cols + 1 + torch.randint(0, max(n_src - 1, 1), cols.shape, generator=g)) % n_src, cols)


def _edges(kind: str, sizes, n_src: int, row_begin: int, g: torch.Generator) -> torch.Tensor:
    """COO edges with local rows [0, N) (returned offset by row_begin) and table columns [0, n_src); no self loops."""
    N = sum(sizes)
    empty = torch.zeros(2, 0, dtype=torch.long)
    if kind == "none" or n_src < 2 or N == 0:
        return empty
    if kind in ("random", "two_launch"):          # degree about 6 inside each graph, a fifth of the rows isolated
        rows, cols, off = [], [], 0
        for n in sizes:
            if n >= 2:
                e = 6 * n
                r = torch.randint(0, n, (e,), generator=g)
                c = (r + 1 + torch.randint(0, n - 1, (e,), generator=g)) % n
                rows.append(r + off); cols.append(c + off)
            off += n
        if not rows:
            return empty
        rows, cols = torch.cat(rows), torch.cat(cols)
        iso = torch.rand(N, generator=g) < 0.2
        keep = ~iso[rows]
        rows, cols = rows[keep], cols[keep]
    elif kind == "subrange":                       # rows of a part of a larger source table, columns anywhere in it
        e = 6 * N
        rows = torch.randint(0, N, (e,), generator=g)
        cols = _no_self(rows, torch.randint(0, n_src, (e,), generator=g), n_src, row_begin, g)
        keep = ~(torch.rand(N, generator=g) < 0.2)[rows]
        rows, cols = rows[keep], cols[keep]
    elif kind == "hub":                            # one row of degree 800 among rows of degree 1
        hub = N // 3
        rows = torch.cat([torch.full((800,), hub, dtype=torch.long), torch.arange(N)[torch.arange(N) != hub]])
        cols = _no_self(rows, torch.randint(0, n_src, rows.shape, generator=g), n_src, row_begin, g)
    elif kind == "deg32_33":                       # rows of degree exactly 32 and 33 (one chunk of edges and one more)
        deg = 32 + (torch.arange(N) % 2)
        rows = torch.repeat_interleave(torch.arange(N), deg)
        cols = _no_self(rows, torch.randint(0, n_src, rows.shape, generator=g), n_src, row_begin, g)
    elif kind == "one_col":                        # every edge into one column
        c0 = n_src // 2
        rows = torch.arange(N)[torch.arange(N) + row_begin != c0].repeat(2)
        cols = torch.full_like(rows, c0)
    else:
        raise KeyError(kind)
    ei = torch.stack([rows + row_begin, cols])
    assert not bool((ei[0] == ei[1]).any()) and (ei.numel() == 0 or (int(ei[1].min()) >= 0 and int(ei[1].max()) < n_src))
    return ei[:, torch.randperm(ei.size(1), generator=g)].contiguous()


# --------------------------------------------------------------------------
# cases
# --------------------------------------------------------------------------
def _layer_params(cfg, wiring, seed):
    """one layer's parameters under the FASTEGNN_P_* slot names, from the parameter set of the wiring's oracle: oracle.fastegnn_ref's
    (init_params), oracle.fastrf_ref's (the same without node_mlp / node_mlp_virtual, coord_mlp_vel.0.weight [H,1]), oracle.egnn_ref's
    (state_dict keys of models/basic.py, mapped to slots as fastegnn_amd.egnn does)"""
    dt = torch.float64
    if wiring[0] == "egnn":
        from fastegnn_amd.egnn import _SLOT_OF
        g = torch.Generator().manual_seed(seed)
        q = {}
        for name, (o, i) in {"edge_message_net.scalar_net.mlp.0": (H, 1 + 2 * H + cfg.edge_attr_nf), "edge_message_net.scalar_net.mlp.2": (H, H),
                             "coord_net.mlp.0": (H, H), "coord_net.mlp.2": (1, H), "node_net.mlp.0": (H, 2 * H), "node_net.mlp.2": (H, H),
                             **({"node_v_net.mlp.0": (H, H), "node_v_net.mlp.2": (1, H)} if cfg.with_v else {})}.items():
            lin = R._linear(g, o, i, dtype=dt)
            if name == "coord_net.mlp.2":                  # an O(1) head, as coord_gain = 1.0 below
                lin["weight"] = R._xavier(g, o, i, 1.0, dtype=dt)["weight"]
            q[name + ".weight"], q[name + ".bias"] = lin["weight"], lin["bias"]
        return {"gcl_0." + slot: q[key].float().double() for slot, key in _SLOT_OF.items() if key in q}
    # O(1) heads (coord_gain 1.0, not the 1e-3 of a fresh model): no output hides behind a small weight
    p = {k: v.float().double() for k, v in R.init_params(cfg, seed=seed, coord_gain=1.0, dtype=dt).items()}
    if wiring[0] == "rf":
        p = {k: v for k, v in p.items() if ".node_mlp" not in k}
        p["gcl_0.coord_mlp_vel.0.weight"] = R._linear(torch.Generator().manual_seed(7700 + seed), H, 1, dtype=dt)["weight"].float().double()
    return p


def _ulps(v, k):
    """v + k units in the last place of each fp32 component of v (exact in fp32; v != 0)"""
    return v + k * torch.exp2(torch.floor(torch.log2(v.abs())) - 23)


def _egnn_operand_edges(cfg, t, ei, n_src, row_begin, g):
    """the two operand edges of the EGNN wiring a random draw does not produce (after the draw, in place)
    clamp engaged: aggx x 100 (about a third of its components beyond +-100), eight components exactly on the gate's boundary;
    norm below its epsilon: eight connected pairs whose coordinates differ by 1..4 ulps per component (r < 1e-12, r x 1e12 a live
    feature with derivative 1e12) and four that coincide (r = 0) -- fewer of each on a graph too small for twelve disjoint pairs.  The row node of each pair is moved onto its column node; a row node is
    brought below 1 first (an exact power of two), so that r <= 3 x (4 x 2^-24)^2 = 1.7e-13 stays well clear of the epsilon in fp32 and fp64."""
    a = t["aggx"] * 100.0
    flat = a.view(-1)
    pick = torch.randperm(flat.numel(), generator=g)[:8]
    flat[pick] = torch.tensor([100.0, -100.0] * 4, dtype=a.dtype)[:pick.numel()]
    t["aggx"] = a
    if not cfg.norm or ei.size(1) == 0:
        return
    src, x = t["QX_src"], t["x"]
    moved, anchor, done = set(), set(), 0
    for e in torch.randperm(ei.size(1), generator=g).tolist():
        r, c = int(ei[0, e]), int(ei[1, e])               # table numbering
        if r in moved or r in anchor or c in moved:
            continue
        xc = src[c, H:H + 3].clone()
        big = float(xc.abs().max())
        if big >= 1.0:                                    # (only an anchor nobody has used yet is rescaled)
            if c in anchor:
                continue
            xc = xc * 2.0 ** -(int(torch.floor(torch.log2(torch.tensor(big)))) + 1)
            src[c, H:H + 3] = xc
            if row_begin <= c < row_begin + x.size(0):
                x[c - row_begin] = xc
        k = torch.randint(1, 5, (3,), generator=g).double() * (torch.randint(0, 2, (3,), generator=g).double() * 2 - 1)
        xr = xc.clone() if done % 3 == 2 else _ulps(xc, k)     # every third pair coincides: a graph too small for twelve pairs has both kinds
        x[r - row_begin] = xr
        src[r, H:H + 3] = xr
        moved.add(r); anchor.add(c)
        done += 1
        if done == 12:
            break


@functools.lru_cache(maxsize=None)
def make_case(sizes: Tuple[int, ...], C: int, ea: int, na: int, flags: Tuple[str, ...], graph_kind: str = "random",
              seed: int = 0, wiring: tuple = FASTEGNN_WIRING, act: tuple = SILU, magnitude: str = "unit") -> Case:
    from fastegnn_amd._lib import PARAM_SLOTS
    sizes, flags = tuple(sizes), tuple(flags)
    if magnitude != "unit":
        return _with_magnitude(make_case(sizes, C, ea, na, flags, graph_kind, seed, wiring, act), magnitude)
    cfg = config(C, ea, na, flags, wiring, act)
    N, B = sum(sizes), len(sizes)
    sub = graph_kind == "subrange"
    n_src, row_begin = (N + 37, 19) if sub else (N, 0)
    g = torch.Generator().manual_seed(1000 + seed)

    def rnd(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float32).double()

    p = _layer_params(cfg, wiring, seed)
    params = [p.get("gcl_0." + s) for s in PARAM_SLOTS]
    grads0 = [rnd(*w.shape) if w is not None else None for w in params]
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    ei = _edges(graph_kind, sizes, n_src, row_begin, g)
    E = ei.size(1)
    t = {}
    # layer inputs and products of earlier stages: each drawn on its own
    for k, s in dict(h=(N, H), x=(N, 3), vel=(N, 3), Z=(B, 3, C), HvT=(B, C, H), P=(N, H), A=(N, H), Bc=(B, C, H), svel=(N,),
                     sgrav=(N,), aggm=(N, H), aggx=(N, 3)).items():
        t[k] = rnd(*s)
    if na:
        t["node_attr"] = rnd(N, na)
    if ea:
        t["ea"] = rnd(E, ea)                       # in the caller's edge order; every backend sorts it with its own graph
    src = rnd(n_src, QX_LD)                        # Q | x | pad of the source table; the part's own rows carry its x
    src[:, H + 3:] = 0.0
    src[row_begin:row_begin + N, H:H + 3] = t["x"]
    t["QX_src"] = src
    # upstream gradients: each drawn on its own
    for k, s in dict(g_h_out=(N, H), g_x_out=(N, 3), g_Z_out=(B, 3, C), g_HvT_out=(B, C, H), g_aggm=(N, H), g_aggx=(N, 3),
                     g_poolV=(B, C, H), g_poolX=(B, 3, C), g_Bc=(B, C, H), g_Zp=(B, 3, C), g_P=(N, H), g_A=(N, H), g_svel=(N,),
                     g_sgrav=(N,), g_QX=(N, QX_LD), g_xrow=(N, 3), g_xbar=(B, 3)).items():
        t[k] = rnd(*s)
    # start values of what the ABI accumulates (+=): '=' in the place of '+=' shows
    for k, s in dict(g_vel0=(N, 3), g_h0=(N, H), g_x0=(N, 3), g_HvT0=(B, C, H), g_Z0=(B, 3, C),
                     g_ea0=(max(E, 1), max(ea, 1)), g_na0=(N, max(na, 1))).items():
        t[k] = rnd(*s)
    name = f"{'x'.join(map(str, sizes))}c{C}e{ea}a{na}-{graph_kind}"
    if wiring[0] == "egnn":
        _egnn_operand_edges(cfg, t, ei, n_src, row_begin, g)
    if wiring != FASTEGNN_WIRING or act != SILU:
        name += "-" + wiring_tag(wiring, act)
        return Case(name, cfg, flags, sizes, N, B, C, n_src, row_begin, graph_kind, params, grads0, ei, batch, t,
                    key=(sizes, C, ea, na, flags, graph_kind, seed, wiring, act), wiring=wiring, act=act)
    return Case(name, cfg, flags, sizes, N, B, C, n_src, row_begin, graph_kind, params, grads0, ei, batch, t,
                key=(sizes, C, ea, na, flags, graph_kind, seed))


# --------------------------------------------------------------------------
# magnitude profiles: the finished unit draw, rescaled in place by exact powers of two (make_case(..., magnitude=...)).
# The default build splits every gradient operand relative to a power-of-two scale -- per 64-value item (csrc/common.h: vsplit2_scaled)
# or per operand stream of a weight-gradient consumer (WgScale) -- and a plain randn draw gives every item and every ticket the SAME
# scale: a scale taken from the wrong lanes, a stream scale that is never lowered, an inverse applied before a lowering all compute the
# right number there.  Under a profile the rows of one tensor differ by 2^12 .. 2^130.
#   backward profiles scale the upstream gradients (G_NODE / G_GRAPH / G_EDGE: every g_* operand and the start values of what the ABI
#   accumulates); the backward is linear in them and the graphs of a batch are independent, so the truth of every graph-local output of
#   a per-graph profile is exactly 2^s_b times the unit case's (tests/test_stage_magnitudes_cpu.py);
#   the forward profile scales the feature operands (F_NODE / F_GRAPH and the Q block of QX_src) mildly; nothing is linear there.
# Parameters, coordinates, velocities, attributes and the start values of the PARAMETER gradients are never scaled.
# --------------------------------------------------------------------------
MAG_GRAPH = {"g_ramp_up": (-12, 0, 12), "g_ramp_down": (12, 0, -12), "g_far": (-100, 0, 30), "f_ramp": (-6, 0, 3)}   # s_b, cyclic in graph order
BACKWARD_PROFILES, FORWARD_PROFILES = ("g_ramp_up", "g_ramp_down", "g_rows", "g_far"), ("f_ramp",)
MAGNITUDES = BACKWARD_PROFILES + FORWARD_PROFILES
ROWS_UP, ROWS_DOWN = 20, -20               # g_rows: rows 0 and 15 of every 16-row tile and the last row of every graph; row 7 of every tile
G_NODE = ("g_h_out", "g_x_out", "g_aggm", "g_aggx", "g_P", "g_A", "g_svel", "g_sgrav", "g_QX", "g_xrow", "g_vel0", "g_h0", "g_x0", "g_na0")
G_GRAPH = ("g_Z_out", "g_HvT_out", "g_poolV", "g_poolX", "g_Bc", "g_Zp", "g_xbar", "g_HvT0", "g_Z0")
G_EDGE = ("g_ea0",)                        # rows in sorted-edge order (run_stage hands it over as g_ea_sorted)
F_NODE, F_GRAPH = ("h", "P", "A", "aggm"), ("Bc", "HvT")


def _sorted_rows(case) -> torch.Tensor:
    """local row of every edge in sorted-edge order (the order of g_ea_sorted: a stable sort by row)"""
    return torch.sort(case.edge_index[0] - case.row_begin, stable=True).values


def _with_magnitude(unit: Case, profile: str) -> Case:
    assert profile in MAGNITUDES, profile
    assert unit.n_src == unit.N and unit.row_begin == 0 and unit.graph_kind != "two_launch", "magnitude profiles: whole-table graphs only"
    N, B = unit.N, unit.B
    if profile == "g_rows":
        i = torch.arange(N)
        last = torch.tensor([sum(unit.sizes[:b + 1]) - 1 for b in range(B) if unit.sizes[b] > 0], dtype=torch.long)
        row_exp = torch.zeros(N, dtype=torch.long)
        row_exp[i % 16 == 7] = ROWS_DOWN
        row_exp[(i % 16 == 0) | (i % 16 == 15)] = ROWS_UP
        row_exp[last] = ROWS_UP
        graph_exp = torch.zeros(B, dtype=torch.long)
    else:
        if profile == "g_far":
            assert B >= 3, "g_far: at least three graphs"
        s = MAG_GRAPH[profile]
        graph_exp = torch.tensor([s[b % 3] for b in range(B)], dtype=torch.long)
        row_exp = graph_exp[unit.batch]
    t = {k: v.clone() for k, v in unit.t.items()}

    def scale(k, e):
        v = t[k]
        t[k] = v * torch.exp2(e.double()).view(-1, *([1] * (v.dim() - 1)))

    if profile in BACKWARD_PROFILES:
        assert {k for k in t if k.startswith("g_")} == set(G_NODE + G_GRAPH + G_EDGE)
        for k in G_NODE:
            scale(k, row_exp)
        for k in G_GRAPH:
            scale(k, graph_exp)
        E = unit.edge_index.size(1)
        edge_exp = torch.zeros(t["g_ea0"].size(0), dtype=torch.long)
        edge_exp[:E] = row_exp[_sorted_rows(unit)]
        scale("g_ea0", edge_exp)
    else:
        for k in F_NODE:
            scale(k, row_exp)
        for k in F_GRAPH:
            scale(k, graph_exp)
        q = t["QX_src"][:, :H].clone()
        t["QX_src"][:, :H] = q * torch.exp2(row_exp.double()).view(-1, 1)      # (the x columns, and t["x"] with them, stay)
    for k, v in t.items():
        if not torch.equal(v, unit.t[k]):
            assert torch.equal(v, v.float().double()) and bool(torch.isfinite(v).all()), f"{profile}: {k} is not exact in fp32"
    key = unit.key + ((0,) if len(unit.key) == 6 else ())
    key = key + ((unit.wiring, unit.act) if len(key) == 7 else ()) + (profile,)
    return dataclasses.replace(unit, name=f"{unit.name}:mag-{profile}", t=t, key=key, magnitude=profile, row_exp=row_exp, graph_exp=graph_exp)


def groups_of(case: Case):
    """-> None for a unit case; otherwise the row groups a magnitude case is compared by, as {"node": [(label, rows)], "edge": [(label,
    sorted-edge indices)]}: the rows of every graph and, for g_rows, the three row classes -- so that a slice 12 .. 130 binades under
    the tensor's maximum is held to its OWN magnitude.  An edge belongs to the group of its row."""
    if case.magnitude == "unit":
        return None
    sets = [(f"g{b}", case.batch == b) for b in range(case.B)]
    if case.magnitude == "g_rows":
        sets += [("rows+20", case.row_exp == ROWS_UP), ("rows-20", case.row_exp == ROWS_DOWN), ("rows0", case.row_exp == 0)]
    erow = _sorted_rows(case)
    return {"node": [(lab, torch.nonzero(m).view(-1)) for lab, m in sets],
            "edge": [(lab, torch.nonzero(m[erow]).view(-1)) for lab, m in sets]}


def wiring_tag(wiring: tuple, act: tuple) -> str:
    w = wiring[0] + ("".join(("+v" if wiring[1] else "-v", "+norm" if wiring[2] else "")) if wiring[0] == "egnn" else "")
    return w + ("" if act == SILU else f"-{act[0]}" + (f"{act[1]:g}" if act[1] else ""))


def case_name(stage: str, case: Case, variant: str = "", build: str = "cpu") -> str:
    fl = "+".join(case.flags) or "plain"
    return f"stage:{stage}:{case.name}:{fl}{(',' + variant) if variant else ''}:{build}"


# --------------------------------------------------------------------------
# runners
# --------------------------------------------------------------------------
class CpuRunner:
    """CpuOracleBackend in one dtype"""
    hip = False

    def __init__(self, dtype, backend_cls=CpuOracleBackend):
        self.dtype, self.backend_cls = dtype, backend_cls
        self.name = {torch.float32: "cpu32", torch.float64: "cpu64"}[dtype]

    def backend(self, case):
        return self.backend_cls(None, 1, case.cfg, dtype=self.dtype)

    def pq_scale(self, case):
        return 1.0

    def put(self, v):
        return v.to(self.dtype).clone()

    def put_int(self, v):
        return v.clone()

    def new(self, *shape):
        return torch.full(shape, float("nan"), dtype=self.dtype)

    def scratch(self, n):
        return None

    def get(self, v):
        return v.detach().double().clone()

    def spec(self, case, det):
        return None

    def check_bands(self, what):
        pass

    def reset(self):
        pass


class BandedPool:
    """Device buffers between two BAND-float guard bands of a fixed NaN bit pattern (the tail up to the next multiple of four
    floats belongs to the band behind the buffer); check_bands: every band is bit-identical to what it was filled with"""

    def __init__(self, dev=None):
        self.dev = torch.device("cuda:0") if dev is None else dev
        self._bufs = []

    def _alloc(self, n, dtype=torch.float32):
        assert dtype in (torch.float32, torch.int32)
        flat = torch.empty(BAND + (n + 3) // 4 * 4 + BAND, dtype=torch.int32, device=self.dev)
        flat.fill_(BAND_BITS)
        self._bufs.append((flat, n))
        return flat.view(dtype)[BAND:BAND + n]

    def check_bands(self, what):
        torch.cuda.synchronize()
        for bits, n in self._bufs:
            ok = bool((bits[:BAND] == BAND_BITS).all()) and bool((bits[BAND + n:] == BAND_BITS).all())
            assert ok, f"{what}: a guard band around a {n}-element buffer was written"

    def reset(self):
        self._bufs = []


class HipRunner(BandedPool):
    """One of the shipped libraries (K.lib(act, wide)) behind fastegnn_amd.sharded.HipBackend"""
    hip = True

    def __init__(self, act: bool, wide: bool):
        from fastegnn_amd.sharded import HipBackend
        super().__init__()
        self.be = HipBackend(self.dev, act=act, wide=wide)
        self.name = "hip" + ("_act" if act else "") + ("_x3" if wide else "")
        self._scale = {}

    def backend(self, case):
        return self.be

    def put(self, v):
        out = self._alloc(v.numel()).view(v.shape)
        out.copy_(v.to(torch.float32))
        return out

    def put_int(self, v):
        return v.to(self.dev)

    def new(self, *shape):
        n = 1
        for d in shape:
            n *= d
        return self._alloc(n).view(*shape)         # (stays filled with the NaN pattern: an element nobody writes shows)

    def scratch(self, n):
        return self._alloc(int(n))

    def get(self, v):
        return v.detach().double().cpu()

    def spec(self, case, det):
        import fastegnn_amd
        from fastegnn_amd import _lib as K
        from fastegnn_amd.model import _Spec
        c = case.cfg
        key = (c.virtual_channels, c.edge_attr_nf, c.node_attr_nf, case.flags, det)
        if case.wiring != FASTEGNN_WIRING or case.act != SILU:
            key += (case.wiring, case.act)
        sp = _SPECS.get(key)
        if sp is None and case.wiring[0] == "egnn":
            from tests.gpu_util import act_module
            m = fastegnn_amd.EGNN(1, 1, c.edge_attr_nf, H, activation=act_module(c), device="cuda", with_v=c.with_v, norm=c.norm)
            m.deterministic = det
            m._build_spec()
            sp = _SPECS[key] = m._spec
            present = [s is not None for s in sp.layer_slots[0]]
            assert present == [w is not None for w in case.params], "parameter slots of the module and of the oracle differ"
        if sp is None:
            kw = {}
            if case.act != SILU:
                from tests.gpu_util import act_module
                kw["act_fn"] = act_module(c)
            cls = fastegnn_amd.FastRF if case.wiring[0] == "rf" else fastegnn_amd.FastEGNN
            m = cls(1, c.node_attr_nf, c.edge_attr_nf, H, c.virtual_channels, device="cuda", n_layers=1,
                    residual=c.residual, attention=c.attention, normalize=c.normalize, tanh=c.tanh,
                    gravity=c.gravity, mlp_dtype=torch.bfloat16 if c.bf16 else torch.float32, **kw)
            if c.coords_agg == "sum":
                m._extra_flags = m._extra_flags | K.F_COORDS_SUM
            sp = _SPECS[key] = _Spec(m, deterministic=det)
            present = [s is not None for s in sp.layer_slots[0]]
            assert present == [w is not None for w in case.params], "parameter slots of the module and of the oracle differ"
        return sp

    def pq_scale(self, case):
        """1.0 or log2(e): the units in which this library keeps P and Q for this operand mode (module docstring)"""
        bf = case.cfg.bf16
        if bf not in self._scale:
            self._scale[bf] = self._probe(bf, FASTEGNN_WIRING, SILU)
        if case.wiring != FASTEGNN_WIRING or case.act != SILU:      # probed once more under each wiring and activation: one library, one answer
            key = (bf, case.wiring, case.act)
            if key not in self._scale:
                self._scale[key] = self._probe(bf, case.wiring, case.act)
                assert self._scale[key] == self._scale[bf], f"{self.name}: P in other units under {wiring_tag(case.wiring, case.act)}"
        return self._scale[bf]

    def _probe(self, bf, wiring, act):
        probe = make_case((16,), 0 if wiring[0] == "egnn" else 1, 0, 0, ("bf16",) if bf else (), "none", 99, wiring, act)
        got = run_stage(self, "node_pre_forward", probe, _raw=True)
        ref = run_stage(CpuRunner(torch.float64), "node_pre_forward", probe)
        r = float((got["P"] * ref["P"]).sum() / (ref["P"] * ref["P"]).sum())
        s = min((1.0, LOG2E), key=lambda v: abs(v - r))
        assert abs(r - s) < (2e-2 if bf else 1e-4), f"{self.name}: P is {r} x the pre-activation share: neither plain nor in units of ln 2"
        return s


_SPECS: dict = {}


# --------------------------------------------------------------------------
# one stage
# --------------------------------------------------------------------------
def _true_pq(case: Case, scale: float):
    """the pre-activation shares P, Q that a library holding the case's draw in `scale` units works with (exact in fp64)"""
    src = case.t["QX_src"].clone()
    src[:, :H] = src[:, :H] / scale
    return case.t["P"] / scale, src


def run_stage(rn, name: str, case: Case, null: bool = False, want: bool = True, det: bool = False, batch: bool = False,
              accum: bool = False, scale: Optional[float] = None, _raw: bool = False) -> Dict[str, torch.Tensor]:
    """Runs stage `name` of `case` on runner `rn` and returns its outputs as fp64 CPU tensors: plain outputs under their
    buffer name, accumulated buffers (+=) MINUS their start value, parameter gradients as "grad.<slot>" minus their start.
      null   the null h_out / HvT_out (forward) or g_h_out / g_HvT_out (backward) wiring of include/fastegnn_hip.h
      want   g_ea_sorted / g_node_attr are wanted
      det    FASTEGNN_F_DETERMINISTIC (edge_backward: g_QXe + edge_col_reduce on a graph with the CSC index)
      batch  HIP only: the stage queues into an open weight-gradient batch (wgrad_open ... wgrad_close)
      accum  edge_backward with FASTEGNN_F_GQX_ACCUM on a g_QX_src that holds the sums of an earlier launch
      scale  CPU only: the units of the case's P / Q draw (what the HIP run it is the reference of measured)"""
    from fastegnn_amd._lib import F_GQX_ACCUM, PARAM_SLOTS
    t, N, B, C, cfg = case.t, case.N, case.B, case.C, case.cfg
    be = rn.backend(case)
    rn.reset()
    if rn.hip:
        scale = 1.0 if _raw else rn.pq_scale(case)
        rn.reset()
        P_in, src_in = t["P"], t["QX_src"]         # the library's own representation
    else:
        scale = 1.0 if scale is None else scale
        P_in, src_in = _true_pq(case, scale)
    spec = rn.spec(case, det)
    rf, egnn = case.wiring[0] == "rf", case.wiring[0] == "egnn"
    assert not (egnn and name not in EGNN_STAGES), f"{name}: the EGNN wiring has no per-graph stages"
    assert not (null and (rf or egnn)), "a null h_out / g_h_out is an error under the rf and egnn wirings (test it as one)"
    grav = cfg.gravity is not None
    ea, na = cfg.edge_attr_nf, cfg.node_attr_nf
    edge = name in EDGE_STAGES
    two = case.graph_kind == "two_launch" and name == "edge_backward"
    params = [rn.put(w) if w is not None else None for w in case.params]
    b = {}                                         # the stage's view of the layer: name -> backend tensor
    outs, accs = {}, {}                            # plain outputs; accumulators: name -> (buffer, start value)

    def inp(*keys):
        for k in keys:
            b[k] = rn.put(t[k])

    def out(k, *shape):
        b[k] = outs[k] = rn.new(*shape)

    def acc(k, start):
        b[k] = rn.put(start)
        accs[k] = (b[k], start)

    b["batch"] = rn.put_int(case.batch.to(torch.int32) if rn.hip else case.batch)
    if rn.hip:
        b["wpack"] = rn.scratch((be.wpack_floats(C) + 3) // 4 * 4)
    graph = None

    def build_graph(ei, n_rows, row0):
        return be.build_graph(rn.put_int(ei), n_rows, case.n_src, row0, csc=det)

    if not two:
        graph = build_graph(case.edge_index, N, case.row_begin)
    else:
        graph = build_graph(case.edge_index[:, :0], N, case.row_begin)     # (sizes of the descriptor of the non-edge calls)
    if rn.hip:
        be.stage("pack_weights", spec, N, B, graph, dict(wpack=b["wpack"]), params)

    def call(stage, tb=None, gr=None, n_rows=None, grads=None, flags=0):
        be.stage(stage, spec, N if n_rows is None else n_rows, B, graph if gr is None else gr,
                 {k: v for k, v in (b if tb is None else tb).items() if v is not None}, params, grads, flags)

    def xsum():
        inp("x")
        b["xsum"] = rn.new(B, 4)
        call("graph_xsum")

    def virt_forward_products():
        """npre, poolV, poolX of the backend under test, from its own virt_forward on the case's operands"""
        if egnn:                                   # C = 0: no virtual buffers, no pools (fastegnn_amd/egnn.py)
            inp("h", "A", "x", "vel", "aggm", "aggx", "svel")
            b["x_out"], b["h_out"], b["npre"] = rn.new(N, 3), rn.new(N, H), rn.new(N, H)
            call("virt_forward")
            return
        inp("h", "A", "Bc", "x", "vel", "Z", "aggm", "aggx", "svel", "sgrav")
        if na:
            inp("node_attr")
        b["x_out"], b["poolX"] = rn.new(N, 3), rn.new(B, 3, C)
        if not null:
            b["h_out"], b["npre"], b["poolV"] = rn.new(N, H), rn.new(N, H), rn.new(B, C, H)
        call("virt_forward")

    grads = None
    if name in BACKWARD:
        grads = [rn.put(g0) if g0 is not None else None for g0 in case.grads0]
        if rn.hip:
            b["wg_slab"] = rn.scratch(be.wg_slab_floats())
            b["wg_node"] = rn.scratch(be.wg_node_floats(N, B, C))
    wb = None

    if name == "node_pre_forward":
        inp("h", "x")
        if rf:
            inp("vel")                             # the velocity head's operand (its detached norm)
        # svel is an output under every wiring: without the head (EGNN, with_v=False) the kernel stores zeros, and so does the statement
        out("P", N, H); out("QX", N, QX_LD); out("A", N, H); out("svel", N)
        if grav:
            out("sgrav", N)
    elif name == "graph_xsum":
        inp("x")
        out("xsum", B, 4)
    elif name == "graph_pre_forward":
        xsum()
        inp("Z", "HvT")
        out("Bc", B, C, H)
    elif name == "edge_forward":
        b["P"], b["QX_src"], b["x"] = rn.put(P_in), rn.put(src_in), rn.put(t["x"])
        b["QX"] = b["QX_src"][case.row_begin:case.row_begin + N]
        b["ea_sorted"] = graph.permute(rn.put(t["ea"])) if ea else None
        out("aggm", N, H); out("aggx", N, 3)
    elif name == "virt_forward":
        virt_forward_products()
        # (rf: poolV is zeroed, not summed -- nothing pools v without node_model_virtual; the statement holds zeros)
        for k in ("x_out", "h_out") if egnn else ("x_out", "poolX") + (() if null else ("h_out", "poolV")):
            outs[k] = b[k]
    elif name == "graph_post_forward":
        xsum()
        virt_forward_products()
        for k in ("h_out", "x_out", "npre"):
            b.pop(k, None)
        inp("HvT")
        out("Z_out", B, 3, C)
        if not null:
            out("HvT_out", B, C, H)
    elif name == "graph_post_backward":
        xsum()
        virt_forward_products()
        for k in ("h_out", "x_out", "npre"):
            b.pop(k, None)
        inp("HvT", "g_Z_out")
        if not null:
            inp("g_HvT_out")
            out("g_poolV", B, C, H)
        out("g_Z", B, 3, C); out("g_HvT", B, C, H); out("g_poolX", B, 3, C)
    elif name == "virt_backward":
        virt_forward_products()
        for k in ("h_out", "x_out", "poolV", "poolX"):
            b.pop(k, None)
        if egnn:
            inp("g_x_out", "g_h_out")
        else:
            inp("g_x_out", "g_poolX")
            if not null:
                inp("g_h_out", "g_poolV")
        # g_svel = <g_x_out, vel> is written under every wiring (with_v=False: node_pre_backward does not read it)
        shapes = dict(g_h=(N, H), g_x=(N, 3), g_A=(N, H), g_aggm=(N, H), g_aggx=(N, 3), g_svel=(N,))
        if not egnn:
            shapes.update(g_Bc=(B, C, H), g_Zp=(B, 3, C))
        for k, s in shapes.items():
            out(k, *s)
        if grav:
            out("g_sgrav", N)
        if na and want and not null:
            acc("g_node_attr", t["g_na0"])
        if rn.hip and not egnn:
            b["wg_virt"] = rn.scratch(be.wg_virt_floats(N, C, spec.flags))
    elif name == "graph_pre_backward":
        xsum()
        inp("Z", "HvT", "g_Bc", "g_Zp")
        acc("g_HvT", t["g_HvT0"]); acc("g_Z", t["g_Z0"])
        b["g_xbar"] = outs["g_xbar"] = rn.new(B * 4) if rn.hip else rn.new(B, 4)
    elif name == "edge_backward":
        b["P"], b["QX_src"], b["x"] = rn.put(P_in), rn.put(src_in), rn.put(t["x"])
        b["QX"] = b["QX_src"][case.row_begin:case.row_begin + N]
        inp("g_aggm", "g_aggx")
        out("g_P", N, H); out("g_xrow", N, 3)
        if accum:
            # FASTEGNN_F_GQX_ACCUM adds to the col-keyed sums an earlier launch of the layer left over OTHER rows: the start value is
            # such a table -- the exact sums of this very launch, dealt to other table rows (what the table holds decides the
            # rounding of every atomic that lands in it: a start value of another magnitude would measure that, not the kernel)
            base = reference(name, case.key, (), scale)[1]["g_QX_src"]
            deal = torch.randperm(case.n_src, generator=torch.Generator().manual_seed(7))
            start = base[deal]
            if case.row_exp is not None:           # a magnitude case: every row starts at the magnitude of its OWN sums (an exact factor)
                start = start * torch.exp2((case.row_exp - case.row_exp[deal]).double()).view(-1, 1)
            acc("g_QX_src", start.float().double())
        else:
            out("g_QX_src", case.n_src, QX_LD)
        if rn.hip:
            b["wg_edge"] = rn.scratch(be.wg_edge_floats(case.edge_index.size(1)))
    elif name == "node_pre_backward":
        inp("h", "g_P", "g_QX", "g_A", "g_svel", "g_sgrav", "g_xrow", "g_x_out", "svel")
        if rf:
            inp("vel")
        # g_vel += svel x g_x_out under every wiring (with_v=False: the caller's svel is the zero table; here it is a draw)
        gx = torch.zeros(B, 4, dtype=torch.float64)
        if rn.hip:                                 # the kernels' g_xbar is [B,3] packed (in a [B,4]-sized scratch array)
            gx.view(-1)[:B * 3] = t["g_xbar"].reshape(-1)
            gx = gx.view(-1)
        else:
            gx[:, :3] = t["g_xbar"]
        b["g_xbar"] = rn.put(gx)
        acc("g_h", t["g_h0"]); acc("g_x", t["g_x0"]); acc("g_vel", t["g_vel0"])
    else:
        raise KeyError(name)

    # ---- the call itself
    snap = None
    try:
        if name in BACKWARD and batch and rn.hip:
            wb = be.wgrad_open(spec, N, B, graph, dict(wg_slab=b["wg_slab"]), params)
            b["wgrad_batch"] = wb
        if name == "edge_backward":
            every = torch.ones(case.edge_index.size(1), dtype=torch.bool)
            if not two:
                parts = [(0, N, every, graph)]
            else:                                  # two launches over disjoint row ranges; the second adds to g_QX_src
                n1 = N // 2
                m1 = case.edge_index[0] < n1
                parts = [(r0, n, m, build_graph(case.edge_index[:, m].contiguous(), n, r0)) for r0, n, m in ((0, n1, m1), (n1, N - n1, ~m1))]
            g_ea_parts = []
            for k, (r0, n, mask, gr) in enumerate(parts):
                ei = case.edge_index[:, mask]
                tb = dict(b)
                for key in ("P", "QX", "x", "g_aggm", "g_aggx", "g_P", "g_xrow"):
                    tb[key] = b[key][r0:r0 + n]
                if ea:
                    tb["ea_sorted"] = gr.permute(rn.put(t["ea"][mask]))
                    if want:
                        start = t["g_ea0"][:max(ei.size(1), 1), :ea]
                        tb["g_ea_sorted"] = rn.put(start)
                        g_ea_parts.append((tb["g_ea_sorted"], start, ei.size(1)))
                if rn.hip:                         # per-edge rows of the deterministic form; one row otherwise, as the callers carve it
                    tb["g_QXe"] = rn.scratch((max(ei.size(1), 1) if det else 1) * QX_LD)
                fl = F_GQX_ACCUM if (accum or k > 0) else 0
                call("edge_backward", tb, gr, n, grads, fl)
                call("edge_col_reduce", tb, gr, n, grads)
        else:
            call(name, grads=grads)
        if wb is not None:
            torch.cuda.synchronize()
            snap = {k: v.clone() for k, v in b.items() if isinstance(v, torch.Tensor) and k not in ("wg_slab", "wg_edge", "wg_virt")}
    finally:
        if wb is not None:
            be.wgrad_close(wb)
    rn.check_bands(case_name(name, case, build=rn.name))
    if snap is not None:
        for k, v in snap.items():
            same = torch.equal(v.view(torch.int32), b[k].view(torch.int32)) if v.is_floating_point() else torch.equal(v, b[k])
            assert same, f"{name}: {k} changed between the stage call and fastegnn_wgrad_batch_close"

    # ---- outputs
    res = {k: rn.get(v) for k, v in outs.items()}
    for k, (buf, start) in accs.items():
        res[k] = rn.get(buf) - start
    if name == "edge_backward" and ea and want:
        for k, (buf, start, e) in enumerate(g_ea_parts):
            res["g_ea_sorted" + (f".{k}" if two else "")] = (rn.get(buf) - start)[:e]
    if "g_xbar" in res:
        res["g_xbar"] = res["g_xbar"].reshape(-1)[:B * 3].reshape(B, 3) if rn.hip else res["g_xbar"][:, :3].clone()
    if name == "node_pre_forward" and rn.hip and not _raw:      # what the library stores -> the pre-activation shares
        res["P"] = res["P"] / scale
        res["QX"][:, :H] = res["QX"][:, :H] / scale
    if grads is not None:
        for s, g, g0 in zip(PARAM_SLOTS, grads, case.grads0):
            if g is not None:
                res["grad." + s] = rn.get(g) - g0
    rn.reset()
    return res


@functools.lru_cache(maxsize=None)
def reference(name: str, case_key: tuple, variant: tuple, scale: float):
    """(fp32, fp64) outputs of the CPU statement of a stage: computed once, shared by every build (never modified)"""
    case = make_case(*case_key)
    kw = dict(variant)
    return (run_stage(CpuRunner(torch.float32), name, case, scale=scale, **kw),
            run_stage(CpuRunner(torch.float64), name, case, scale=scale, **kw))


# --------------------------------------------------------------------------
# comparison
# --------------------------------------------------------------------------
BF16_FACTOR, BF16_FLOOR = 3.0, 5e-3      # tests/test_gpu_bf16.py: distance to the fp64 mirror <= 3 x the fp32 mirror's own + 5e-3


LEDGER = None            # a list: every comparison is noted in it as (case, buffer, err / tolerance) -- the accuracy record of a run


def _check(case, key, got, ref32, truth, bad, bf16):
    if not bool(torch.isfinite(got).all()):
        bad.append(f"{key}: {int((~torch.isfinite(got)).sum())} of {got.numel()} elements not finite (never written?)")
        return
    if truth.numel() == 0:
        return
    if LEDGER is not None:
        from tests.helpers import grad_tolerance
        e_got, e_ref = rel_err(got, truth), rel_err(ref32, truth)
        LEDGER.append((case, key, e_got / (BF16_FACTOR * e_ref + BF16_FLOOR if bf16 else grad_tolerance(case, key, e_ref))))
    if bf16:
        e_got, e_ref = rel_err(got, truth), rel_err(ref32, truth)
        if e_got > BF16_FACTOR * e_ref + BF16_FLOOR:
            bad.append(f"{key} {e_got:.2e} (mirror32 {e_ref:.2e})")
        return
    grad_check(case, key, got, ref32, truth, bad)


def compare(case: str, got: Dict[str, torch.Tensor], ref32: Dict[str, torch.Tensor], truth64: Dict[str, torch.Tensor],
            sizes=None, bf16: bool = False, groups=None) -> List[str]:
    """-> the comparisons of `got` that are further from `truth64` than the project's rule allows (tests.helpers.grad_check;
    the bf16 mode's own rule with bf16=True).  Every key of truth64 must be in got: a missing output is reported.  A parameter
    gradient the stage must leave alone ("grad.<slot>" whose truth is zero everywhere) must be exactly its start value.
    groups (groups_of(case), a magnitude case): every node- and edge-level buffer is ALSO compared on the rows of each group."""
    bad: List[str] = []
    n_node = sum(sizes) if sizes is not None else None
    assert groups is None or sizes is not None
    ptr = None
    if sizes is not None:
        ptr = [0]
        for n in sizes:
            ptr.append(ptr[-1] + n)
    for k, tr in truth64.items():
        if k not in got:
            bad.append(f"{k} missing")
            continue
        g, r = got[k], ref32[k]
        if g.shape != tr.shape:
            bad.append(f"{k}: shape {tuple(g.shape)} for {tuple(tr.shape)}")
            continue
        if k.startswith("grad.") and not bool(tr.any()):
            if bool(g.any()):
                bad.append(f"{k}: a gradient this stage does not own moved by {float(g.abs().max()):.2e}")
            continue
        if k == "xsum":
            if not torch.equal(g[:, 3], tr[:, 3]):
                bad.append(f"xsum: node counts {g[:, 3].tolist()} for {tr[:, 3].tolist()}")
            for i in range(tr.size(0)):
                _check(case, f"xsum[g{i}]", g[i, :3], r[i, :3], tr[i, :3], bad, bf16)
        elif k in MIXED_QX:
            _check(case, k + ":Q", g[:, :H], r[:, :H], tr[:, :H], bad, bf16)
            _check(case, k + ":x", g[:, H:H + 3], r[:, H:H + 3], tr[:, H:H + 3], bad, bf16)
        elif k in PER_GRAPH:
            for i in range(tr.size(0)):
                _check(case, f"{k}[g{i}]", g[i], r[i], tr[i], bad, bf16)
        else:
            _check(case, k, g, r, tr, bad, bf16)
        if groups is not None and not k.startswith("grad.") and k != "xsum" and k not in PER_GRAPH and tr.dim() >= 1:
            # a magnitude case: the rows of each group on their own as well, under the same rule -- the tolerance of a slice is set by
            # the fp32 CPU evaluation's error on THAT slice (weight gradients and other sums over all rows stay whole-tensor comparisons)
            level = "edge" if k.startswith("g_ea_sorted") else "node"
            if level == "node" and tr.size(0) != n_node:
                bad.append(f"{k}: {tr.size(0)} rows: neither a node-level nor an edge-level buffer of a magnitude case")
                continue
            for lab, idx in groups[level]:
                if k in MIXED_QX:
                    _check(case, f"{k}:Q[{lab}]", g[idx, :H], r[idx, :H], tr[idx, :H], bad, bf16)
                    _check(case, f"{k}:x[{lab}]", g[idx, H:H + 3], r[idx, H:H + 3], tr[idx, H:H + 3], bad, bf16)
                else:
                    _check(case, f"{k}[{lab}]", g[idx], r[idx], tr[idx], bad, bf16)
    return bad


# --------------------------------------------------------------------------
# the matrix: the smallest shapes at which these kernels can go wrong (16-row MFMA tiles, 8-wave workgroups, 32-edge row
# chunks, consumer flushes every 768 rows, 1024 nodes per wave of the centroid sums) x every flag, graph kind and width
# --------------------------------------------------------------------------
S_ONE, S_RAGGED, S_EXACT, S_65, S_EMPTY, S_MANY = (1,), (15, 1, 17, 31), (16, 16, 32), (65,), (20, 0, 13), (300, 180, 201)
NA_MAX = 8                     # the widest node_attr the fused path's small contractions take (csrc/misc.hip)
# (sizes, C, ea, na, flags, graph kind)
MATRIX = [
    (S_ONE, 1, 0, 0, ALL_FLAGS, "none"),
    (S_RAGGED, 3, 2, 1, ALL_FLAGS, "random"),
    (S_EXACT, 16, 1, 0, ALL_FLAGS, "random"),
    (S_65, 5, 7, 0, ALL_FLAGS, "deg32_33"),
    (S_EMPTY, 4, 2, 0, ALL_FLAGS, "random"),
    (S_MANY, 16, 2, 0, ALL_FLAGS, "random"),
    (S_MANY, 17, 0, 0, (), "random"),
    (S_MANY, 33, 1, NA_MAX, ("attention",), "hub"),
    (S_MANY, 64, 2, 0, ("normalize",), "random"),
    (S_RAGGED, 3, 2, 1, ("tanh",), "one_col"),
    (S_RAGGED, 3, 0, 0, ("noresidual",), "random"),
    (S_RAGGED, 3, 7, NA_MAX, ("gravity",), "random"),
    (S_RAGGED, 3, 2, 0, ("coords_sum",), "random"),
    (S_RAGGED, 3, 2, 1, (), "random"),
    (S_RAGGED, 3, 2, 1, ("bf16",), "random"),
]
EDGE_ONLY = [                  # graph forms that only the edge stage sees
    (S_EMPTY, 4, 2, 0, (), "none"),
    (S_RAGGED, 3, 2, 0, (), "subrange"),
    (S_MANY, 16, 2, 0, ALL_FLAGS, "subrange"),
    (S_RAGGED, 3, 2, 0, (), "two_launch"),
    (S_65, 5, 2, 0, ALL_FLAGS, "two_launch"),
]
GRAPH_ONLY = [                 # wave and workgroup boundaries of the per-graph sums
    ((4100,), 3, 0, 0, ALL_FLAGS, "none"),
    ((1030, 3070), 3, 0, 0, ALL_FLAGS, "none"),
]
NULL_STAGES = ("virt_forward", "graph_post_forward", "graph_post_backward", "virt_backward")


def stage_cases(stage: str):
    """-> [(case key, variant)] of one stage; variant: the keyword arguments of run_stage that the references share
    (null, want, accum) plus det -- as a sorted tuple of pairs (hashable: reference() caches by it)"""
    keys = list(MATRIX)
    if stage in EDGE_STAGES:
        keys += [k for k in EDGE_ONLY if stage == "edge_backward" or k[5] != "two_launch"]
    if stage in GRAPH_LEVEL:
        keys += GRAPH_ONLY
    out = []
    for k in keys:
        sizes, C, ea, na, flags, kind = k
        out.append((k, ()))
        if stage in NULL_STAGES and (sizes, flags) in ((S_RAGGED, ALL_FLAGS), (S_MANY, ALL_FLAGS), (S_RAGGED, ("bf16",))):
            out.append((k, (("null", True),)))
        if stage == "virt_backward" and na > 0:
            out.append((k, (("want", False),)))
        if stage == "edge_backward":
            if kind != "two_launch":
                out.append((k, (("det", True),)))
            if ea > 0 and (sizes, kind) in ((S_RAGGED, "random"), (S_65, "deg32_33")):
                out.append((k, (("want", False),)))
            if (sizes, flags) in ((S_RAGGED, ALL_FLAGS), (S_MANY, ALL_FLAGS)) and kind != "two_launch":
                out.append((k, (("accum", True),)))
    return out


def variant_id(key, variant) -> str:
    sizes, C, ea, na, flags, kind = key
    v = ",".join(k for k, on in variant if on) + ",".join("no" + k for k, on in variant if not on)
    return f"{'x'.join(map(str, sizes))}c{C}e{ea}a{na}-{kind}-{'+'.join(flags) or 'plain'}" + (f"-{v}" if v else "")


# --------------------------------------------------------------------------
# the sibling wirings and the activation kinds (tests/test_gpu_stage_wirings.py): tables of their own, the matrix above is as it was.
# A key here is the full argument tuple of make_case: (sizes, C, ea, na, flags, graph kind, seed, wiring, act)
# --------------------------------------------------------------------------
RF = ("rf",)
RF_MATRIX = [
    (S_ONE, 1, 0, 0, ALL_FLAGS, "none"),
    (S_RAGGED, 3, 2, 0, ALL_FLAGS, "random"),
    (S_RAGGED, 3, 2, 0, ("bf16",), "random"),
    (S_65, 5, 7, 0, (), "deg32_33"),
    (S_EMPTY, 4, 2, 0, ("gravity",), "random"),
    (S_MANY, 16, 2, 0, ALL_FLAGS, "random"),
]
# (N, ea, graph kind) of the EGNN wiring, one graph each: 16-row tiles around N = 16, one node, degree 32 / 33, a hub, one column
EGNN_SHAPES = [(1, 2, "none"), (15, 2, "random"), (16, 2, "random"), (17, 0, "none"), (17, 7, "random"), (65, 0, "deg32_33"),
               (65, 7, "random"), (681, 2, "hub"), (681, 2, "one_col"), (681, 2, "random")]
EGNN_EDGE_ONLY = [(65, 7, "subrange"), (681, 2, "subrange")]
EDGE_LEVEL, NODE_LEVEL = ("edge_forward", "edge_backward"), ("node_pre_forward", "virt_forward", "virt_backward", "node_pre_backward")

# (Config.act, Config.act_param); the kinked kinds -- a derivative that jumps at 0 -- run at seeds chosen so that no pre-activation of the
# fp64 reference lies within 1e-5 of 0 (KINK_SEEDS; tests/test_stage_harness_cpu.py asserts it), and stay at the small shapes for that
KINDS = [("relu", 0.0), ("leaky_relu", 0.2), ("tanh", 0.0), ("sigmoid", 0.0), ("elu", 1.3), ("gelu", 0.0), ("softplus", 1.7)]
KINKED = ("relu", "leaky_relu", "elu")
KINK_BAND = 1e-5
ACT_SHAPES = [(S_RAGGED, 3, 2, 1, ALL_FLAGS, "random"), (S_65, 5, 7, 0, ALL_FLAGS, "deg32_33"), (S_EMPTY, 4, 2, 0, (), "random")]
ACT_SMOOTH_SHAPES = [(S_ONE, 1, 0, 0, ALL_FLAGS, "none"), (S_MANY, 16, 2, 0, ALL_FLAGS, "random"), (S_MANY, 33, 1, NA_MAX, ("attention",), "hub")]
ACT_X3 = [(k, sh) for k in (("sigmoid", 0.0), ("gelu", 0.0)) for sh in (ACT_SHAPES[0], ACT_SMOOTH_SHAPES[1])]
# act(0) != 0: once under each sibling wiring as well
ACT_SIBLINGS = [(k, w, sh) for k in (("sigmoid", 0.0), ("softplus", 1.7))
                for w, sh in ((RF, (S_RAGGED, 3, 2, 0, ALL_FLAGS, "random")), (("egnn", True, False), ((17,), 0, 7, 0, (), "random")),
                              (("egnn", True, False), ((65,), 0, 0, 0, (), "deg32_33")))]
# (kind, index into ACT_SHAPES, stage) -> the smallest seed >= 0 whose fp64 reference has no pre-activation with |z| < KINK_BAND
KINK_SEEDS = {(kind, i, st): seed for (kind, i), seeds in {
    # in the order of STAGES: node_pre_f, graph_xsum, graph_pre_f, edge_f, virt_f, graph_post_f, graph_post_b, virt_b, graph_pre_b, edge_b, node_pre_b
    # (a stage that runs virt_forward for its operands counts that call's pre-activations too; the 65-node degree-32/33 shape evaluates
    # 400 000 pre-activations in its edge stage: its first clean seed is in the thousands)
    ("relu", 0): (0, 0, 0, 3, 1, 1, 1, 1, 0, 3, 0),
    ("relu", 1): (2, 0, 0, 5057, 38, 38, 38, 38, 0, 5057, 2),
    ("relu", 2): (0, 0, 0, 1, 1, 1, 1, 1, 0, 1, 0),
    ("leaky_relu", 0): (0, 0, 0, 2, 3, 3, 3, 3, 0, 2, 0),
    ("leaky_relu", 1): (2, 0, 0, 10398, 29, 29, 29, 29, 0, 10398, 2),
    ("leaky_relu", 2): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
    ("elu", 0): (0, 0, 0, 0, 2, 2, 2, 2, 0, 0, 0),
    ("elu", 1): (2, 0, 0, 3581, 0, 0, 0, 0, 0, 3581, 2),
    ("elu", 2): (0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0),
}.items() for st, seed in zip(STAGES, seeds)}


def min_abs_preactivation(stage: str, key: tuple) -> float:
    """min |z| over every pre-activation the fp64 statement of `stage` evaluates on the case (inf: the stage has no activation)"""
    from oracle.factored import track_min_abs_z
    with track_min_abs_z() as tr:
        run_stage(CpuRunner(torch.float64), stage, make_case(*key))
    return tr.value


def _variants(stage, k, wiring):
    sizes, C, ea, na, flags, kind = k[:6]
    out = [()]
    if stage == "edge_backward":
        out.append((("det", True),))
        if ea > 0 and (sizes, kind) in ((S_RAGGED, "random"), (S_65, "deg32_33")):
            out.append((("want", False),))
    if stage == "virt_backward" and na > 0:
        out.append((("want", False),))
    return out


def rf_cases(stage: str, duplicate: bool = False):
    """duplicate: the run on a second build of the same kernels, without the variants"""
    return [(k + (0, RF, SILU), v) for k in RF_MATRIX for v in (_variants(stage, k, RF)[:1] if duplicate else _variants(stage, k, RF))]


def egnn_cases(stage: str, duplicate: bool = False):
    """the six stages of the EGNN wiring; with_v and norm on and off where the stage can see them: norm lives in the edge stage,
    the velocity head in the node-level stages (the other switch is crossed in at N = 17).  duplicate: the run on a second build of
    the same kernels -- the first setting of a shape, and norm in the edge stages; without N = 15, 16 and the one-column graph"""
    out = []
    shapes = EGNN_SHAPES + (EGNN_EDGE_ONLY if stage in EDGE_LEVEL else [])
    if duplicate:
        shapes = [sh for sh in shapes if sh[0] not in (15, 16) and sh[2] != "one_col"]
    for n, ea, kind in shapes:
        if stage in EDGE_LEVEL:
            combos = [(True, False), (True, True)] + ([(False, True)] if n == 17 else [])
        else:
            combos = [(True, False), (False, False)] + ([(False, True)] if n == 17 else [])
        for with_v, norm in (combos[:2 if stage in EDGE_LEVEL else 1] if duplicate else combos):
            k = ((n,), 0, ea, 0, (), kind, 0, ("egnn", with_v, norm), SILU)
            out += [(k, v) for v in [()] + ([(("det", True),)] if stage == "edge_backward" else [])]
    return out


def act_cases(stage: str):
    """FastEGNN wiring on the generic-activation build: every kind at ACT_SHAPES (the kinked ones at their committed seeds), the
    smooth kinds at the larger shapes too, and the null wiring of NULL_STAGES at the ragged shape"""
    out = []
    for kind in KINDS:
        for i, sh in enumerate(ACT_SHAPES):
            seed = KINK_SEEDS[(kind[0], i, stage)] if kind[0] in KINKED else 0
            k = sh + (seed, FASTEGNN_WIRING, kind)
            out += [(k, v) for v in _variants(stage, k, FASTEGNN_WIRING)]
            if stage in NULL_STAGES and sh[0] == S_RAGGED and kind[0] not in KINKED:
                out.append((k, (("null", True),)))
        if kind[0] not in KINKED:
            out += [(sh + (0, FASTEGNN_WIRING, kind), ()) for sh in ACT_SMOOTH_SHAPES]
    return out


def act_x3_cases(stage: str):
    return [(sh + (0, FASTEGNN_WIRING, kind), ()) for kind, sh in ACT_X3]


def act_sibling_cases(stage: str):
    return [(sh + (0, w, kind), ()) for kind, w, sh in ACT_SIBLINGS if w[0] != "egnn" or stage in EGNN_STAGES]


def wiring_case_id(key, variant) -> str:
    return variant_id(key[:6], variant) + "-" + wiring_tag(key[7], key[8]) + (f"-s{key[6]}" if key[6] else "")


# --------------------------------------------------------------------------
# the magnitude cases (tests/test_gpu_stage_magnitudes.py): the smallest shapes with more than one ticket per weight-gradient consumer and
# ragged tiles.  A key is the full argument tuple of make_case, the profile last
# --------------------------------------------------------------------------
_PER_GRAPH_PROFILES = ("g_ramp_up", "g_ramp_down", "g_rows", "g_far", "f_ramp")
MAG_SHAPES = [       # (shape, wiring, profiles)
    ((S_RAGGED, 3, 2, 1, ALL_FLAGS, "random"), FASTEGNN_WIRING, _PER_GRAPH_PROFILES),
    ((S_MANY, 16, 2, 0, ALL_FLAGS, "random"), FASTEGNN_WIRING, _PER_GRAPH_PROFILES),
    ((S_65, 5, 7, 0, ALL_FLAGS, "deg32_33"), FASTEGNN_WIRING, ("g_rows", "f_ramp")),          # one graph
    ((S_RAGGED, 3, 2, 0, ALL_FLAGS, "random"), RF, _PER_GRAPH_PROFILES),
    (((65,), 0, 7, 0, (), "random"), ("egnn", True, False), ("g_rows",)),
    ((S_RAGGED, 3, 2, 1, ("bf16",), "random"), FASTEGNN_WIRING, ("g_ramp_up",)),
]


def magnitude_keys(stage: str):
    """the make_case keys of one stage: backward profiles on the backward stages (g_rows scales no per-graph operand: not on the per-graph
    stages, which it leaves as they are), the forward profile on the forward stages"""
    out = []
    for sh, wiring, profiles in MAG_SHAPES:
        if wiring[0] == "egnn" and stage not in EGNN_STAGES:
            continue
        for p in profiles:
            if (stage in BACKWARD) != (p in BACKWARD_PROFILES) or (p == "g_rows" and stage in GRAPH_LEVEL):
                continue
            out.append(sh + (0, wiring, SILU, p))
    return out


def magnitude_cases(stage: str):
    return [(k, v) for k in magnitude_keys(stage) for v in [()] + ([(("det", True),)] if stage == "edge_backward" else [])]


def magnitude_case_id(key, variant) -> str:
    return wiring_case_id(key[:9], variant) + "-" + key[9]
