"""-m gpu: the wide-range builds (libfastegnn_hip_x3.so / libfastegnn_hip_act_x3.so: three-part bf16 products, no log2(e) fold) under the
comparisons the suite holds the default f16x2 build to -- the same functions, shapes, case names and tolerances, in this process.

A module runs on the build its RangeGuard names on every call (spec.wide = guard.wide -> K.lib(act=..., wide=True)), and setting
`m._range.wide = True` before the first call is what RangeGuard.switch() does after an overflow; the product itself loads both libraries into one
process on a fallback.  The model factories of the other test files are wrapped (monkeypatch) so that they hand out such a module, and the
existing test functions are called as they are: `_check_vs_oracle` takes its case name from the calling function, so every comparison falls under
the rows of helpers.GRAD_EXCEPTIONS of its f16x2 twin.  Nothing is granted to the build: three-part bf16 carries more mantissa than two-part fp16.

What differs from the default build on these shapes (csrc): virt_fwd_kernel in its one-wave form with three image parts; the bf16x3 consumers of
edge_bwd_pc_kernel / virt_bwd_pc_kernel on the row-major bf16 images; virt_bwd_gv_kernel + the producer / consumer kernel at every size (the
channel-phased form never runs); unfolded weights and P / Q in natural units; and the LDS rings of the producer / consumer virtual backward, which
the 27 648-byte images leave at 4 + 2 slots up to C = 16 and 3 + 2 from C = 32 (f16x2: 5 + 4 / 5 + 3 / 5 + 2) -- DESIGN.md section 6d.

Every test ends with the three statements of `_X3.finish`: the modules are still wide, no fallback warning was raised (the build was chosen, not
fallen back to), and the library that ran reports no f16 operands.

The oracle comparisons reuse the inputs of tests/test_gpu_properties.py byte for byte: behind that file in one session (the alphabetical order) the
session's oracle cache (FASTEGNN_ORACLE_CACHE, keyed on those bytes) serves the checker's side; run alone, every comparison costs one CPU oracle
evaluation (fp32 + fp64) -- a few seconds of CPU for each of the two many-tiles cases, no GPU time.
"""
import contextlib
import ctypes as C
import warnings

import pytest
import torch

from fastegnn_amd import _lib as K
from oracle import fastegnn_ref as R
from tests import gpu_util as U
from tests import test_gpu_egnn as EG
from tests import test_gpu_fastrf as RF
from tests import test_gpu_last_layer_skip as S
from tests import test_gpu_parity as PAR
from tests import test_gpu_properties as P
from tests.helpers import golden_names, rel_err
from tests.test_egnn_oracle_cpu import EGNN_NAMES

pytestmark = pytest.mark.gpu

# the factories as their files define them (kept here so that a wrapper never wraps a wrapper)
_MODELS, _FROM_GOLDEN, _EGNN_OF_GOLDEN, _SKIP_MODEL = P._models, U.model_from_golden, EG._egnn_of_golden, S._model


class _X3:
    """the modules the wrapped factories handed out during one test, and the stage-level backends built for them"""

    def __init__(self, deterministic=None):
        self.made, self.backends, self.deterministic = [], [], deterministic

    def widen(self, m):
        m._range.wide = True          # RangeGuard.switch(), without the overflow that leads to it
        if self.deterministic is not None:
            m.deterministic = self.deterministic
        self.made.append(m)
        return m

    @staticmethod
    def specs(m):
        return [s for s in (getattr(m, "_spec", None), getattr(m, "_spec_det", None)) if s is not None]

    def forms(self):
        """the edge-backward form every module that ran took: 'csc' (col-keyed ordered sum) or 'atomic' (fp32 atomic scatter)"""
        out = set()
        for m in self.made:
            if m._spec is not None:
                out.add("csc" if m._spec.flags & K.F_DETERMINISTIC or m._spec_det is not None else "atomic")
        return out

    def finish(self, seen):
        ran = [m for m in self.made if self.specs(m)]
        assert ran, "no wrapped factory built a module that ran"
        for m in self.made:
            assert m._range.wide and not m._range.warned
        assert not [str(w.message) for w in seen if issubclass(w.category, RuntimeWarning) and "wide-range" in str(w.message)]
        for m in ran:
            assert any(s.wide for s in self.specs(m))                           # spec.wide: the build of the last call through that spec
            act = self.specs(m)[0].act_kind != K.ACT_SILU
            assert K.lib_path(act, True) in K._libs                             # loaded by a call, not by this statement
            assert K.lib(act, wide=True).fastegnn_f16_operands() == 0


@contextlib.contextmanager
def _x3(monkeypatch, deterministic=None):
    ran = _X3(deterministic)

    def models(*a, **k):
        p, m = _MODELS(*a, **k)
        return p, ran.widen(m)

    def from_golden(*a, **k):
        return ran.widen(_FROM_GOLDEN(*a, **k))

    def skip_model(*a, **k):
        cfg, m = _SKIP_MODEL(*a, **k)
        return cfg, ran.widen(m)

    monkeypatch.setattr(P, "_models", models)
    for mod in (U, PAR, RF):
        monkeypatch.setattr(mod, "model_from_golden", from_golden)
    monkeypatch.setattr(EG, "_egnn_of_golden", lambda g: ran.widen(_EGNN_OF_GOLDEN(g)))
    monkeypatch.setattr(S, "_model", skip_model)
    with warnings.catch_warnings(record=True) as seen:
        warnings.simplefilter("always")
        yield ran
    ran.finish(seen)


# ---- a. goldens ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", golden_names())
def test_x3_forward_matches_reference_golden(monkeypatch, name):
    with _x3(monkeypatch):
        PAR.test_forward_matches_reference_golden(name)


@pytest.mark.parametrize("name", golden_names())
def test_x3_backward_matches_reference_golden(monkeypatch, name):
    """parameter and input gradients; the act_* goldens run libfastegnn_hip_act_x3.so backward"""
    with _x3(monkeypatch):
        PAR.test_backward_matches_reference_golden(name)


# (the *_h128 goldens and egnn_flat run the unfused wide path, whose objects are the same in all four libraries)
@pytest.mark.parametrize("name", EGNN_NAMES)
def test_x3_egnn_matches_reference_golden(monkeypatch, name):
    with _x3(monkeypatch):
        EG.test_egnn_matches_reference_golden(name)


@pytest.mark.parametrize("name", [n for n in RF.CASES if not n.endswith("_h128")])
def test_x3_fastrf_matches_reference_golden(monkeypatch, name):
    with _x3(monkeypatch):
        RF.test_fastrf_forward_backward_match_reference_golden(name)


# ---- b. oracle comparisons -----------------------------------------------------------------------------------------------------------------
# (id, the test of tests/test_gpu_properties.py, its arguments, the edge-backward form the shape takes: FastEGNN.deterministic_for sends graphs of at
#  most 512 edges to the col-keyed sum, everything else with fp32 operands to the atomic scatter -- the same on both builds)
ORACLE_CASES = [
    ("cfg1", P.test_cfg1_shape_vs_oracle, (), "atomic"),                                    # 100 graphs x 5 nodes: tiles span many graphs
    ("cfg2", P.test_cfg2_shape_vs_oracle, (), "atomic"),                                    # fully connected 4 x 100
    ("ragged_c16", P.test_ragged_c16_gravity_vs_oracle, (), "atomic"),                      # 1 / 130 / 17 / 300: rings 4 + 2, several tiles
    ("c32", P.test_c32_vs_oracle, (), "atomic"),                                            # 257 nodes: the first 3 + 2 shape
    ("c48", P.test_more_than_32_channels_vs_oracle, (48,), "atomic"),                       # 1 033 nodes, 3 + 2
    ("c64", P.test_more_than_32_channels_vs_oracle, (64,), "atomic"),                       # 3 + 2 with three accumulator banks
    ("edge_attr_5_and_0", P.test_wide_edge_attr_and_node_feat_vs_oracle, (), "atomic"),
    ("input_grads_ea2", P.test_input_gradients_vs_oracle, (2, 3, 4), "atomic"),             # attention, node_attr, three layers
    ("input_grads_ea5", P.test_input_gradients_vs_oracle, (5, 2, 16), "atomic"),
    ("input_grads_ea1", P.test_input_gradients_vs_oracle, (1, 0, 3), "atomic"),
    ("hidden32", P.test_narrow_hidden_nf_vs_oracle, (32, 4), "atomic"),                     # padded parameters through the unfolded pack
    ("hidden20", P.test_narrow_hidden_nf_vs_oracle, (20, 3), "atomic"),
    ("coords_sum", P.test_coords_agg_sum_vs_oracle, (), "atomic"),
    ("hub_rows", P.test_hub_rows_and_skewed_degrees_vs_oracle, (), "atomic"),               # uneven producers against the shorter rings
    ("no_edges_isolated", P.test_no_edges_and_isolated_nodes, (), "csc"),
    ("empty_middle_graph", P.test_empty_middle_graph_vs_oracle, (), "csc"),
    ("act_gelu", P.test_other_activations_mid_size_vs_oracle, ("gelu", 0.0), "atomic"),     # act_x3 at 4 000 nodes, the strict rule
    ("act_leaky_relu", P.test_other_activations_mid_size_vs_oracle, ("leaky_relu", 0.2), "atomic"),   # parameter + kink rule
    # the smallest shapes at which every workgroup owns nine tiles, so both walks wrap and one tile is left over: on this build through the
    # one-wave virt_fwd, virt_bwd_gv_kernel and the producer / consumer backward
    ("many_tiles", P.test_many_tiles_per_workgroup_vs_oracle, (), "atomic"),
    ("many_tiles_c3", P.test_many_tiles_odd_channel_counts_vs_oracle, (3,), "atomic"),
]


@pytest.mark.parametrize("fn,args,form", [c[1:] for c in ORACLE_CASES], ids=[c[0] for c in ORACLE_CASES])
def test_x3_vs_oracle(monkeypatch, fn, args, form):
    with _x3(monkeypatch) as ran:
        fn(*args)
        assert ran.forms() == {form}


# ---- c. both forms of the edge backward ----------------------------------------------------------------------------------------------------
def test_x3_ragged_c16_col_keyed_sum_vs_oracle(monkeypatch):
    """the 4 032 edges of test_ragged_c16_gravity_vs_oracle take the atomic scatter by default (above); here deterministic = True sends the same input
    through the per-edge rows + CSC-ordered sum of this build, under the same case name"""
    with _x3(monkeypatch, deterministic=True) as ran:
        P.test_ragged_c16_gravity_vs_oracle()
        assert ran.forms() == {"csc"}


def test_x3_col_keyed_sum_repeats_the_last_layer_edge_gradients(monkeypatch):
    """two deterministic runs on that input: the last layer's edge-stage weight gradients to 1e-5, the bound test_deterministic_backward_matches_atomic_scatter
    holds the default build to at 20 000 nodes (the col-side scatter does not precede them; what is left is the ticket order of the in-workgroup
    weight-gradient sums).  They are not bit for bit on this build either: 8.8e-7 measured on gcl_1.coord_mlp_r.0.weight."""
    with _x3(monkeypatch, deterministic=True) as ran:
        cfg = R.Config(2, 0, 2, 64, 16, n_layers=2, gravity=[0, -1, 0])
        _, m = P._models(cfg, 4)
        inp = P._batch([1, 130, 17, 300], 9, 16, seed=4)
        runs = []
        for _ in range(2):
            for p in m.parameters():
                p.grad = None
            runs.append(P._run_module(m, inp, inp["node_loc"] + 0.5)[2])
        assert ran.forms() == {"csc"}
        for k in ("gcl_1.coord_mlp_r.0.weight", "gcl_1.edge_mlp.2.weight"):
            print(f"x3 deterministic repeat {k}: {rel_err(runs[1][k], runs[0][k]):.3e}")
            assert runs[0][k].abs().max() > 0 and rel_err(runs[1][k], runs[0][k]) < 1e-5, k


# ---- d. last-layer skip --------------------------------------------------------------------------------------------------------------------
def test_x3_last_layer_skip_small_shape_vs_oracle(monkeypatch):
    with _x3(monkeypatch):
        S.test_small_shape_vs_oracle()


@pytest.mark.parametrize("C_,L,att", [(3, 2, False), (3, 1, False), (3, 2, True), (16, 2, False), (5, 2, False)],
                         ids=["C3-L2", "C3-L1", "C3-L2-attention", "C16-L2", "C5-L2"])
def test_x3_small_ragged_batch_skip_on_matches_skip_off(monkeypatch, C_, L, att):
    with _x3(monkeypatch):
        S.test_small_ragged_batch_skip_on_matches_skip_off(C_, L, att, False)


# ---- e. stage-level API --------------------------------------------------------------------------------------------------------------------
def test_x3_stage_level_api_world1_matches_whole_layer_path(monkeypatch):
    """ShardedFastEGNN around a wide module builds HipBackend(wide=True): the staged entry points of libfastegnn_hip_x3.so against its whole-layer
    path at the existing 1e-6 / 1e-5.  The body is the original test's (same is_initialized guard, which also tears the group down); the
    rendezvous port is another one."""
    from fastegnn_amd import sharded
    backend = sharded.HipBackend
    monkeypatch.setenv("MASTER_ADDR", "127.0.0.1")
    monkeypatch.setenv("MASTER_PORT", "29541")
    with _x3(monkeypatch) as ran:
        def recording(dev, act=False, wide=False):
            ran.backends.append((act, wide))
            return backend(dev, act=act, wide=wide)
        monkeypatch.setattr(sharded, "HipBackend", recording)
        P.test_stage_level_api_world1_matches_whole_layer_path()
        assert ran.backends and all(wide for _, wide in ran.backends), ran.backends
    assert not torch.distributed.is_initialized()


# ---- f. the switch is real -----------------------------------------------------------------------------------------------------------------
def _profile(lib):
    """K.profile_collect of one library (every loaded build keeps its own counters)"""
    n = lib.fastegnn_profile_kernels()
    ms, cnt = (C.c_double * n)(), (C.c_int64 * n)()
    K.check(lib.fastegnn_profile_collect(ms, cnt), "fastegnn_profile_collect")
    return {lib.fastegnn_profile_name(i).decode(): int(cnt[i]) for i in range(n) if cnt[i] > 0}


def test_x3_and_f16x2_modules_run_different_arithmetic(monkeypatch):
    """one f16x2 module and one wide module with the same weights on the same input: the outputs agree to 1e-5 and are NOT the same bits"""
    cfg = R.Config(2, 0, 2, 64, 16, n_layers=2, gravity=[0, -1, 0])
    inp = {k: v.cuda() for k, v in P._batch([700, 333], 9, 16, seed=4).items()}
    _, m16 = _MODELS(cfg, 4)
    with _x3(monkeypatch):
        _, m3 = P._models(cfg, 4)
        with torch.no_grad():
            a, b = m16(**inp)[0], m3(**inp)[0]
        assert not m16._range.wide and not m16._spec.wide
        assert all(torch.equal(p, q) for p, q in zip(m16.parameters(), m3.parameters()))
        assert torch.isfinite(a).all() and rel_err(b, a) < 1e-5
        assert not torch.equal(a, b)


def test_x3_runs_the_gv_kernel_where_the_default_build_runs_the_phased_form(monkeypatch):
    """52 000 nodes of the cfg4 shape (3 250 tiles: from here the default build runs the channel-phased virt_bwd_cs_kernel, which has no Gv stage):
    the kernel ids of one forward + backward on either build, finite results, no oracle.  (Like tests/test_gpu_last_layer_skip.py's phased case
    this is about the default switches: FASTEGNN_VIRT_CS=0 in the environment fails the f16x2 half.)"""
    frame = {k: v.cuda() for k, v in P._frame_cpu(52000, 16, 45).items()}
    cfg = R.Config(2, 0, 2, 64, 16, n_layers=2, gravity=[0, -1, 0])
    _, m16 = _MODELS(cfg, 45)
    prof = {}
    with _x3(monkeypatch):
        _, m3 = P._models(cfg, 45)
        for tag, m in (("f16x2", m16), ("x3", m3)):
            lib = K.lib(wide=m._range.wide)
            lib.fastegnn_profile_enable(1)
            _profile(lib)
            try:
                loc, vloc = m(**frame)
                P._loss(loc, vloc, frame["node_loc"] + 0.5).backward()
                torch.cuda.synchronize()
                prof[tag] = _profile(lib)
            finally:
                lib.fastegnn_profile_enable(0)
            assert torch.isfinite(loc).all() and torch.isfinite(vloc).all()
            assert all(torch.isfinite(p.grad).all() for p in m.parameters() if p.grad is not None)
    assert prof["x3"].get("virt_bwd_gv_kernel", 0) >= 1 and prof["x3"].get("virt_bwd_kernel", 0) == 2, prof["x3"]
    assert "virt_bwd_gv_kernel" not in prof["f16x2"] and prof["f16x2"].get("virt_bwd_kernel", 0) == 2, prof["f16x2"]
