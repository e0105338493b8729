"""The stage entry points under the wirings and activations tests/test_gpu_stages.py does not reach, each stage on its own against the
fp64 statement of the same stage (oracle/factored.py with a wiring and an activation, through tests/stage_harness.py):

  FASTEGNN_F_RF                       all eleven stages, default and wide-range build (stage_harness.RF_MATRIX);
  FASTEGNN_F_EGNN [+ _EGNN_NORM]      the six stages that wiring has, N = 1 .. 681, with and without the velocity head, the clamp engaged with
                                      components exactly on +-100, pairs closer than the normalisation's epsilon and coincident pairs;
  the seven non-SiLU activation kinds FastEGNN wiring on the generic-activation builds, Sigmoid and Softplus (act(0) != 0: a padding lane that
                                      leaks shows) under the sibling wirings too.

Same comparison as tests/test_gpu_stages.py: stage_harness.compare under tests.helpers.grad_tolerance (the bf16 rule for the bf16 case), every
backward stage with wgrad_batch NULL and open, guard bands, exact scratch sizes.  tests/test_stage_harness_cpu.py shows that the references
equal autograd of the three op-for-op oracles and that this comparison reports eleven single-term errors of these branches.

FASTEGNN_STAGE_LEDGER=<file>: the largest err / tolerance per wiring and activation kind, and the buffer it occurred on, is written there."""
import os

import pytest
import torch

from tests import stage_harness as S

pytestmark = pytest.mark.gpu

_RUNNERS = {}
_USED = set()
S.LEDGER = _LEDGER = []


def _runner(act, wide):
    if (act, wide) not in _RUNNERS:
        _RUNNERS[(act, wide)] = S.HipRunner(act, wide)
    _USED.add((act, wide))
    return _RUNNERS[(act, wide)]


def _params(cases, stages=S.STAGES):
    return [pytest.param(stage, key, variant, id=f"{stage}-{S.wiring_case_id(key, variant)}")
            for stage in stages for key, variant in cases(stage)]


def _run(stage, key, variant, act, wide):
    rn = _runner(act, wide)
    case = S.make_case(*key)
    kw = dict(variant)
    shared = tuple(p for p in variant if p[0] != "det")                     # det changes the kernels, not the mathematics
    ref32, truth = S.reference(stage, key, shared, rn.pq_scale(case))
    bad = []
    for batch in ((False, True) if stage in S.BACKWARD else (False,)):
        got = S.run_stage(rn, stage, case, batch=batch, **kw)
        name = S.case_name(stage, case, ",".join(f"{k}={int(v)}" for k, v in variant + (("batch", batch),)), rn.name)
        bad += [f"[wgrad_batch {'open' if batch else 'NULL'}] {m}" for m in
                S.compare(name, got, ref32, truth, sizes=case.sizes, bf16=case.cfg.bf16)]
    assert not bad, bad


@pytest.mark.parametrize("stage,key,variant", _params(S.rf_cases))
def test_rf_stage_against_fp64(stage, key, variant):
    _run(stage, key, variant, False, False)


@pytest.mark.parametrize("stage,key,variant", _params(lambda st: S.rf_cases(st, duplicate=True)))
def test_rf_stage_against_fp64_wide_range_build(stage, key, variant):
    """(without the det / want variants: the file's wall time is held to that of tests/test_gpu_stages.py)"""
    _run(stage, key, variant, False, True)


@pytest.mark.parametrize("stage,key,variant", _params(S.egnn_cases, S.EGNN_STAGES))
def test_egnn_stage_against_fp64(stage, key, variant):
    _run(stage, key, variant, False, False)


@pytest.mark.parametrize("stage,key,variant", _params(lambda st: S.egnn_cases(st, duplicate=True), S.EGNN_STAGES))
def test_egnn_stage_against_fp64_wide_range_build(stage, key, variant):
    """(fewer settings than on the default build: the file's wall time is held to that of tests/test_gpu_stages.py)"""
    _run(stage, key, variant, False, True)


@pytest.mark.parametrize("stage,key,variant", _params(S.act_cases))
def test_activation_stage_against_fp64(stage, key, variant):
    _run(stage, key, variant, True, False)


@pytest.mark.parametrize("stage,key,variant", _params(S.act_x3_cases))
def test_activation_stage_against_fp64_wide_range_build(stage, key, variant):
    _run(stage, key, variant, True, True)


@pytest.mark.parametrize("stage,key,variant", _params(S.act_sibling_cases))
def test_activation_stage_under_sibling_wirings_against_fp64(stage, key, variant):
    _run(stage, key, variant, True, False)


@pytest.mark.parametrize("wiring,key", [("rf", S.RF_MATRIX[1] + (0, S.RF, S.SILU)),
                                        ("egnn", ((17,), 0, 7, 0, (), "random", 0, ("egnn", True, False), S.SILU))])
def test_null_h_out_is_invalid_under_the_sibling_wirings(wiring, key):
    """include/fastegnn_hip.h: a null h_out is FASTEGNN_E_INVALID under FASTEGNN_F_RF / _EGNN, checked before any launch: x_out keeps its fill"""
    rn = _runner(False, False)
    case = S.make_case(*key)
    be, t = rn.be, case.t
    rn.reset()
    spec = rn.spec(case, False)
    params = [rn.put(w) if w is not None else None for w in case.params]
    graph = be.build_graph(rn.put_int(case.edge_index), case.N, case.n_src, case.row_begin, csc=False)
    keys = ("h", "A", "x", "vel", "aggm", "aggx", "svel") + (() if wiring == "egnn" else ("Bc", "Z", "sgrav"))
    b = {k: rn.put(t[k]) for k in keys}
    b.update(batch=rn.put_int(case.batch.to(torch.int32)), wpack=rn.scratch((be.wpack_floats(case.C) + 3) // 4 * 4),
             x_out=rn.new(case.N, 3), npre=rn.new(case.N, S.H))
    if wiring != "egnn":
        b.update(poolX=rn.new(case.B, 3, case.C), poolV=rn.new(case.B, case.C, S.H))
    be.stage("pack_weights", spec, case.N, case.B, graph, dict(wpack=b["wpack"]), params)
    with pytest.raises(RuntimeError, match=r"code -1"):
        be.stage("virt_forward", spec, case.N, case.B, graph, b, params)
    torch.cuda.synchronize()
    for k in ("x_out", "npre") + (() if wiring == "egnn" else ("poolX", "poolV")):
        assert bool((b[k].view(torch.int32) == S.BAND_BITS).all()), f"{k} was written by a call that returned FASTEGNN_E_INVALID"
    rn.check_bands("virt_forward with a null h_out")
    rn.reset()


def test_accuracy_ledger():
    """(runs after the stage tests of this file) the largest err / tolerance per wiring and activation kind, and where it occurred"""
    worst = {}
    for case, key, ratio in _LEDGER:
        tag = case.split(":")[2].split("-")
        if len(tag) < 3:                       # (a case of another file of the session: plain FastEGNN wiring with SiLU)
            continue
        group = "-".join(tag[2:])
        if ratio > worst.get(group, (-1.0,))[0]:
            worst[group] = (ratio, key, case)
    lines = [f"{g:32s} {r:6.3f}  {k:28s} {c}" for g, (r, k, c) in sorted(worst.items())]
    print("\n".join(["largest err / tolerance per wiring-activation group: group, ratio, buffer, case"] + lines))
    out = os.environ.get("FASTEGNN_STAGE_LEDGER")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")
    assert all(r <= 1.0 for r, _, _ in worst.values())


def test_no_bounded_wait_gave_up():
    """(runs last in this file) the channel-phased virtual backward's bounded waits: none gave up during the stage tests"""
    from fastegnn_amd import _lib as K
    for act, wide in sorted(_USED):
        assert K.lib(act, wide).fastegnn_spin_timeouts(1) == 0
