"""Every stage entry point of the fused layer (fastegnn_node_pre_forward ... fastegnn_node_pre_backward) on its own, on all
four shipped libraries, against the fp64 statement of the same stage (tests/cpu_stage_backend.py through
tests/stage_harness.py): independent random operands, every output buffer compared under the project's rule
err(HIP, fp64) <= GRAD_FACTOR x err(CPU fp32, fp64) + GRAD_FLOOR (tests.helpers.grad_tolerance; the bf16 operand mode under the
rule of tests/test_gpu_bf16.py), per graph slice and per unit, guard bands around every buffer the call can write, scratch
arrays of exactly the sizes the ABI returns.  Every backward stage runs twice: finishing its own weight-gradient jobs
(wgrad_batch == NULL) and queueing them into an open batch, whose operands must be unchanged when it closes.

The shapes and why they are the smallest that matter: stage_harness.MATRIX.  tests/test_stage_harness_cpu.py shows that this
comparison reports each of eleven single-term errors, and that the reference equals autograd of the op-for-op oracle."""
import pytest
import torch

from tests import stage_harness as S

pytestmark = pytest.mark.gpu

BUILDS = [(False, False), (True, False), (False, True), (True, True)]      # K.lib(act, wide): default f16x2, _act, _x3, _act_x3
_RUNNERS = {}


def _runner(act, wide):
    if (act, wide) not in _RUNNERS:
        _RUNNERS[(act, wide)] = S.HipRunner(act, wide)
    return _RUNNERS[(act, wide)]


def _params():
    out = []
    for stage in S.STAGES:
        for key, variant in S.stage_cases(stage):
            out.append(pytest.param(stage, key, variant, id=f"{stage}-{S.variant_id(key, variant)}"))
    return out


@pytest.mark.parametrize("act,wide", BUILDS, ids=["f16x2", "act", "x3", "act_x3"])
@pytest.mark.parametrize("stage,key,variant", _params())
def test_stage_against_fp64(stage, key, variant, act, wide):
    rn = _runner(act, wide)
    case = S.make_case(*key)
    kw = dict(variant)
    shared = tuple(p for p in variant if p[0] != "det")                     # det changes the kernels, not the mathematics
    ref32, truth = S.reference(stage, key + (0,), shared, rn.pq_scale(case))
    bad = []
    for batch in ((False, True) if stage in S.BACKWARD else (False,)):
        got = S.run_stage(rn, stage, case, batch=batch, **kw)
        name = S.case_name(stage, case, ",".join(f"{k}={int(v)}" for k, v in variant + (("batch", batch),)), rn.name)
        bad += [f"[wgrad_batch {'open' if batch else 'NULL'}] {m}" for m in
                S.compare(name, got, ref32, truth, sizes=case.sizes, bf16=case.cfg.bf16)]
    assert not bad, bad


def test_no_bounded_wait_gave_up():
    """(runs last in this file) the channel-phased virtual backward's bounded waits: none gave up during the stage tests"""
    from fastegnn_amd import _lib as K
    for act, wide in BUILDS:
        assert K.lib(act, wide).fastegnn_spin_timeouts(1) == 0
