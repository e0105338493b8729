"""The stage entry points on operands of MIXED magnitude, on all four shipped libraries, against the fp64 statement of the same stage.

The default build takes every fp32-grade product through 2-part fp16 splits and carries three pieces of dynamic-range machinery for it
(csrc/common.h): the unscaled forward split, a power-of-two scale per 64-value item for gradient operands (vsplit2_scaled) and a sticky
scale per operand stream in the in-workgroup weight-gradient consumers (WgScale: lowered, never raised, the accumulators multiplied by the
ratio).  Under the N(0,1) operands of tests/test_gpu_stages.py every item and every ticket of a stream has the same scale, so a scale taken
from the wrong lanes, a stream scale that is never lowered or a mis-formed lowering factor computes the right number.  Here the operands
are the same draws under the magnitude profiles of tests/stage_harness.py:

  g_ramp_up    upstream gradients x 2^(-12, 0, +12) by graph: later tickets are larger, the lowering branch runs with ratio 2^-12;
  g_ramp_down  the reverse: the scale is set by the first graph, later rows sit 24 binades under it (the low-part residual path);
  g_rows       rows 0 and 15 of every 16-row tile and the last row of every graph x 2^20, row 7 of every tile x 2^-20: neighbouring items of one
               tile differ by 2^20 and 2^40;
  g_far        x 2^(-100, 0, +30) by graph: normal fp32 everywhere, 130 binades between the first tickets of a stream and the last;
  f_ramp       the feature operands of the forward stages x 2^(-6, 0, +3) by graph: an ordinary fp64 comparison, inside the documented range
               of the unscaled forward split (tests/test_stage_magnitudes_cpu.py asserts that).

Same comparison as tests/test_gpu_stages.py (stage_harness.compare under tests.helpers.grad_tolerance, the bf16 rule for the bf16 case, every
backward stage with wgrad_batch NULL and open, guard bands, exact scratch sizes) and, on top of it, every node- and edge-level buffer per
GROUP of rows -- the rows of each graph, and the three row classes of g_rows -- under the same rule: the tolerance of a slice comes from the fp32
CPU evaluation's own error on that slice, so a 2^-12 graph cannot hide behind a 2^+12 one.  tests/test_stage_magnitudes_cpu.py shows that
honest fp32 in another association passes this, and that three scale-bookkeeping mutants pass the unit draw and are reported here.

FASTEGNN_MAG_LEDGER=<file>: the largest err / tolerance per (profile, stage, build) and the slice it occurred on is written there."""
import os

import pytest

from tests import stage_harness as S

pytestmark = pytest.mark.gpu

BUILDS = [(False, False), (True, False), (False, True), (True, True)]      # K.lib(act, wide): default f16x2, _act, _x3, _act_x3
_RUNNERS = {}
if S.LEDGER is None:
    S.LEDGER = []


def _runner(act, wide):
    if (act, wide) not in _RUNNERS:
        _RUNNERS[(act, wide)] = S.HipRunner(act, wide)
    return _RUNNERS[(act, wide)]


def _params():
    return [pytest.param(stage, key, variant, id=f"{stage}-{S.magnitude_case_id(key, variant)}")
            for stage in S.STAGES for key, variant in S.magnitude_cases(stage)]


@pytest.mark.parametrize("act,wide", BUILDS, ids=["f16x2", "act", "x3", "act_x3"])
@pytest.mark.parametrize("stage,key,variant", _params())
def test_stage_against_fp64_on_mixed_magnitudes(stage, key, variant, act, wide):
    rn = _runner(act, wide)
    case = S.make_case(*key)
    kw = dict(variant)
    shared = tuple(p for p in variant if p[0] != "det")                     # det changes the kernels, not the mathematics
    ref32, truth = S.reference(stage, key, shared, rn.pq_scale(case))
    groups = S.groups_of(case)
    bad = []
    for batch in ((False, True) if stage in S.BACKWARD else (False,)):
        got = S.run_stage(rn, stage, case, batch=batch, **kw)
        name = S.case_name(stage, case, ",".join(f"{k}={int(v)}" for k, v in variant + (("batch", batch),)), rn.name)
        bad += [f"[wgrad_batch {'open' if batch else 'NULL'}] {m}" for m in
                S.compare(name, got, ref32, truth, sizes=case.sizes, bf16=case.cfg.bf16, groups=groups)]
    assert not bad, bad


def test_magnitude_ledger():
    """(runs after the stage tests of this file) the largest err / tolerance per profile, stage and build, and the slice it came from"""
    worst = {}
    for case, key, ratio in S.LEDGER:
        if ":mag-" not in case:
            continue
        part = case.split(":")
        group = (part[3][4:], part[1], part[-1])
        if ratio > worst.get(group, (-1.0,))[0]:
            worst[group] = (ratio, key, part[2])
    lines = [f"{p:12s} {st:20s} {b:10s} {r:6.3f}  {k:28s} {c}" for (p, st, b), (r, k, c) in sorted(worst.items())]
    print("\n".join(["largest err / tolerance: profile, stage, build, ratio, slice, shape"] + lines))
    out = os.environ.get("FASTEGNN_MAG_LEDGER")
    if out:
        with open(out, "w") as f:
            f.write("\n".join(lines) + "\n")


def test_no_bounded_wait_gave_up():
    """(runs last in this file) the channel-phased virtual backward's bounded waits: none gave up during the stage tests"""
    from fastegnn_amd import _lib as K
    for act, wide in BUILDS:
        assert K.lib(act, wide).fastegnn_spin_timeouts(1) == 0
