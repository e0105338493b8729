"""-m gpu: the forward-only loss with its running sums on the device (fastegnn_loss_mse_mmd_eval, fastegnn_amd.train.mse_mmd_eval) and
fastegnn_amd.train.evaluate -- the reference's validation epoch, utils/train.py:23-179 with backprop=False.

Values: against tests/eval_ref.py's float64 restatement of utils/train.py:104-165, under the bound the existing loss tests grant the
training loss against fp64 (tests/test_gpu_train_kernels.py, taken over by tests/test_gpu_mmd_sampler.py for the ragged kernel):
|got - fp64| <= LOSS_K u s, s the fp32 sensitivity of the number from the float64 mirror (tests/mmd_sampler_ref.py).  The new kernel
evaluates the same fp32 kernel values and sums them in fp64, so it has nothing the bound does not already pay for; a call advances
acc[0] by B * MSE and acc[1] by B * loss, hence B times the bound, plus the rounding of the fp64 addition itself."""
import json
import os
import subprocess
import sys
import warnings

import numpy as np
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd.train import MMDSampler, augment_edge_attr, evaluate, mse_mmd_eval, mse_mmd_loss
from oracle import fastegnn_ref as R
from tests.eval_ref import acc_step, batch_loss_fp64
from tests.helpers import U32
from tests.mmd_sampler_ref import mse_mmd_ragged_fp64
from tests.test_gpu_properties import _batch, _models
from tests.test_gpu_train_kernels import LOSS_K

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
U64 = 2.0 ** -53


def _problem(sizes, C, seed):
    g = torch.Generator().manual_seed(seed)
    N, B = sum(sizes), len(sizes)
    loc = torch.randn(N, 3, generator=g)
    return loc, torch.randn(B, 3, C, generator=g), loc + 0.1 * torch.randn(N, 3, generator=g), g


def _sample(sizes, S, g):
    """per graph min(S, n) distinct nodes, the rest of the row -1 (what MMDSampler.draw writes) -> (nodes int32 [B,S], count int32 [B])"""
    rows, cnt, off = [], [], 0
    for n in sizes:
        take = min(S, n)
        rows.append(torch.cat([off + torch.randperm(n, generator=g)[:take], torch.full((S - take,), -1, dtype=torch.long)]))
        cnt.append(take)
        off += n
    return torch.stack(rows).to(torch.int32), torch.tensor(cnt, dtype=torch.int32)


def _bounds(loc, vloc, tgt, samp, cnt, sigma, weight):
    """(fp64 mse, fp64 loss, bound on B * mse, bound on B * loss) of one batch"""
    B = vloc.size(0)
    mse, loss = batch_loss_fp64(loc, vloc, tgt, samp, cnt, sigma, weight)
    if samp is None:
        t = mse_mmd_ragged_fp64(loc, vloc, tgt, torch.zeros(B, 1, dtype=torch.long), torch.zeros(B, dtype=torch.long), sigma, weight)
        s_mse = s_loss = float(t["s_mse"])
    else:
        t = mse_mmd_ragged_fp64(loc, vloc, tgt, samp, cnt, sigma, weight)
        # the mirror and the restatement of the reference's loops are the same numbers in float64
        assert abs(float(t["loss"]) - float(loss)) <= 1e-12 * max(1.0, abs(float(loss))) and abs(float(t["mse"]) - float(mse)) <= 1e-13
        s_mse, s_loss = float(t["s_mse"]), float(t["s_loss"])
    return mse, loss, B * LOSS_K * U32 * s_mse, B * LOSS_K * U32 * s_loss


# (graph sizes, C, S, ragged): B = 1, 3, 7; C = 1, 3, 16; S = 1, S = the smallest graph, S beyond it; a one-node graph, an empty one (count 0)
CASES = {
    "equal_B1_C1_S1": ([12], 1, 1, False),
    "equal_B3_C3_Sall": ([10, 10, 10], 3, 10, False),
    "equal_B7_C16_S4": ([6] * 7, 16, 4, False),
    "ragged_B3_C3_S1": ([9, 4, 6], 3, 1, True),
    "ragged_B3_C3_Smin": ([9, 4, 6], 3, 4, True),
    "ragged_B3_C16_Sbeyond": ([9, 4, 6], 16, 6, True),
    "ragged_B7_C3_one_node_and_empty": ([5, 1, 8, 0, 3, 12, 2], 3, 3, True),
    "ragged_B1_C1_S_beyond_N": ([3], 1, 5, True),
    "ragged_B7_C16_more_than_a_wave_of_pairs": ([300, 141, 77, 1, 64, 65, 2], 16, 48, True),
    "no_sample_B3_C3": ([9, 4, 6], 3, None, False),
    "no_sample_B1_C16_many_nodes": ([100003], 16, None, False),      # 300 009 elements: the 16-byte body, the scalar tail, 293 trips per thread
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_eval_kernel_values_vs_fp64(name):
    sizes, C, S, ragged = CASES[name]
    sigma, weight = 1.5, 0.7
    loc, vloc, tgt, g = _problem(sizes, C, 100 + len(name))
    samp = cnt = None
    if S is not None:
        samp, cnt = _sample(sizes, S, g)
        if not ragged:
            assert cnt.tolist() == [S] * len(sizes)
            cnt = None
    B = len(sizes)
    mse, loss, b_mse, b_loss = _bounds(loc, vloc, tgt, samp, cnt, sigma, weight)
    if S is None:
        assert float(loss) == float(mse)
    acc0 = torch.tensor([1.5, -2.25, 4.0], dtype=torch.float64)
    want = acc_step(acc0, B, mse, loss)
    acc = acc0.cuda()
    out = mse_mmd_eval(loc.cuda(), vloc.cuda(), tgt.cuda(), acc, sigma, weight, samp.cuda() if samp is not None else None,
                       cnt.cuda() if cnt is not None else None)
    assert out is acc
    got = acc.cpu()
    err = (got - want).abs()
    tol = [b_mse + 4 * U64 * abs(float(want[0])), b_loss + 4 * U64 * abs(float(want[1]))]
    print(f"eval[{name}]: acc {got.tolist()} fp64 {want.tolist()} err/tol {float(err[0]) / tol[0]:.3f} {float(err[1]) / tol[1]:.3f}")
    assert torch.isfinite(got).all()
    assert float(got[2]) == 4.0 + B                                                # exact
    assert float(err[0]) <= tol[0] and float(err[1]) <= tol[1], (name, err.tolist(), tol)


def test_full_counts_equal_no_counts_bitwise_and_junk_behind_the_count_is_not_read():
    sizes, C, S = [9, 4, 6], 3, 4
    loc, vloc, tgt, g = _problem(sizes, C, 7)
    samp, cnt = _sample(sizes, S, g)
    args = (loc.cuda(), vloc.cuda(), tgt.cuda())
    a = mse_mmd_eval(*args, torch.zeros(3, dtype=torch.float64, device="cuda"), 1.5, 1.0, samp.cuda(), None)
    b = mse_mmd_eval(*args, torch.zeros(3, dtype=torch.float64, device="cuda"), 1.5, 1.0, samp.cuda(), cnt.cuda())
    assert torch.equal(a, b)
    sizes = [9, 2, 6]
    loc, vloc, tgt, g = _problem(sizes, C, 8)
    samp, cnt = _sample(sizes, S, g)
    junk = samp.clone()
    junk[1, 2:] = 2 ** 30
    args = (loc.cuda(), vloc.cuda(), tgt.cuda())
    a = mse_mmd_eval(*args, torch.zeros(3, dtype=torch.float64, device="cuda"), 1.5, 1.0, samp.cuda(), cnt.cuda())
    b = mse_mmd_eval(*args, torch.zeros(3, dtype=torch.float64, device="cuda"), 1.5, 1.0, junk.cuda(), cnt.cuda())
    assert torch.equal(a, b)


def test_two_runs_are_bit_identical_and_no_graph_leaves_acc_alone():
    sizes, C, S = [300, 141, 77, 1, 64], 16, 48
    loc, vloc, tgt, g = _problem(sizes, C, 21)
    samp, cnt = _sample(sizes, S, g)
    dev = [t.cuda() for t in (loc, vloc, tgt)]
    acc0 = torch.tensor([0.125, 3.0, 2.0], dtype=torch.float64)
    runs = []
    for _ in range(2):
        acc = acc0.cuda()
        for _ in range(3):                                                         # three advances from the same start
            mse_mmd_eval(*dev, acc, 1.5, 0.7, samp.cuda(), cnt.cuda())
        runs.append(acc.cpu())
    assert torch.equal(runs[0], runs[1]) and float(runs[0][2]) == 2.0 + 15
    # B == 0: nothing is launched, acc keeps its bits
    acc = acc0.cuda()
    empty = torch.zeros(0, 3, device="cuda")
    mse_mmd_eval(empty, torch.zeros(0, 3, C, device="cuda"), empty, acc, 1.5, 0.7, torch.zeros(0, S, dtype=torch.int32, device="cuda"),
                 torch.zeros(0, dtype=torch.int32, device="cuda"))
    mse_mmd_eval(empty, 0, empty, acc, 1.5, 0.7)
    assert torch.equal(acc.cpu(), acc0)


def test_invalid_arguments_are_refused_before_any_launch():
    L = K.lib()
    f = L.fastegnn_loss_mse_mmd_eval
    buf = torch.zeros(64, device="cuda")
    idx = torch.zeros(64, dtype=torch.int32, device="cuda")
    acc0 = torch.tensor([1.0, 2.0, 3.0], dtype=torch.float64)
    acc = acc0.cuda()
    p, i, a = K.ptr(buf), K.ptr(idx), K.ptr(acc)
    for what, args in (("null acc", (p, p, p, i, i, 4, 2, 2, 2, 1.0, 1.0, None, None)),
                       ("negative N", (p, p, p, i, i, -1, 2, 2, 2, 1.0, 1.0, a, None)),
                       ("negative B", (p, p, p, i, i, 4, -2, 2, 2, 1.0, 1.0, a, None)),
                       ("negative C", (p, p, p, i, i, 4, 2, -1, 2, 1.0, 1.0, a, None)),
                       ("negative S", (p, p, p, i, i, 4, 2, 2, -3, 1.0, 1.0, a, None)),
                       ("S > 4096", (p, p, p, i, i, 4, 2, 2, 4097, 1.0, 1.0, a, None)),
                       ("null loc_pred", (None, p, p, i, i, 4, 2, 2, 2, 1.0, 1.0, a, None))):
        assert f(*args) == -1, what                                                # FASTEGNN_E_INVALID
        assert b"loss_mse_mmd_eval" in L.fastegnn_last_error(), what
    torch.cuda.synchronize()
    assert torch.equal(acc.cpu(), acc0)
    with pytest.raises(ValueError):
        mse_mmd_eval(buf[:12].view(4, 3), 2, buf[:12].view(4, 3), torch.zeros(3, device="cuda"), 1.0, 1.0)      # acc must be float64


# ----------------------------------------------------------------------------------------------------------------------
# evaluate()
# ----------------------------------------------------------------------------------------------------------------------
def _loader(C, seed):
    """five ragged batches with 3 / 1 / 4 / 2 / 5 graphs, the collated dicts train_step takes (edge_attr of width 1: the model's second
    edge feature is the edge length evaluate() appends)"""
    out = []
    for i, sizes in enumerate(([20, 7, 13], [31], [5, 9, 2, 16], [12, 12], [3, 8, 21, 4, 10])):
        inp = _batch(sizes, 4, C, seed=seed + i, ea=1)
        g = torch.Generator().manual_seed(seed + 50 + i)
        loc_t = inp["node_loc"] + 0.3 * inp["node_vel"] + 0.05 * torch.randn(inp["node_loc"].shape, generator=g)
        data = dict(loc_0=inp["node_loc"], vel_0=inp["node_vel"], loc_t=loc_t, node_feat=inp["node_feat"], edge_index=inp["edge_index"],
                    edge_attr=inp["edge_attr"], batch=inp["data_batch"], loc_mean=inp["loc_mean"],
                    ptr=torch.tensor(np.cumsum([0] + sizes), dtype=torch.int64))
        out.append({k: v.cuda() for k, v in data.items()})
    return out


def _plain_loop(m, loader, sigma, weight, sampler, S):
    """the loop a caller writes today: one .item() per batch (utils/train.py:104-108) -> (mse, loss, bound on mse, bound on loss)"""
    tot_mse = tot_loss = tol_mse = tol_loss = 0.0
    graphs = 0
    with torch.no_grad():
        for data in loader:
            ea = augment_edge_attr(data["edge_attr"], data["loc_0"], data["edge_index"])
            loc, vloc = m(node_loc=data["loc_0"], node_vel=data["vel_0"], node_attr=None, node_feat=data["node_feat"],
                          edge_index=data["edge_index"], loc_mean=data["loc_mean"], data_batch=data["batch"], edge_attr=ea)
            nodes, count = sampler.draw(data["ptr"], min(S, data["loc_0"].size(0)))
            loss, mse = mse_mmd_loss(loc, vloc, data["loc_t"], nodes, sigma, weight, sample_count=count)
            B = vloc.size(0)
            tot_mse += mse.item() * B
            tot_loss += loss.item() * B
            graphs += B
            t = mse_mmd_ragged_fp64(loc, vloc, data["loc_t"], nodes, count, sigma, weight)
            tol_mse += B * LOSS_K * U32 * float(t["s_mse"])
            tol_loss += B * LOSS_K * U32 * float(t["s_loss"])
    return tot_mse / graphs, tot_loss / graphs, tol_mse / graphs, tol_loss / graphs, graphs


def test_evaluate_equals_the_plain_loop_with_one_synchronisation():
    C, S, sigma, weight, seed = 3, 9, 1.5, 0.3, 0xE7A1
    cfg = R.Config(2, 0, 2, 64, C, n_layers=2)
    _, m = _models(cfg, 17)
    loader = _loader(C, 300)
    mse, loss, tol_mse, tol_loss, graphs = _plain_loop(m, loader, sigma, weight, MMDSampler(seed), S)
    assert graphs == 15
    m.train()
    r = evaluate(m, loader, sigma, weight)                          # no sampler: the MMD term is skipped
    assert m.training                                               # the previous mode is back
    print(f"evaluate: mse {r['mse']:.9g} loop {mse:.9g} (bound {tol_mse:.3g})")
    assert r["graphs"] == 15 and r["loss"] == r["mse"]
    assert abs(r["mse"] - mse) <= tol_mse, (r, mse, tol_mse)
    m.eval()
    r2 = evaluate(m, loader, sigma, weight, sampler=MMDSampler(seed), num_sample=S)      # the same draws as the loop's sampler
    assert not m.training
    print(f"evaluate: loss {r2['loss']:.9g} loop {loss:.9g} (bound {tol_loss:.3g})")
    assert abs(r2["mse"] - mse) <= tol_mse and abs(r2["loss"] - loss) <= tol_loss, (r2, mse, loss)
    assert r2["loss"] != r2["mse"]
    with pytest.raises(ValueError):
        evaluate(m, loader, sigma, weight, sampler=MMDSampler(seed))
    # exactly one synchronisation, after the last batch: torch reports every synchronising call in this mode
    smp = MMDSampler(seed)
    evaluate(m, loader, sigma, weight, sampler=smp, num_sample=S)   # (warm: the sampler's buffers of every (B, S) are not kept, the graphs are)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("warn")
    try:
        with warnings.catch_warnings(record=True) as seen:
            warnings.simplefilter("always")
            r3 = evaluate(m, loader, sigma, weight)
    finally:
        torch.cuda.set_sync_debug_mode("default")
    syncs = [str(w.message) for w in seen if "synchroniz" in str(w.message).lower()]
    assert len(syncs) == 1, syncs
    assert r3 == r or abs(r3["mse"] - r["mse"]) <= tol_mse
    assert evaluate(m, [], sigma, weight)["graphs"] == 0


def test_evaluate_runs_the_egnn_branch():
    """utils/train.py:66-68: EGNN takes (x, h, edge_index, edge_fea, v) and has no MMD term"""
    import fastegnn_amd
    torch.manual_seed(9)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
    loader = _loader(3, 400)[:2]
    r = evaluate(m, loader, 1.5, 0.3)
    tot = bound = n = 0
    with torch.no_grad():
        for data in loader:
            ea = augment_edge_attr(data["edge_attr"], data["loc_0"], data["edge_index"])
            x = m(x=data["loc_0"], h=data["node_feat"], edge_index=data["edge_index"], edge_fea=ea, v=data["vel_0"])[0]
            B = data["ptr"].numel() - 1
            mse = batch_loss_fp64(x, None, data["loc_t"], None, None, 1.5, 0.3)[0].item()
            tot += mse * B
            # this forward and evaluate()'s are two runs of one input: each within the output bar (1e-5 of max |x|) of the reference, and
            # outputs e apart move a mean of squares by at most 2 e sqrt(mse) + e^2
            e = 2e-5 * float(x.abs().max())
            bound += (2 * e * mse ** 0.5 + e * e) * B
            n += B
    assert r["graphs"] == n == 4 and r["loss"] == r["mse"]
    assert abs(r["mse"] - tot / n) <= bound / n, (r, tot / n, bound / n)


def test_evaluate_switches_to_the_wide_range_build_and_reruns():
    """tests/wide_range_runner.py's construction (hidden features of ~1e5 on the f16x2 build) in a fresh process: evaluate() warns once,
    returns the numbers of the wide-range build, and they are the oracle's"""
    env = {k: v for k, v in os.environ.items() if k not in ("FASTEGNN_WIDE_RANGE", "FASTEGNN_RANGE_CHECK")}
    r = subprocess.run([sys.executable, "-m", "tests.evaluate_range_runner", "3e5"], cwd=ROOT, env=env, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    b = json.loads([l for l in r.stdout.splitlines() if l.startswith("{")][-1])
    print(b)
    assert b["lib"] == "libfastegnn_hip.so" and not b["wide_before"] and b["wide"] and b["warned"] == 1, b
    assert b["finite"] and b["ref_finite"] and b["graphs"] == 2 * b["B"] and b["training_restored"], b
    assert b["err_loc"] < 1e-4, b                                   # tests/test_gpu_wide_range.py's bound on the outputs at this scale
    assert abs(b["mse"] - b["ref_mse"]) <= b["mse_bound"], b        # ... carried through the mean of squares (the runner derives it)
    assert b["loss"] == b["mse"]
    assert b["passes"] == 2                                         # the loader ran once more, once
