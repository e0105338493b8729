"""CPU: the buffer plan of the forward-only path (fastegnn_amd.model.inference_plan) and the recurrence of the
device-side evaluation accumulator (fastegnn_loss_mse_mmd_eval) against the reference's validation epoch.  No GPU."""
import math

import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd.model import PING_PONG, STAGE_SET, _carve, _padded, inference_plan, plan_offsets
from tests.eval_ref import acc_step, batch_loss_fp64

H = K.H
SHAPES = [(20000, 1, 3), (518, 4, 3), (77, 3, 16), (1, 1, 1), (60, 2, 64), (0, 0, 5)]


def _split(shapes):
    stage = {k: v for k, v in shapes.items() if "@" not in k}
    sets = {}
    for k, v in shapes.items():
        if "@" in k:
            name, s = k.split("@")
            sets.setdefault(int(s), {})[name] = v
    return stage, sets


def _floats(group):
    return sum(_padded(s) for s in group.values())


@pytest.mark.parametrize("N,B,C", SHAPES)
@pytest.mark.parametrize("wiring", ["fastegnn", "fastrf", "egnn"])
def test_total_is_one_stage_set_plus_two_ping_pong_sets(N, B, C, wiring):
    if wiring == "egnn":
        B, C = 1, 0
    totals = set()
    for L in (2, 3, 4, 7):
        shapes, total = inference_plan(N, B, C, L, wiring)
        stage, sets = _split(shapes)
        assert sorted(sets) == [0, 1] and sets[0] == sets[1]
        assert total == _floats(stage) + 2 * _floats(sets[0])
        assert set(stage) <= set(STAGE_SET) and set(sets[0]) <= set(PING_PONG)
        totals.add((total, tuple(shapes.items())))
    assert len(totals) == 1                                   # independent of n_layers from 2 layers on
    shapes, _ = inference_plan(N, B, C, 4, wiring)
    stage, sets = _split(shapes)
    # the shapes the layer descriptor documents (include/fastegnn_hip.h)
    assert stage["P"] == stage["A"] == stage["aggm"] == stage["npre"] == sets[0]["h"] == (N, H)
    assert stage["QX"] == (N, K.QX_LD) and stage["aggx"] == sets[0]["x"] == (N, 3) and stage["svel"] == (N,)
    if wiring != "egnn":
        assert stage["Bc"] == stage["poolV"] == sets[0]["HvT"] == (B, C, H)
        assert stage["poolX"] == sets[0]["Z"] == (B, 3, C) and stage["xsum"] == (B, 4) and stage["sgrav"] == (N,)


@pytest.mark.parametrize("N,B,C", SHAPES)
@pytest.mark.parametrize("L", [0, 1, 2, 5])
@pytest.mark.parametrize("wiring", ["fastegnn", "fastrf", "egnn"])
def test_every_slice_is_16_byte_aligned_and_inside_the_total(N, B, C, L, wiring):
    if wiring == "egnn":
        B, C = 1, 0
    shapes, total = inference_plan(N, B, C, L, wiring)
    off = plan_offsets(shapes)
    end = 0
    for k, s in shapes.items():
        assert off[k] % 4 == 0 and off[k] >= end, k          # offsets in floats: a multiple of 4 is 16 bytes; no overlap
        end = off[k] + math.prod(s)
    assert end <= total
    # the allocation the model carves follows the same layout
    views = _carve(torch.device("cpu"), shapes)
    base = min(v.data_ptr() for v in views.values()) if views else 0
    for k, v in views.items():
        assert tuple(v.shape) == tuple(shapes[k]) and v.data_ptr() - base == 4 * off[k], k
        assert v.numel() == 0 or v.data_ptr() % 16 == 0, k


def test_wirings_plan_only_what_their_kernels_take():
    N, B, C = 300, 3, 4
    egnn, _ = inference_plan(N, 1, 0, 4, "egnn")
    stage, sets = _split(egnn)
    # FASTEGNN_F_EGNN: no virtual nodes -- no pools over them, no Bc / xsum / sgrav, no Z / HvT; its node_net does take npre
    assert set(stage) == {"P", "QX", "A", "svel", "aggm", "aggx", "npre"} and set(sets[0]) == {"h", "x"}
    # a FastEGNN whose only layer is the last one: the node update is dead, npre / poolV stay null, nothing is handed to a next layer
    one, total_one = inference_plan(N, B, C, 1, "fastegnn")
    stage, sets = _split(one)
    assert "npre" not in stage and "poolV" not in stage and sorted(sets) == [0]
    four, total_four = inference_plan(N, B, C, 4, "fastegnn")
    assert total_four - total_one == _padded((N, H)) + _padded((B, C, H)) + _floats(_split(four)[1][1])
    # ... unless the diagnostic switch keeps the dead update
    kept, _ = inference_plan(N, B, C, 1, "fastegnn", dead_last=False)
    assert "npre" in kept and "poolV" in kept and "h@1" in kept
    # FASTEGNN_F_RF: node_mlp is absent, but fastegnn_virt_forward requires npre / poolV / h_out under this wiring (csrc/layer_fwd.hip),
    # and the last layer passes h / Hv on: a single layer already writes the second set
    rf, _ = inference_plan(N, B, C, 1, "fastrf")
    assert "npre" in rf and "poolV" in rf and "h@1" in rf and "HvT@1" in rf
    with pytest.raises(ValueError):
        inference_plan(N, B, C, 2, "wide")
    with pytest.raises(ValueError):
        inference_plan(-1, B, C, 2)


def test_accumulator_recurrence_is_the_reference_epoch_average():
    """three batches of different graph counts: acc[0] / acc[2] is utils/train.py:107-108,179's result['loss'] / result['counter'],
    acc[1] / acc[2] the same average of the full objective, acc[2] the graph count; without a sample both averages agree"""
    g = torch.Generator().manual_seed(3)
    sigma, weight, C, S = 1.5, 0.3, 3, 4
    result = {"loss": 0.0, "counter": 0.0}
    full = 0.0
    acc = torch.zeros(3, dtype=torch.float64)
    acc_plain = torch.zeros(3, dtype=torch.float64)
    for sizes in ([5, 9, 2], [7], [3, 3, 3, 3, 11]):
        n_graphs, N = len(sizes), sum(sizes)
        pred = torch.randn(N, 3, generator=g, dtype=torch.float64)
        tgt = pred + 0.1 * torch.randn(N, 3, generator=g, dtype=torch.float64)
        vloc = torch.randn(n_graphs, 3, C, generator=g, dtype=torch.float64)
        off, rows, cnt = 0, [], []
        for n in sizes:
            take = min(S, n)
            rows.append(torch.cat([off + torch.randperm(n, generator=g)[:take], torch.full((S - take,), -1)]))
            cnt.append(take)
            off += n
        samp, cnt = torch.stack(rows), torch.tensor(cnt)
        mse, loss = batch_loss_fp64(pred, vloc, tgt, samp, cnt, sigma, weight)
        assert float(mse) == float(torch.nn.functional.mse_loss(pred, tgt)) and float(loss) != float(mse)
        result["loss"] += mse.item() * n_graphs                              # utils/train.py:107
        result["counter"] += n_graphs                                        # :108
        full += loss.item() * n_graphs
        acc = acc_step(acc, n_graphs, mse, loss)
        plain = batch_loss_fp64(pred, vloc, tgt, None, None, sigma, weight)
        acc_plain = acc_step(acc_plain, n_graphs, *plain)
    assert acc[2].item() == result["counter"] == 9
    assert abs(acc[0].item() / acc[2].item() - result["loss"] / result["counter"]) <= 4 * 2.0 ** -53 * result["loss"] / result["counter"]
    assert abs(acc[1].item() / acc[2].item() - full / result["counter"]) <= 4 * 2.0 ** -53 * abs(full) / result["counter"]
    assert torch.equal(acc_plain[0], acc_plain[1]) and torch.equal(acc_plain[0], acc[0])
