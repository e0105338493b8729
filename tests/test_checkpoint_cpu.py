"""Resumable training without a GPU: FusedAdam.state_dict / load_state_dict in torch.optim.Adam's layout, the one-file checkpoint
(fastegnn_amd/checkpoint.py: readable with weights_only=True, replaced atomically, generator and RNG state restored), the control
flow of fit() against a direct transcription of the reference's train() (utils/train.py:181-226) with train_epoch / evaluate replaced
by scripted sequences, copies and pickles of a RangeGuard and of the modules, and the new exports of the four libraries."""
import copy
import ctypes as C
import io
import json
import os
import pickle
import re
import warnings

import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import checkpoint as CK
from fastegnn_amd import data as D
from fastegnn_amd.model import RangeGuard
from fastegnn_amd.train import FusedAdam
from tests.packed_ref import TorchCollateOps, ragged_frames

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SHAPES = [(3, 4), (5,), (1,), (2, 3, 2)]


def _params(seed=0):
    g = torch.Generator().manual_seed(seed)
    return [torch.nn.Parameter(torch.randn(*s, generator=g)) for s in SHAPES]


def _torch_adam_after_steps(params, steps=3, skip=2):
    """torch.optim.Adam stepped on the CPU; parameter `skip` never has a gradient, parameter 1 misses the first step"""
    g = torch.Generator().manual_seed(9)
    opt = torch.optim.Adam(params, lr=3e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-2)
    for t in range(steps):
        for i, p in enumerate(params):
            p.grad = None if i == skip or (i == 1 and t == 0) else torch.randn(p.shape, generator=g)
        opt.step()
    return opt


# ---- FusedAdam state ----
def test_state_dict_has_torch_adams_layout():
    params = _params()
    opt = FusedAdam(params, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=1e-2)
    sd = opt.state_dict()
    assert set(sd) == {"state", "param_groups"} and len(sd["param_groups"]) == 1
    group = sd["param_groups"][0]
    assert group["params"] == [0, 1, 2, 3] and sorted(sd["state"]) == [0, 1, 2, 3]
    assert (group["lr"], group["betas"], group["eps"], group["weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 1e-2)
    assert group["capturable"] is False and group["max_grad_norm"] is None
    want = torch.optim.Adam(_params()).state_dict()["param_groups"][0]
    assert set(want) <= set(group)                                    # every key torch's own group has
    for i, p in enumerate(params):
        e = sd["state"][i]
        assert set(e) == {"step", "exp_avg", "exp_avg_sq"}
        assert isinstance(e["step"], torch.Tensor) and e["step"].dim() == 0 and float(e["step"]) == 0.0
        assert e["exp_avg"].shape == p.shape and e["exp_avg_sq"].shape == p.shape
        assert e["exp_avg"].data_ptr() != opt.exp_avg[i].data_ptr()   # copies: a later step does not move a saved state


def test_torch_adam_state_loads_and_round_trips():
    params = _params()
    tadam = _torch_adam_after_steps(params)
    tsd = tadam.state_dict()
    assert sorted(tsd["state"]) == [0, 1, 3]                          # parameter 2 never stepped: no entry
    opt = FusedAdam(params, lr=1.0)
    ptrs = [t.data_ptr() for t in opt.exp_avg + opt.exp_avg_sq]
    opt.exp_avg[2].fill_(5.0)                                         # a missing entry means ZERO state, whatever was there
    opt.load_state_dict(tsd)
    assert ptrs == [t.data_ptr() for t in opt.exp_avg + opt.exp_avg_sq]   # in place
    assert opt.steps == [3, 2, 0, 3]
    assert (opt.lr, opt.betas, opt.eps, opt.weight_decay) == (3e-3, (0.8, 0.99), 1e-7, 1e-2)
    for i in (0, 1, 3):
        assert torch.equal(opt.exp_avg[i], tsd["state"][i]["exp_avg"]) and torch.equal(opt.exp_avg_sq[i], tsd["state"][i]["exp_avg_sq"])
    assert not opt.exp_avg[2].any() and not opt.exp_avg_sq[2].any()
    # round trip through a second FusedAdam: every tensor and every count
    sd = opt.state_dict()
    again = FusedAdam(_params(), lr=7.0)
    again.load_state_dict(sd)
    sd2 = again.state_dict()
    assert sd2["param_groups"] == sd["param_groups"]
    for i in range(4):
        for k in ("step", "exp_avg", "exp_avg_sq"):
            assert torch.equal(sd2["state"][i][k], sd["state"][i][k]), (i, k)
    assert again.steps == opt.steps and again.step_count == opt.step_count


def test_torch_adam_loads_the_fused_state_and_steps_on():
    """the reverse direction: torch.optim.Adam takes FusedAdam's state_dict and its next step is the step of the optimizer the state came from"""
    pa, pb = _params(), _params()
    ta = _torch_adam_after_steps(pa)
    fused = FusedAdam(pa)
    fused.load_state_dict(ta.state_dict())
    with torch.no_grad():
        for a, b in zip(pa, pb):
            b.copy_(a)
    tb = torch.optim.Adam(pb)
    tb.load_state_dict(fused.state_dict())
    g = torch.Generator().manual_seed(3)
    for a, b in zip(pa, pb):
        a.grad = torch.randn(a.shape, generator=g)
        b.grad = a.grad.clone()
    ta.step(); tb.step()
    for i, (a, b) in enumerate(zip(pa, pb)):
        assert torch.equal(a, b), i
        assert float(tb.state[b]["step"]) == float(ta.state[a]["step"])
    assert float(tb.state[pb[2]]["step"]) == 1.0


def test_load_state_dict_refuses_a_wrong_count_or_shape_and_changes_nothing():
    params = _params()
    opt = FusedAdam(params)
    good = _torch_adam_after_steps(_params()).state_dict()
    opt.load_state_dict(good)
    before = [t.clone() for t in opt.exp_avg + opt.exp_avg_sq], list(opt.steps), opt.lr
    fewer = copy.deepcopy(good)
    fewer["param_groups"][0]["params"] = [0, 1, 2]
    with pytest.raises(ValueError, match="3 parameters.*4"):
        opt.load_state_dict(fewer)
    shape = copy.deepcopy(good)
    shape["param_groups"][0]["lr"] = 123.0
    shape["state"][3]["exp_avg_sq"] = torch.zeros(2, 3, 3)
    with pytest.raises(ValueError, match="exp_avg_sq of parameter 3"):
        opt.load_state_dict(shape)
    two = copy.deepcopy(good)
    two["param_groups"].append(copy.deepcopy(two["param_groups"][0]))
    with pytest.raises(ValueError, match="2 parameter groups"):
        opt.load_state_dict(two)
    clip = copy.deepcopy(good)
    clip["param_groups"][0]["max_grad_norm"] = 1.0
    with pytest.raises(ValueError, match="capturable=True"):
        opt.load_state_dict(clip)
    after = [t.clone() for t in opt.exp_avg + opt.exp_avg_sq], list(opt.steps), opt.lr
    assert all(torch.equal(a, b) for a, b in zip(before[0], after[0])) and before[1:] == after[1:]


def test_a_capturable_state_converts_to_the_host_side_optimizer_and_back():
    """on CPU parameters a capturable optimizer keeps its counts on the host until it meets a device: the conversion is the same code"""
    good = _torch_adam_after_steps(_params()).state_dict()
    cap = FusedAdam(_params(), capturable=True, max_grad_norm=2.0)
    cap.load_state_dict(good)                                        # torch's group names no max_grad_norm: the optimizer keeps its own
    assert cap.capturable and cap.max_grad_norm == 2.0 and cap.steps == [3, 2, 0, 3]
    sd = cap.state_dict()
    assert sd["param_groups"][0]["capturable"] is True and sd["param_groups"][0]["max_grad_norm"] == 2.0
    sd["param_groups"][0]["max_grad_norm"] = None
    host = FusedAdam(_params())
    host.load_state_dict(sd)
    assert not host.capturable and host.steps == [3, 2, 0, 3]
    assert all(torch.equal(a, b) for a, b in zip(host.exp_avg + host.exp_avg_sq, cap.exp_avg + cap.exp_avg_sq))


# ---- the checkpoint file ----
def _small():
    torch.manual_seed(1)
    model = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    opt = FusedAdam(model.parameters(), lr=1e-3)
    opt.load_state_dict(_torch_adam_after_steps(list(model.parameters()), skip=-1).state_dict())
    return model, opt


def test_checkpoint_is_read_with_weights_only_and_restores_every_state(tmp_path, monkeypatch):
    monkeypatch.setattr(D, "_COLLATE_OPS", TorchCollateOps)
    frames = ragged_frames(C=3, seed=0)
    packed = D.PackedDataset(frames)

    def loaders(seed):
        return (D.DataLoader(frames, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(seed)),
                D.PackedLoader(packed, batch_size=4, shuffle=True, generator=torch.Generator().manual_seed(seed + 1)),
                D.DataLoader(frames, batch_size=4, shuffle=True),      # no generator of its own: torch's global one
                [1, 2, 3])                                             # no state at all

    def order(loader):
        return [b["loc_0"].clone() for b in loader]
    model, opt = _small()
    lds = loaders(5)
    for ld in lds[:3]:
        order(ld)                                                      # one epoch behind every loader
    path = tmp_path / "run" / "ckpt.pt"
    CK.save_checkpoint(path, model, opt, loaders=lds, extra={"epoch_index": 7, "log_dict": {"loss": [0.5, float("inf")]}})
    want = [order(ld) for ld in lds[:3]]                               # the uninterrupted run's next epoch
    blob = torch.load(path, weights_only=True)
    assert blob["format"] == CK.FORMAT and blob["version"] == CK.FORMAT_VERSION
    assert set(blob) == {"format", "version", "model", "guard", "optimizer", "sampler", "loaders", "rng", "extra"}
    assert blob["guard"] is None and blob["sampler"] is None and blob["loaders"][3] is None and blob["loaders"][2] == {"generator": None}
    assert os.listdir(path.parent) == ["ckpt.pt"]                      # no temporary file left
    # fresh objects, other seeds, the global generator somewhere else
    torch.manual_seed(99)
    model2 = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    opt2 = FusedAdam(model2.parameters(), lr=9.0)
    lds2 = loaders(50)
    extra = CK.load_checkpoint(path, model2, opt2, loaders=lds2)
    assert extra == {"epoch_index": 7, "log_dict": {"loss": [0.5, float("inf")]}}
    for a, b in zip(model.state_dict().values(), model2.state_dict().values()):
        assert torch.equal(a, b)
    assert opt2.steps == opt.steps and opt2.lr == opt.lr
    assert all(torch.equal(a, b) for a, b in zip(opt2.exp_avg + opt2.exp_avg_sq, opt.exp_avg + opt.exp_avg_sq))
    got = [order(ld) for ld in lds2[:3]]
    for w, g_ in zip(want, got):
        assert len(w) == len(g_) and all(torch.equal(a, b) for a, b in zip(w, g_))
    with pytest.raises(ValueError, match="4 loader states"):
        CK.load_checkpoint(path, model2, opt2, loaders=lds2[:2])
    with pytest.raises(ValueError, match="loader 2 was saved with a state"):
        CK.load_checkpoint(path, model2, opt2, loaders=(lds2[0], lds2[1], [1], [2]))


def test_a_failing_writer_leaves_the_old_checkpoint_in_place(tmp_path, monkeypatch):
    model, opt = _small()
    path = tmp_path / "ckpt.pt"
    CK.save_checkpoint(path, model, opt, extra={"epoch_index": 1})
    old = path.read_bytes()
    real = torch.save

    def dies_half_way(obj, f, *a, **k):
        real(obj, f, *a, **k)
        with open(f, "r+b") as fh:
            fh.truncate(100)
        raise OSError("disk full")
    monkeypatch.setattr(torch, "save", dies_half_way)
    with pytest.raises(OSError, match="disk full"):
        CK.save_checkpoint(path, model, opt, extra={"epoch_index": 2})
    monkeypatch.setattr(torch, "save", real)
    assert path.read_bytes() == old and os.listdir(tmp_path) == ["ckpt.pt"]
    assert CK.load_checkpoint(path, model, opt) == {"epoch_index": 1}
    torch.save({"model": {}}, tmp_path / "other.pt")
    with pytest.raises(ValueError, match="not a checkpoint"):
        CK.load_checkpoint(tmp_path / "other.pt", model, opt)


# ---- fit(): the reference's control flow ----
def _reference_train(train, valid, test, early_stop, test_interval, max_epochs):
    """utils/train.py:181-226 transcribed: the epochs' numbers come from the three lists; no files, no clock"""
    log_dict = {'epochs': [], 'loss': [], 'loss_train': []}
    best_log_dict = {'epoch_index': 0, 'loss_valid': 1e8, 'loss_test': 1e8, 'loss_train': 1e8}
    valid, test = iter(valid), iter(test)
    for epoch_index in range(1, max_epochs + 1):
        loss_train = train[epoch_index - 1]
        log_dict['loss_train'].append(loss_train)
        if epoch_index % test_interval == 0:
            loss_valid = next(valid)
            loss_test = next(test)
            log_dict['epochs'].append(epoch_index)
            log_dict['loss'].append(loss_test)
            if loss_valid < best_log_dict['loss_valid']:
                best_log_dict = {'epoch_index': epoch_index, 'loss_valid': loss_valid, 'loss_test': loss_test, 'loss_train': loss_train}
            if epoch_index - best_log_dict['epoch_index'] >= early_stop:
                best_log_dict['early_stop'] = epoch_index
                break
    return best_log_dict, log_dict


class _Script:
    """train_epoch / evaluate replaced by scripted sequences: every call is recorded, `mse` is the logged number and `loss` a decoy"""

    def __init__(self, monkeypatch, train, valid, test):
        self.train, self.evals, self.calls = list(train), {"valid": list(valid), "test": list(test)}, []
        monkeypatch.setattr(CK, "train_epoch", self.train_epoch)
        monkeypatch.setattr(CK, "evaluate", self.evaluate)

    def train_epoch(self, model, optimizer, loader, sigma, weight, *, sampler=None, num_sample=None):
        assert loader == "train" and (sigma, weight, num_sample) == (1.5, 0.25, 6)
        self.calls.append("train")
        return dict(mse=self.train.pop(0), loss=-1.0, graphs=8)

    def evaluate(self, model, loader, sigma, weight, **kw):
        assert (sigma, weight) == (1.5, 0.25) and not kw
        self.calls.append(loader)
        return dict(mse=self.evals[loader].pop(0), loss=-1.0, graphs=8)


TRAIN = [0.9, 0.8, 0.7, 0.6, 0.5, 0.45, 0.4, 0.35, 0.3, 0.25, 0.2, 0.15]
VALID = [0.50, 0.40, 0.40, 0.45, 0.39, 0.60]        # an equal value (third) is NO improvement: the rule is strict
TEST = [0.55, 0.41, 0.30, 0.47, 0.42, 0.61]


def _strip(best):
    return {k: v for k, v in best.items() if k != "time_cost"}


@pytest.mark.parametrize("early_stop,test_interval,max_epochs", [(float("inf"), 2, 12), (4, 2, 12), (2, 2, 12), (1, 1, 6), (float("inf"), 5, 12),
                                                                 (3, 3, 12), (float("inf"), 2, 5)])
def test_fit_follows_the_reference_loop(tmp_path, monkeypatch, early_stop, test_interval, max_epochs):
    script = _Script(monkeypatch, TRAIN, VALID, TEST)
    model, opt = _small()
    log_path, best_path = tmp_path / "logs" / "log.json", tmp_path / "best.pth"
    best, log = fastegnn_amd.fit(model, opt, "train", "valid", "test", 1.5, 0.25, max_epochs=max_epochs, num_sample=6, early_stop=early_stop,
                                 test_interval=test_interval, log_path=log_path, best_path=best_path)
    want_best, want_log = _reference_train(TRAIN, VALID, TEST, early_stop, test_interval, max_epochs)
    assert _strip(best) == want_best and log == want_log
    assert best["time_cost"] >= 0.0
    epochs = len(want_log["loss_train"])
    assert script.calls == [c for e in range(1, epochs + 1) for c in (["train", "valid", "test"] if e % test_interval == 0 else ["train"])]
    on_disk = json.loads(log_path.read_text())
    assert isinstance(on_disk, list) and len(on_disk) == 2
    assert list(on_disk[1]) == ["epochs", "loss", "loss_train"] and on_disk[1] == want_log
    assert set(on_disk[0]) >= {"epoch_index", "loss_valid", "loss_test", "loss_train", "time_cost"} and _strip(on_disk[0]) == want_best
    if want_best["epoch_index"]:
        saved = torch.load(best_path, weights_only=True)
        assert all(torch.equal(a, b) for a, b in zip(saved.values(), model.state_dict().values()))
    else:
        assert not best_path.exists()
    if early_stop == 2:
        assert want_best["epoch_index"] == 4 and want_best["early_stop"] == 6      # the tie at epoch 6 did not reset the count


def test_fit_resumes_at_the_next_epoch_with_the_logs_intact(tmp_path, monkeypatch):
    want_best, want_log = _reference_train(TRAIN, VALID, TEST, 4, 2, 12)
    assert want_best == {"epoch_index": 4, "loss_valid": 0.40, "loss_test": 0.41, "loss_train": 0.6, "early_stop": 8}
    ckpt, log_path = tmp_path / "ckpt.pt", tmp_path / "log.json"
    kw = dict(num_sample=6, early_stop=4, test_interval=2, log_path=log_path, checkpoint_path=ckpt)
    # the first leg ends after epoch 5 (an epoch without evaluation, between two that have one)
    first = _Script(monkeypatch, TRAIN[:5], VALID[:2], TEST[:2])
    model, opt = _small()
    best5, log5 = fastegnn_amd.fit(model, opt, "train", "valid", "test", 1.5, 0.25, max_epochs=5, **kw)
    assert log5["epochs"] == [2, 4] and len(log5["loss_train"]) == 5
    assert torch.load(ckpt, weights_only=True)["extra"]["epoch_index"] == 5
    # fresh objects; the second leg's script starts where the first one ended
    second = _Script(monkeypatch, TRAIN[5:], VALID[2:], TEST[2:])
    torch.manual_seed(123)
    model2 = torch.nn.Sequential(torch.nn.Linear(3, 4), torch.nn.Linear(4, 2))
    opt2 = FusedAdam(model2.parameters(), lr=4.0)
    best, log = fastegnn_amd.fit(model2, opt2, "train", "valid", "test", 1.5, 0.25, max_epochs=12, resume=True, **kw)
    assert second.calls[:3] == ["train", "valid", "test"]              # epoch 6 came first
    assert _strip(best) == want_best and log == want_log
    assert best["time_cost"] >= best5["time_cost"]
    assert opt2.steps == opt.steps and all(torch.equal(a, b) for a, b in zip(model2.state_dict().values(), model.state_dict().values()))
    assert json.loads(log_path.read_text())[1] == want_log
    # a finished (early-stopped) run resumes to nothing: no epoch runs, the logs come back
    third = _Script(monkeypatch, [], [], [])
    best3, log3 = fastegnn_amd.fit(model2, opt2, "train", "valid", "test", 1.5, 0.25, max_epochs=12, resume=True, **kw)
    assert third.calls == [] and _strip(best3) == want_best and log3 == want_log
    # resume=True without a file starts at epoch 1
    fresh = _Script(monkeypatch, TRAIN, VALID, TEST)
    fastegnn_amd.fit(model2, opt2, "train", "valid", "test", 1.5, 0.25, max_epochs=1, resume=True, num_sample=6,
                     checkpoint_path=tmp_path / "none.pt", checkpoint_interval=3)
    assert fresh.calls == ["train"] and (tmp_path / "none.pt").exists()       # the last epoch is always saved


# ---- copies ----
def _guard_with_fake_words():
    g = RangeGuard()
    g._words = (C.c_int32 * 2)(1, 0)       # stands for the host-mapped words (a ctypes object: neither copyable state nor picklable)
    g.wide, g.warned, g.warned_inputs, g.mode, g.launched = True, True, True, "sync", True
    return g


@pytest.mark.parametrize("with_words", [False, True])
def test_range_guard_copies_and_pickles_without_its_words(with_words):
    g = _guard_with_fake_words() if with_words else RangeGuard()
    try:
        for c in (copy.deepcopy(g), copy.copy(g), pickle.loads(pickle.dumps(g))):
            assert c is not g and c._words is None and not c.launched
            assert (c.forced, c.wide, c.mode, c.warned, c.warned_inputs) == (g.forced, g.wide, g.mode, g.warned, g.warned_inputs)
        assert (g._words is not None) == with_words                     # the original keeps its own
    finally:
        g._words = None                                                 # (nothing for __del__ to hand to the library)


def test_range_guard_state_dict_restores_the_build_without_a_warning():
    g = RangeGuard()
    assert g.state_dict() == {"wide": bool(K.WIDE_RANGE)}
    h = RangeGuard()
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        h.load_state_dict({"wide": True})
    if h.forced is not False and not K.SAFE_WAITS:
        assert h.wide and h.state_dict() == {"wide": True} and not h.warned
    h.load_state_dict({"wide": False})                                  # a guard on the wide-range build stays there
    assert h.wide == (h.forced is not False and not K.SAFE_WAITS)


@pytest.mark.parametrize("kind", ["FastEGNN", "FastEGNN_wide", "FastRF", "EGNN", "EGNN_flat"])
def test_modules_copy_and_pickle_with_derived_state_dropped(kind):
    torch.manual_seed(0)
    make = {"FastEGNN": lambda: fastegnn_amd.FastEGNN(2, 0, 2, 64, 3, n_layers=2, gravity=[0.0, -1.0, 0.0]),
            "FastEGNN_wide": lambda: fastegnn_amd.FastEGNN(2, 0, 2, 128, 3, n_layers=2),
            "FastRF": lambda: fastegnn_amd.FastRF(2, 0, 2, 64, 3, n_layers=2),
            "EGNN": lambda: fastegnn_amd.EGNN(2, 2, 2, 64),
            "EGNN_flat": lambda: fastegnn_amd.EGNN(2, 2, 2, 32, flat=True)}[kind]
    m = make()
    m.deterministic = True
    # what a forward leaves behind, faked: words, a spec that names the guard, a parameter list, a cached graph, the wide path's caches
    m._range._words = (C.c_int32 * 2)(0, 0)
    m._spec = type("Spec", (), {"guard": m._range, "table": (C.c_void_p * 2)()})()
    m._plist = list(m.parameters())
    m._graph_cache = {("key",): (C.c_void_p * 2)()}
    m._wide_ordered = (C.c_void_p * 2)()
    m._gravity_dev = (("cpu",), (C.c_void_p * 2)())
    try:
        buf = io.BytesIO()
        torch.save(m, buf)
        buf.seek(0)
        for c in (copy.deepcopy(m), torch.load(buf, weights_only=False)):
            assert type(c) is type(m) and c._range is not m._range and c._range._words is None
            assert c._spec is None and c._plist is None and c._graph_cache == {}
            assert not hasattr(c, "_wide_ordered") and not hasattr(c, "_gravity_dev")
            assert c.deterministic is True
            sa, sb = m.state_dict(), c.state_dict()
            assert list(sa) == list(sb) and all(torch.equal(sa[k], sb[k]) and sa[k].data_ptr() != sb[k].data_ptr() for k in sa)
        assert m._spec is not None and m._plist is not None and m._graph_cache and m._range._words is not None   # the original is untouched
    finally:
        m._range._words = None


# ---- the new exports ----
def test_new_symbols_are_declared_bound_and_exported_by_all_four_libraries():
    src = open(os.path.join(ROOT, "include", "fastegnn_hip.h")).read()
    assert re.search(r"\bsize_t fastegnn_loss_ordered_ws_doubles\(", src) and re.search(r"\bint fastegnn_loss_mse_mmd_ordered\(", src)
    assert K.ABI_VERSION == 108 and "#define FASTEGNN_ABI_VERSION 108" in re.sub(r"[ \t]+", " ", src)
    assert {"fit", "save_checkpoint", "load_checkpoint"} <= set(fastegnn_amd.__all__)
    if K.SAFE_WAITS:    # (that switch loads the diagnostic build only)
        return
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            for name in ("fastegnn_loss_ordered_ws_doubles", "fastegnn_loss_mse_mmd_ordered"):
                assert name in K.EXPORTED and hasattr(L, name), (act, wide, name)
            assert L.fastegnn_loss_ordered_ws_doubles(700, 1) == 3


def test_ordered_loss_rejects_bad_arguments_before_any_launch():
    L = K.lib()
    SOME = C.c_void_p(64)
    f = L.fastegnn_loss_mse_mmd_ordered

    def call(loc=SOME, tgt=SOME, vloc=SOME, samp=SOME, cnt=SOME, N=60, B=3, Cn=5, S=7, loss2=SOME, g_loc=SOME, g_vloc=SOME, ws=SOME,
             ws_doubles=4):
        return f(loc, tgt, vloc, samp, cnt, N, B, Cn, S, 1.0, 0.5, loss2, g_loc, g_vloc, ws, ws_doubles, None)
    for what, kw in (("N < 0", dict(N=-1)), ("B < 0", dict(B=-1)), ("C < 0", dict(Cn=-1)), ("S < 0", dict(S=-1)), ("C > 256", dict(Cn=257)),
                     ("S > 4096", dict(S=4097)), ("null loss2", dict(loss2=None)), ("null ws", dict(ws=None)), ("null loc_pred", dict(loc=None)),
                     ("null loc_t", dict(tgt=None)), ("null vloc", dict(vloc=None)), ("null sample_nodes", dict(samp=None)),
                     ("null g_loc", dict(g_loc=None)), ("null g_vloc", dict(g_vloc=None)), ("ws too small", dict(ws_doubles=3))):
        assert call(**kw) == -1, what                                      # FASTEGNN_E_INVALID
    assert b"workspace too small" in L.fastegnn_last_error()
