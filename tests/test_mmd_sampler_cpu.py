"""CPU: the device-side MMD sample and the ragged loss without a device -- the float64 mirror of the ragged loss against the
rectangular one and against a plain loop; the integer mirror of the permutation (tests/mmd_sampler_ref.py, which the GPU tests
compare the kernel with bit for bit) as a sampler: distinct, in range, and uniform under fixed-seed chi-square statistics next to
torch.randperm's; and the host logic of fastegnn_amd.train around the two new C-ABI calls, on a recording stub of the library."""
import math

import numpy as np
import pytest
import torch

import fastegnn_amd
from fastegnn_amd import _lib as K
from fastegnn_amd import train as T
from tests.helpers import mse_mmd_fp64
from tests.mmd_sampler_ref import mse_mmd_ragged_fp64, perm_bits, perm_ref, sample_ref

NEW_SYMBOLS = ["fastegnn_mmd_sample", "fastegnn_loss_mse_mmd_ragged"]
SEED = 20240229


# ----------------------------------------------------------------------------------------------------------------------
# the fp64 mirror of the ragged loss
# ----------------------------------------------------------------------------------------------------------------------
def _problem(sizes, C, seed):
    g = torch.Generator().manual_seed(seed)
    N, B = sum(sizes), len(sizes)
    loc = torch.randn(N, 3, generator=g)
    return loc, torch.randn(B, 3, C, generator=g), loc + 0.1 * torch.randn(N, 3, generator=g), g


@pytest.mark.parametrize("sizes,C,S", [([20, 30, 25], 4, 7), ([9] * 5, 1, 9)])
def test_ragged_mirror_with_full_counts_is_the_rectangular_mirror(sizes, C, S):
    loc, vloc, tgt, g = _problem(sizes, C, 3)
    off = np.cumsum([0] + sizes)
    samp = torch.stack([off[b] + torch.randperm(n, generator=g)[:S] for b, n in enumerate(sizes)])
    want = mse_mmd_fp64(loc, vloc, tgt, samp, 1.3, 0.7)
    for cnt in (None, torch.full((len(sizes),), S, dtype=torch.int32)):
        got = mse_mmd_ragged_fp64(loc, vloc, tgt, samp, cnt, 1.3, 0.7)
        assert set(got) == set(want)
        for k in want:
            assert torch.equal(got[k], want[k]), k


def test_ragged_mirror_equals_a_plain_loop_over_graphs():
    """utils/train.py:121-142 in the test's own words: per graph all valid rows, sums of kernel values, ONE division by B * S * C"""
    sizes, C, S, sigma, weight = [2, 5, 0, 9, 40], 3, 9, 1.1, 0.6
    loc, vloc, tgt, _ = _problem(sizes, C, 4)
    ptr = torch.tensor(np.cumsum([0] + sizes))
    samp, cnt = sample_ref(ptr, S, SEED, 7)
    assert cnt.tolist() == [2, 5, 0, 9, 9]
    x = loc.double().clone().requires_grad_(True)
    v = vloc.double().clone().requires_grad_(True)
    B = len(sizes)
    l_vv, l_rv = 0.0, 0.0
    for b in range(B):
        Vb = v[b].t()                                            # [C,3]
        rows = x[samp[b, :int(cnt[b])].long()]
        for a in range(C):
            for c in range(C):
                d = (Vb[a] - Vb[c]).pow(2).sum()
                l_vv = l_vv + torch.exp(-(d.sqrt() if float(d.detach()) > 0 else d) / (2 * sigma ** 2))   # zero subgradient at distance 0
        for r in rows:
            for c in range(C):
                l_rv = l_rv + torch.exp(-(r - Vb[c]).pow(2).sum().sqrt() / (2 * sigma ** 2))
    mse = (x - tgt.double()).pow(2).mean()
    loss = mse + weight * (l_vv / B / C / C - 2 * l_rv / B / S / C)
    loss.backward()
    got = mse_mmd_ragged_fp64(loc, vloc, tgt, samp, cnt, sigma, weight)
    rel = lambda a, b: float((a - b).abs().max() / b.abs().max())          # noqa: E731
    assert rel(got["loss"], loss.detach()) <= 1e-12 and rel(got["mse"], mse.detach()) <= 1e-12
    assert rel(got["g_loc"], x.grad) <= 1e-12 and rel(got["g_vloc"], v.grad) <= 1e-12
    # the entries past the count are never read: any value there gives the same result
    junk = samp.clone()
    junk[torch.arange(S)[None, :] >= cnt[:, None]] = 10 ** 6
    again = mse_mmd_ragged_fp64(loc, vloc, tgt, junk, cnt, sigma, weight)
    assert all(torch.equal(again[k], got[k]) for k in got)


# ----------------------------------------------------------------------------------------------------------------------
# the mirror is a sampler
# ----------------------------------------------------------------------------------------------------------------------
NS = [(5, 3), (8, 3), (17, 6), (100, 9), (1000, 48), (3341, 24)]


def test_domain_of_the_network_is_below_4n():
    for n in list(range(1, 70)) + [255, 256, 257, 1023, 1025, 3341, 100000, 2 ** 31 - 1]:
        k = perm_bits(n)
        assert k % 2 == 0 and k >= 2 and 2 ** k >= n and (n < 2 or 2 ** k < 4 * n)


@pytest.mark.parametrize("n,S", NS)
def test_every_draw_is_distinct_and_in_range(n, S):
    draws = perm_ref(SEED, np.arange(300)[:, None], 2, n, np.arange(S)[None, :])
    assert draws.shape == (300, S) and (draws < n).all()
    assert all(len(set(row.tolist())) == S for row in draws)
    full = perm_ref(SEED, 11, 1, n, np.arange(n))                      # the whole permutation: a bijection of [0, n)
    assert sorted(full.tolist()) == list(range(n))


def test_sample_ref_rows():
    """n <= S: nodes 0 .. n-1 in order; n > S: ptr[b] + perm_b(j); -1 behind the count; graphs and draws differ"""
    sizes = [3, 9, 0, 10, 50, 50]
    ptr = np.cumsum([0] + sizes)
    nodes, cnt = sample_ref(torch.tensor(ptr), 9, SEED, 5)
    assert nodes.dtype == torch.int32 and cnt.dtype == torch.int32 and cnt.tolist() == [3, 9, 0, 9, 9, 9]
    assert nodes[0].tolist() == [0, 1, 2] + [-1] * 6 and nodes[1].tolist() == list(range(3, 12)) and nodes[2].tolist() == [-1] * 9
    for b in (3, 4, 5):
        assert nodes[b].tolist() == (ptr[b] + perm_ref(SEED, 5, b, sizes[b], np.arange(9)).astype(np.int64)).tolist()
        assert ptr[b] <= int(nodes[b].min()) and int(nodes[b].max()) < ptr[b + 1]
    assert (nodes[4] - 22).tolist() != (nodes[5] - 72).tolist()          # same size, another graph: another permutation
    assert not torch.equal(nodes, sample_ref(torch.tensor(ptr), 9, SEED, 6)[0])
    assert not torch.equal(nodes, sample_ref(torch.tensor(ptr), 9, SEED + 1, 5)[0])


def _z(chi2, dof):
    return (chi2 - dof) / math.sqrt(2 * dof)


def _inclusion_z(draws, n, S):
    D = draws.shape[0]
    p = S / n
    c = np.bincount(draws.reshape(-1).astype(np.int64), minlength=n).astype(np.float64)
    # variance of a count under sampling without replacement, D independent draws: D p (1 - p); the counts sum to D S, which
    # the factor (n - 1) / n accounts for
    return _z((n - 1) / n * ((c - D * p) ** 2).sum() / (D * p * (1 - p)), n - 1)


def _cells_z(idx, cells, D, skip=None):
    c = np.bincount(idx.astype(np.int64), minlength=cells).astype(np.float64)
    if skip is not None:
        assert (c[skip] == 0).all()                                      # the diagonal of a pair without replacement
        c = c[~skip]
    e = D / c.size
    return _z(((c - e) ** 2).sum() / e, c.size - 1)


@pytest.mark.parametrize("n,S", NS)
def test_uniformity(n, S):
    """Fixed seed, counters 0 .. D-1: chi-square statistics as z = (chi2 - dof) / sqrt(2 dof), each required within |z| <= 4 -- a
    condition on the permutation, not a measurement (everything here is deterministic).  torch.randperm, the reference's sampler,
    is held to the same bound on the inclusion statistic at the same (n, S, D)."""
    D = 20000 if n <= 100 else 4000
    draws = perm_ref(SEED, np.arange(D)[:, None], 0, n, np.arange(S)[None, :])
    z = {"inclusion": _inclusion_z(draws, n, S), "position0": _cells_z(draws[:, 0], n, D)}
    if n <= 17:
        diag = (np.arange(n * n) // n) == (np.arange(n * n) % n)
        z["pair01"] = _cells_z(draws[:, 0] * np.uint64(n) + draws[:, 1], n * n, D, skip=diag)
        z["consecutive"] = _cells_z(draws[:-1, 0] * np.uint64(n) + draws[1:, 0], n * n, D - 1)
    g = torch.Generator().manual_seed(SEED)
    ref = torch.stack([torch.randperm(n, generator=g)[:S] for _ in range(D)]).numpy()
    z["randperm_inclusion"] = _inclusion_z(ref, n, S)
    print(f"n={n} S={S} D={D}: " + "  ".join(f"{k} z={v:+.2f}" for k, v in z.items()))
    bad = {k: v for k, v in z.items() if not abs(v) <= 4.0}
    assert not bad, bad


# ----------------------------------------------------------------------------------------------------------------------
# host logic on a recording stub of the library
# ----------------------------------------------------------------------------------------------------------------------
class _Recorder:
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        def call(*args):
            self.calls.append((name, args))
            return 0
        return call


@pytest.fixture
def stub(monkeypatch):
    rec = _Recorder()
    monkeypatch.setattr(K, "lib", lambda *a, **k: rec)
    monkeypatch.setattr(T, "_stream", lambda dev: None)
    return rec


def _addr(p):
    return p.value if p is not None else None


def test_loss_without_counts_makes_todays_call(stub):
    loc, vloc, tgt, _ = _problem([6, 6], 3, 5)
    samp = torch.tensor([[0, 1, 2, 3], [6, 7, 8, 9]], dtype=torch.int32)
    T.mse_mmd_loss(loc.requires_grad_(True), vloc, tgt, samp, 1.5, 0.5)
    (name, args), = stub.calls
    assert name == "fastegnn_loss_mse_mmd" and len(args) == 14
    assert _addr(args[3]) == samp.data_ptr()                            # int32 and contiguous: passed as it is, not copied
    assert args[4:10] == (12, 2, 3, 4, 1.5, 0.5)
    stub.calls.clear()
    cnt = torch.tensor([4, 2], dtype=torch.int32)
    loss, _ = T.mse_mmd_loss(loc, vloc, tgt, samp, 1.5, 0.5, sample_count=cnt)
    (name, args), = stub.calls
    assert name == "fastegnn_loss_mse_mmd_ragged" and len(args) == 15
    assert _addr(args[3]) == samp.data_ptr() and _addr(args[4]) == cnt.data_ptr() and args[5:11] == (12, 2, 3, 4, 1.5, 0.5)
    loss.backward()                                                      # seven inputs, seven gradient slots
    with pytest.raises(ValueError, match="sample_count"):
        T.mse_mmd_loss(loc, vloc, tgt, samp, 1.5, 0.5, sample_count=torch.zeros(3, dtype=torch.int32))


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self.w = torch.nn.Parameter(torch.ones(1))

    def forward(self, node_loc, data_batch, **kw):
        B = int(data_batch.max()) + 1
        return node_loc * self.w, torch.zeros(B, 3, 2) * self.w


def _data():
    loc, _, tgt, _ = _problem([6, 6], 2, 6)
    return dict(loc_0=loc, vel_0=loc, loc_t=tgt, node_feat=loc[:, :2], edge_index=torch.tensor([[0, 1], [1, 0]]), edge_attr=None,
                batch=torch.tensor([0] * 6 + [1] * 6), loc_mean=None, ptr=torch.tensor([0, 6, 12]))


def test_train_step_without_a_sampler_makes_todays_calls(stub):
    model = _Model()
    opt = T.FusedAdam(model.parameters())
    samp = torch.tensor([[0, 1, 2], [6, 7, 8]])
    T.train_step(model, opt, _data(), samp, 1.5, 0.5)
    assert [n for n, _ in stub.calls] == ["fastegnn_augment_edge_attr", "fastegnn_loss_mse_mmd", "fastegnn_adam_step_v2"]
    assert len(stub.calls[1][1]) == 14 and stub.calls[1][1][4:8] == (12, 2, 2, 3)
    with pytest.raises(ValueError, match="sampler"):
        T.train_step(model, opt, _data(), None, 1.5, 0.5)


def test_train_step_with_a_sampler_draws_and_takes_the_ragged_loss(stub):
    class _Sampler:
        def draw(self, ptr, S, advance=True):
            self.seen = (ptr, S, advance)
            return torch.zeros(2, S, dtype=torch.int32), torch.full((2,), S, dtype=torch.int32)
    model, smp, data = _Model(), _Sampler(), _data()
    opt = T.FusedAdam(model.parameters())
    with pytest.raises(ValueError, match="num_sample"):
        T.train_step(model, opt, data, None, 1.5, 0.5, sampler=smp)
    stub.calls.clear()
    T.train_step(model, opt, data, None, 1.5, 0.5, sampler=smp, num_sample=40)
    assert smp.seen[0] is data["ptr"] and smp.seen[1] == 12 and smp.seen[2] is True      # min(num_sample, N): utils/train.py:117
    assert [n for n, _ in stub.calls] == ["fastegnn_augment_edge_attr", "fastegnn_loss_mse_mmd_ragged", "fastegnn_adam_step_v2"]
    stub.calls.clear()
    T.train_step(model, opt, data, torch.tensor([[0], [6]]), 1.5, 0.5, sampler=smp)      # explicit samples win: today's call
    assert [n for n, _ in stub.calls][1] == "fastegnn_loss_mse_mmd"


def test_sampler_refuses_the_cpu():
    assert fastegnn_amd.MMDSampler is T.MMDSampler
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.MMDSampler(1, device="cpu")
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        T.MMDSampler.draw(object.__new__(T.MMDSampler), torch.tensor([0, 4, 9]), 3)


def test_new_symbols_are_exported_at_revision_108():
    assert set(NEW_SYMBOLS) <= set(K.EXPORTED) and K.ABI_VERSION == 108
    for act in (False, True):
        for wide in (False, True):
            L = K.lib(act=act, wide=wide)
            assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    # refused on the host, before any launch
    import ctypes as C
    L = K.lib()
    one = C.c_void_p(8)
    assert L.fastegnn_mmd_sample(None, 1, 1, one, 0, one, one, None) == -1 and b"null" in L.fastegnn_last_error()
    assert L.fastegnn_mmd_sample(one, 1, 1, None, 0, one, one, None) == -1
    assert L.fastegnn_mmd_sample(one, 1, 1, one, 0, None, one, None) == -1
    assert L.fastegnn_mmd_sample(one, 1, 1, one, 0, one, None, None) == -1
    assert L.fastegnn_mmd_sample(one, -1, 1, one, 0, one, one, None) == -1
    assert L.fastegnn_mmd_sample(one, 1, -1, one, 0, one, one, None) == -1
    assert L.fastegnn_mmd_sample(one, 1, 4097, one, 0, one, one, None) == -1 and b"4096" in L.fastegnn_last_error()
    assert L.fastegnn_loss_mse_mmd_ragged(one, one, one, one, None, 4, 1, 1, 1, 1.0, 1.0, one, one, one, None) == -1
    assert b"sample_count" in L.fastegnn_last_error()
