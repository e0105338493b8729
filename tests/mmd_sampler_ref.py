"""Mirrors for the device-side MMD sample (fastegnn_mmd_sample) and the ragged MMD loss (fastegnn_loss_mse_mmd_ragged).

perm_ref / sample_ref: the permutation of include/fastegnn_hip.h ("the device-side MMD sample"), integer for integer, in NumPy
uint64 arithmetic (wrapping products and sums, 32-bit values masked after every product).  They broadcast over `counter` and `j`,
so that the statistics of tests/test_mmd_sampler_cpu.py evaluate 20 000 draws in one call.

mse_mmd_ragged_fp64: tests.helpers.mse_mmd_fp64 with a per-graph sample count -- the same float64 evaluation and the same
per-element sensitivities s_*, over the valid entries of each row only; l_rv keeps its divisor B * S * C (utils/train.py:142).
"""
import math

import numpy as np
import torch

from tests.helpers import U32

_U = np.uint64
GOLDEN = _U(0x9E3779B97F4A7C15)
ROUNDS = 8
_M32 = _U(0xFFFFFFFF)


def mix64(x):
    """splitmix64's output function of x + GOLDEN (uint64, wrapping)"""
    with np.errstate(over="ignore"):
        z = np.asarray(x, dtype=_U) + GOLDEN
        z = (z ^ (z >> _U(30))) * _U(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> _U(27))) * _U(0x94D049BB133111EB)
        return z ^ (z >> _U(31))


def mix32(x):
    """multiply-xorshift mixer on 32-bit values (held in uint64, masked after each product)"""
    x = np.asarray(x, dtype=_U) & _M32
    x = x ^ (x >> _U(16))
    x = (x * _U(0x7FEB352D)) & _M32
    x = x ^ (x >> _U(15))
    x = (x * _U(0x846CA68B)) & _M32
    return x ^ (x >> _U(16))


def perm_bits(n):
    """k = max(2, ceil(log2 n)) rounded up to even: the Feistel network permutes [0, 2^k), 2^k < 4 n for n >= 2"""
    k = max(2, (int(n) - 1).bit_length())
    return k + (k & 1)


def round_keys(seed, counter, b):
    """-> ROUNDS uint64 keys (arrays over `counter`): key_r = mix64(g + r), g = mix64(mix64(mix64(seed) ^ counter) ^ b)"""
    with np.errstate(over="ignore"):
        g = mix64(mix64(mix64(_U(int(seed) & 0xFFFFFFFFFFFFFFFF)) ^ np.asarray(counter, dtype=_U)) ^ _U(int(b)))
        return [mix64(g + _U(r)) for r in range(ROUNDS)]


def perm_ref(seed, counter, b, n, j):
    """perm_b(j) of draw `counter`: `counter` and `j` broadcast (Python ints or integer arrays) -> uint64 array, every value < n"""
    n = int(n)
    counter = np.asarray(counter).astype(_U)
    x = np.asarray(j).astype(_U)
    assert n >= 1 and (x < _U(n)).all()
    half = _U(perm_bits(n) // 2)
    mask = (_U(1) << half) - _U(1)
    keys = round_keys(seed, counter, b)
    x, _ = np.broadcast_arrays(x, keys[0])
    x = x.copy()
    walking = np.ones(x.shape, dtype=bool)
    while walking.any():          # cycle walking: at most 2^k - n + 1 passes, the walk stays on the cycle of its start (< n)
        y = x
        for key in keys:
            L, R = y >> half, y & mask
            F = (mix32((R ^ key) & _M32) ^ (key >> _U(32))) & mask
            y = (R << half) | (L ^ F)
        x = np.where(walking, y, x)
        walking &= x >= _U(n)
    return x


def sample_ref(ptr, S, seed, counter):
    """-> (sample_nodes int32 [B,S], sample_count int32 [B]) of fastegnn_mmd_sample for one draw (torch, CPU)"""
    ptr = [int(v) for v in torch.as_tensor(ptr).cpu().tolist()]
    B = len(ptr) - 1
    nodes = np.full((B, S), -1, dtype=np.int64)
    count = np.zeros(B, dtype=np.int64)
    for b in range(B):
        n = ptr[b + 1] - ptr[b]
        cnt = min(S, n)
        count[b] = cnt
        if cnt == 0:
            continue
        j = np.arange(cnt)
        nodes[b, :cnt] = ptr[b] + (j if n <= S else perm_ref(seed, int(counter), b, n, j).astype(np.int64))
    return torch.from_numpy(nodes).to(torch.int32), torch.from_numpy(count).to(torch.int32)


def mse_mmd_ragged_fp64(loc_pred, vloc, loc_t, sample_nodes, sample_count, sigma, weight):
    """tests.helpers.mse_mmd_fp64 where row b of sample_nodes [B,S] holds sample_count[b] <= S valid entries (the rest is not
    read): l_rv = 2 sum_b sum_{s < count_b} sum_c k(R_bs, V_bc) / (B S C).  Same dict of values and sensitivities."""
    dt = torch.float64
    x, tgt = loc_pred.detach().to(dt).cpu(), loc_t.detach().to(dt).cpu()
    V = vloc.detach().to(dt).cpu().permute(0, 2, 1)                  # [B,C,3]
    samp = sample_nodes.detach().cpu().long()
    B, C = V.shape[0], V.shape[1]
    S, N = samp.size(1), x.size(0)
    cnt = torch.full((B,), S, dtype=torch.long) if sample_count is None else sample_count.detach().cpu().long()
    valid = torch.arange(S)[None, :] < cnt[:, None]                  # [B,S]
    vf = valid.to(dt)
    i2s = 1.0 / (2.0 * sigma * sigma)
    d = x - tgt
    mse = (d * d).sum() / (3 * N)
    g_loc = 2.0 * d / (3 * N)
    s_loc = 4.0 * g_loc.abs()
    s_loss = mse * (4.0 + math.sqrt(3 * N))
    loss = mse.clone()
    g_vloc = torch.zeros(B, C, 3, dtype=dt)
    a_vloc, n_vloc = torch.zeros(B, C, 3, dtype=dt), torch.zeros(B, C, 3, dtype=dt)
    sv_vloc = torch.zeros(B, C, 3, dtype=dt)

    def pairs(X, w, rows):
        """terms of w * sum_{a,c} k(X_a, V_c) over the rows a with rows[b,a] = 1: value, gradient on X [B,P,3] and on V"""
        diff = X[:, :, None, :] - V[:, None, :, :]                   # [B,P,C,3]
        dist = diff.pow(2).sum(-1).sqrt()
        arg = dist * i2s
        k = torch.exp(-arg) * rows[:, :, None]
        f = torch.where(dist > 0, -w * k * i2s / torch.where(dist > 0, dist, torch.ones_like(dist)), torch.zeros_like(dist))
        t = f[..., None] * diff
        lost = lambda a: a + (a < 2.0 ** -100).to(dt) * a / U32                      # noqa: E731
        ta, tw = t.abs(), lost(t.abs() * (4.0 + arg[..., None]))
        return ((w * k).sum(), lost((w * k).abs().mul(4.0 + arg)).sum(), (w * k).abs().sum(), int(rows.sum()) * C,
                t.sum(2), ta.sum(2), tw.sum(2), -t.sum(1), ta.sum(1), tw.sum(1))

    terms = [(V, weight / (B * C * C), None, torch.ones(B, C, dtype=dt))]
    if S and B:
        idx = torch.where(valid, samp, torch.zeros_like(samp))       # the entries past the count are never used as indices
        terms.append((x[idx.reshape(-1)].reshape(B, S, 3), -2.0 * weight / (B * S * C), idx, vf))
    for X, w, idx, rows in terms:
        val, sw_val, sa_val, n_val, gX, aX, swX, gV, aV, swV = pairs(X, w, rows)
        loss = loss + val
        s_loss = s_loss + sw_val + math.sqrt(n_val) * sa_val
        g_vloc += gV; a_vloc += aV; sv_vloc += swV
        if idx is None:                                               # l_vv: both ends are virtual nodes
            n_vloc += C
            g_vloc += gX; a_vloc += aX; sv_vloc += swX; n_vloc += C
        else:
            n_vloc += cnt.to(dt)[:, None, None]
            flat = idx.reshape(-1)
            n_s = 1.0 + torch.zeros(N, 3, dtype=dt).index_add_(0, flat, (vf.reshape(-1, 1) * float(C)).expand(-1, 3).contiguous())
            a_loc = torch.zeros(N, 3, dtype=dt).index_add_(0, flat, aX.reshape(-1, 3))
            g_loc = g_loc.index_add(0, flat, gX.reshape(-1, 3))
            s_loc = s_loc + torch.zeros(N, 3, dtype=dt).index_add_(0, flat, swX.reshape(-1, 3)) + n_s.sqrt() * a_loc
    s_vloc = sv_vloc + n_vloc.clamp(min=1).sqrt() * a_vloc
    return dict(loss=loss, mse=mse, g_loc=g_loc, g_vloc=g_vloc.permute(0, 2, 1).contiguous(),
                s_loss=s_loss, s_mse=mse * (4.0 + math.sqrt(3 * N)), s_loc=s_loc, s_vloc=s_vloc.permute(0, 2, 1).contiguous())
