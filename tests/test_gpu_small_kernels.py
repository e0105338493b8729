"""The prologue / epilogue kernels of the stage backend interface (fastegnn_amd.sharded.HipBackend) and the two helpers of the
range guard, each on its own: fastegnn_build_batch, fastegnn_embed_forward / _backward, fastegnn_virtual_init / _backward,
fastegnn_permute_rows, fastegnn_check_finite, fastegnn_zero_if_flagged.  Index outputs and copies are compared exactly, sums
against fp64 under the project's rule (tests.helpers.grad_check: 2 x the fp32 CPU evaluation's own error + 1e-6); every
buffer a call writes sits between guard bands (tests/stage_harness.py::BandedPool)."""
import ctypes as C
import struct

import pytest
import torch

from fastegnn_amd import _lib as K
from tests.helpers import grad_check
from tests.stage_harness import BandedPool

pytestmark = pytest.mark.gpu
H = 64


def _st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _rnd(g, *shape):
    return torch.randn(*shape, generator=g, dtype=torch.float32)


def _put(pool, v):
    out = pool._alloc(v.numel(), v.dtype).view(v.shape)
    out.copy_(v)
    return out


# ---------------------------------------------------------------- fastegnn_build_batch
@pytest.mark.parametrize("sizes", [[1], [0, 3, 0, 2, 0], [1, 1, 1] + [0] * 9, [0, 0, 5], [4, 0, 0], [1] * 257 + [0] * 43, [100, 157]],
                         ids=["N1", "empty_first_middle_last", "B+1>N", "empty_first", "empty_last", "N257_B300", "two"])
def test_build_batch(sizes):
    B, N = len(sizes), sum(sizes)
    batch = torch.repeat_interleave(torch.arange(B), torch.tensor(sizes))
    ptr = torch.zeros(B + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(torch.tensor(sizes), 0)
    pool = BandedPool()
    b32, gptr = pool._alloc(N, torch.int32), pool._alloc(B + 1, torch.int32)
    b64 = batch.cuda()
    K.check(K.lib().fastegnn_build_batch(K.ptr(b64), N, B, K.ptr(b32), K.ptr(gptr), _st()), "fastegnn_build_batch")
    pool.check_bands("build_batch")
    assert torch.equal(b32.cpu().long(), batch) and torch.equal(gptr.cpu().long(), ptr)


# ---------------------------------------------------------------- embedding_in
@pytest.mark.parametrize("N", [1, 255, 256, 257, 5000])
@pytest.mark.parametrize("nf", [1, 2, 3, 4, 5, 6, 7, 8])
def test_embed_forward_and_backward(nf, N):
    g = torch.Generator().manual_seed(nf * 10007 + N)
    x, W, b, g_h = _rnd(g, N, nf), _rnd(g, H, nf), _rnd(g, H), _rnd(g, N, H)
    gW0, gb0 = _rnd(g, H, nf), _rnd(g, H)
    lib, pool, case, bad = K.lib(), BandedPool(), f"small:embed:nf{nf}:N{N}", []
    d = {k: _put(pool, v) for k, v in dict(x=x, W=W, b=b, g_h=g_h).items()}
    h = pool._alloc(N * H).view(N, H)
    K.check(lib.fastegnn_embed_forward(K.ptr(d["x"]), N, nf, K.ptr(d["W"]), K.ptr(d["b"]), K.ptr(h), _st()), "fastegnn_embed_forward")
    grad_check(case, "h", h.cpu(), x @ W.T + b, x.double() @ W.double().T + b.double(), bad)
    truth = dict(gW=g_h.double().T @ x.double(), gb=g_h.double().sum(0), g_nf=g_h.double() @ W.double())
    ref32 = dict(gW=g_h.T @ x, gb=g_h.sum(0), g_nf=g_h @ W)
    for want_nf in (True, False):
        gW, gb = _put(pool, gW0), _put(pool, gb0)                      # both accumulate (+=): they start from a random value
        g_nf = pool._alloc(N * nf).view(N, nf) if want_nf else None
        K.check(lib.fastegnn_embed_backward(K.ptr(d["x"]), K.ptr(d["g_h"]), N, nf, K.ptr(d["W"]), K.ptr(gW), K.ptr(gb), K.ptr(g_nf), _st()),
                "fastegnn_embed_backward")
        tag = "" if want_nf else "(g_node_feat null)"
        grad_check(case, "gW" + tag, gW.cpu().double() - gW0.double(), ref32["gW"], truth["gW"], bad)
        grad_check(case, "gb" + tag, gb.cpu().double() - gb0.double(), ref32["gb"], truth["gb"], bad)
        if want_nf:
            assert bool(torch.isfinite(g_nf).all())
            grad_check(case, "g_node_feat", g_nf.cpu(), ref32["g_nf"], truth["g_nf"], bad)
    pool.check_bands(case)
    assert bool(torch.isfinite(h).all()) and not bad, bad


# ---------------------------------------------------------------- virtual_node_feat
@pytest.mark.parametrize("B", [1, 7])
@pytest.mark.parametrize("Cn", [1, 3, 64])
def test_virtual_init_and_backward(Cn, B):
    g = torch.Generator().manual_seed(Cn * 31 + B)
    vnf, g_HvT, g0 = _rnd(g, 1, H, Cn), _rnd(g, B, Cn, H), _rnd(g, 1, H, Cn)
    lib, pool, case, bad = K.lib(), BandedPool(), f"small:virtual_init:C{Cn}:B{B}", []
    HvT = pool._alloc(B * Cn * H).view(B, Cn, H)
    K.check(lib.fastegnn_virtual_init(K.ptr(_put(pool, vnf)), B, Cn, K.ptr(HvT), _st()), "fastegnn_virtual_init")
    assert torch.equal(HvT.cpu(), vnf[0].T.unsqueeze(0).expand(B, -1, -1))
    g_vnf = _put(pool, g0)                                                # accumulates
    K.check(lib.fastegnn_virtual_init_backward(K.ptr(_put(pool, g_HvT)), B, Cn, K.ptr(g_vnf), _st()), "fastegnn_virtual_init_backward")
    grad_check(case, "g_vnf", g_vnf.cpu().double() - g0.double(), g_HvT.sum(0).T.unsqueeze(0), g_HvT.double().sum(0).T.unsqueeze(0), bad)
    pool.check_bands(case)
    assert not bad, bad


# ---------------------------------------------------------------- fastegnn_permute_rows
@pytest.mark.parametrize("E", [1, 255, 257])
@pytest.mark.parametrize("width", [1, 2, 7])
def test_permute_rows(width, E):
    g = torch.Generator().manual_seed(width * 1000 + E)
    src, perm = _rnd(g, E, width), torch.randperm(E, generator=g)
    pool = BandedPool()
    out = pool._alloc(E * width).view(E, width)
    d_src, d_perm = src.cuda(), perm.to(torch.int32).cuda()
    K.check(K.lib().fastegnn_permute_rows(K.ptr(d_src), K.ptr(d_perm), E, width, K.ptr(out), _st()), "fastegnn_permute_rows")
    pool.check_bands("permute_rows")
    assert torch.equal(out.cpu(), src[perm])


# ---------------------------------------------------------------- fastegnn_check_finite
def _i32(bits):
    """the int32 that holds the 32-bit pattern `bits`"""
    return struct.unpack("<i", struct.pack("<I", bits))[0]


BAD_VALUES = {"+inf": 0x7F800000, "-inf": 0xFF800000, "qnan": 0x7FC00001, "qnan_neg_payload": 0xFFC12345, "snan": 0x7F800001,
              "snan_big_payload": 0x7FBFFFFF}
FINE_VALUES = {"flt_max": 0x7F7FFFFF, "-flt_max": 0xFF7FFFFF, "denormal_min": 0x00000001, "denormal_max": 0x007FFFFF, "-0": 0x80000000}
N_BIG = 2 * 1024 * 256 * 8 + 3          # more than the grid cap covers in one pass: the stride loop runs, the last elements are a tail


def _check_finite(a, b, word):
    K.check(K.lib().fastegnn_check_finite(K.ptr(a), 0 if a is None else a.numel(), K.ptr(b), 0 if b is None else b.numel(), K.ptr(word), _st()),
            "fastegnn_check_finite")
    torch.cuda.synchronize()
    return int(word.item())


def test_check_finite_flags_every_non_finite_value_at_either_end_of_either_array():
    pool = BandedPool()
    a, b = pool._alloc(N_BIG, torch.int32), pool._alloc(1027, torch.int32)
    fine = torch.tensor([_i32(v) for v in FINE_VALUES.values()], dtype=torch.int32).cuda()
    a.copy_(fine[torch.arange(N_BIG, device="cuda") % fine.numel()])
    b.copy_(fine[torch.arange(1027, device="cuda") % fine.numel()])
    af, bf = a.view(torch.float32), b.view(torch.float32)
    word = pool._alloc(1, torch.int32)
    word.zero_()
    assert _check_finite(af, bf, word) == 0                       # FLT_MAX, denormals and -0 are finite
    assert _check_finite(af, None, word) == 0 and _check_finite(None, bf, word) == 0
    for name, bits in BAD_VALUES.items():
        v = torch.tensor([_i32(bits)], dtype=torch.int32).cuda()
        for arr, other in ((a, bf), (b, af)):
            for pos in (0, arr.numel() - 1):
                keep = arr[pos].clone()
                arr[pos] = v[0]
                word.zero_()
                assert _check_finite(af, bf, word) == 1, (name, pos)
                word.zero_()
                alone = arr.view(torch.float32)
                assert _check_finite(alone, None, word) == 1 and _check_finite(None, alone, word) == 1, (name, pos, "one array")
                word.zero_()
                assert _check_finite(other, None, word) == 0          # the clean array alone: nothing
                arr[pos] = keep
    word.fill_(1)
    assert _check_finite(af, bf, word) == 1                       # a clean call never clears the word
    pool.check_bands("check_finite")


# ---------------------------------------------------------------- fastegnn_zero_if_flagged
@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 1027, 4 * 512 * 256 * 4 + 2])
def test_zero_if_flagged(n):
    lib, pool = K.lib(), BandedPool()
    g = torch.Generator().manual_seed(n)
    buf = pool._alloc(n + 8)                                      # the floats behind the n the call may touch are payload of this test
    src = _rnd(g, n + 8)
    src[::3] = float("nan")
    src_bits = src.view(torch.int32).cuda()
    buf.view(torch.int32).copy_(src_bits)
    word = pool._alloc(1, torch.int32)
    word.zero_()
    K.check(lib.fastegnn_zero_if_flagged(K.ptr(buf), n, K.ptr(word), _st()), "fastegnn_zero_if_flagged")
    torch.cuda.synchronize()
    assert torch.equal(buf.view(torch.int32), src_bits)           # flag 0: bit-identical, NaNs included
    word.fill_(1)
    K.check(lib.fastegnn_zero_if_flagged(K.ptr(buf), n, K.ptr(word), _st()), "fastegnn_zero_if_flagged")
    torch.cuda.synchronize()
    assert not bool(buf.view(torch.int32)[:n].any())              # exactly n floats are +0 ...
    assert torch.equal(buf.view(torch.int32)[n:], src_bits[n:])   # ... and what follows them is untouched
    pool.check_bands(f"zero_if_flagged n={n}")


def test_zero_if_flagged_refuses_an_unaligned_buffer_before_any_launch():
    lib, pool = K.lib(), BandedPool()
    buf = pool._alloc(64)
    buf.fill_(3.0)
    word = pool._alloc(1, torch.int32)
    word.fill_(1)
    for off in (1, 2, 3):
        assert lib.fastegnn_zero_if_flagged(K.ptr(buf[off:]), 8, K.ptr(word), _st()) == -1      # FASTEGNN_E_INVALID
        assert b"aligned" in lib.fastegnn_last_error()
    torch.cuda.synchronize()
    assert bool((buf == 3.0).all())
    pool.check_bands("zero_if_flagged unaligned")
