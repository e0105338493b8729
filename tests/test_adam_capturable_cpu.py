"""CPU: the host-side contract of the capturable training step -- argument checks that need no device, and the new C-ABI
exports (additive at revision 108: tests/test_abi_cpu.py then checks them against the header and the built libraries)."""
import pytest
import torch

from fastegnn_amd import _lib as K
from fastegnn_amd.train import FusedAdam

NEW_SYMBOLS = ["fastegnn_grad_sqnorm_partials", "fastegnn_grad_sqnorm", "fastegnn_adam_dev_scratch_bytes", "fastegnn_adam_step_dev"]


def test_clipping_needs_the_capturable_path():
    p = [torch.nn.Parameter(torch.zeros(4))]
    with pytest.raises(ValueError, match="capturable"):
        FusedAdam(p, max_grad_norm=1.0)
    with pytest.raises(ValueError, match="capturable"):
        FusedAdam(p).skip_word = 1234
    opt = FusedAdam(p)                       # today's arguments: the host-side path, step counts as a list
    assert not opt.capturable and opt.steps == [0] and opt.lr == 5e-4


def test_new_symbols_are_exported_at_revision_108():
    assert set(NEW_SYMBOLS) <= set(K.EXPORTED) and K.ABI_VERSION == 108
    L = K.lib()
    assert all(hasattr(L, n) for n in NEW_SYMBOLS)
    import ctypes as C
    # host-only size queries: 24 tensors per launch, at most 64 workgroups per tensor, one slot per workgroup
    numel = (C.c_int64 * 30)(*([300000] + [1] * 23 + [4097] + [7] * 5))
    assert L.fastegnn_grad_sqnorm_partials(numel, 30) == 24 * 64 + 6 * 5
    assert L.fastegnn_adam_dev_scratch_bytes(30) == (8 + 2 * 30) * 4
