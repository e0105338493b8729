"""Kernel-trace target for the packed loader's two kernels at the Water-3D-like batch of tools/gpu_loader_timing.py (the sizes
only: 20 frames of 7600..8400 nodes and 139 000 random edges each, one batch of all 20): PackedDataset.batch 23 times, then a
torch copy_ of the same bytes 23 times as the plain-copy yardstick.  profiles/packed_loader_kernel_trace.txt holds the
per-launch durations of

    rocprofv3 --kernel-trace --stats --output-format csv -d <dir> -o gather -- python tools/gpu_loader_trace.py
"""
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastegnn_amd import data as D  # noqa: E402

gen = torch.Generator().manual_seed(3)
frames = []
for n in torch.randint(7600, 8401, (20,), generator=gen).tolist():
    e = 139000
    r = lambda *s: torch.rand(*s, generator=gen)  # noqa: E731
    frames.append(D.Frame(torch.randint(0, n, (2, e), generator=gen), r(e, 1), r(n, 3), r(n, 3), r(n, 3), r(n, 2), r(n, 1),
                          r(1, 3, 3)).to("cuda"))
packed = D.PackedDataset(frames)
ids = torch.randperm(20, generator=gen)
for _ in range(23):
    b = packed.batch(ids)
nbytes = sum(b[k].numel() * b[k].element_size() for k in b.keys())
src = torch.rand(nbytes // 4, device="cuda")
dst = torch.empty_like(src)
for _ in range(23):
    dst.copy_(src)
torch.cuda.synchronize()
print("bytes one way", nbytes)
