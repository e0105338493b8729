"""Times the three forms of the MSE + MMD loss over the C ABI on one GPU -- the atomic training kernels (fastegnn_loss_mse_mmd / _ragged),
the ordered training loss (fastegnn_loss_mse_mmd_ordered) and the forward-only eval kernel (fastegnn_loss_mse_mmd_eval) -- at the cfg1 shape
(100 graphs of 5 nodes, C = 3, S = 9 with 5 valid entries per row) and the cfg4 shape (N = 100 000, B = 1, C = 16, S = 48): every form
warmed up, then 7 windows of 2 000 calls per form, the forms alternating inside every window set, device events around a window; median,
min and max per call.  The ordered outputs are compared with the atomic ones first.  Then fastegnn_amd.fit()'s epoch (hidden 64, 8 steps
of 100 five-node graphs, capturable FusedAdam, MMDSampler, no evaluation epochs) without and with a checkpoint after every epoch: host
clock around 20 epochs that end in a device synchronise, 4 alternating runs.  Prints what profiles/ordered_loss.txt holds.

    python tools/gpu_ordered_loss_timing.py [output file]
"""
import ctypes as C
import os
import statistics
import sys
import tempfile
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import fastegnn_amd  # noqa: E402
from fastegnn_amd import _lib as K  # noqa: E402
from fastegnn_amd import data as D  # noqa: E402
from fastegnn_amd.train import FusedAdam, MMDSampler  # noqa: E402
from tests.packed_ref import make_frame  # noqa: E402

OUT = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "out", "ordered_loss.txt")
lines = []


def say(s=""):
    print(s, flush=True)
    lines.append(s)


def st():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def loss_forms(name, n, B, Cn, S, counts):
    g = torch.Generator().manual_seed(1)
    N = n * B
    loc, tgt = torch.randn(N, 3, generator=g).cuda(), torch.randn(N, 3, generator=g).cuda()
    vloc = torch.randn(B, 3, Cn, generator=g).cuda()
    k = min(S, n)
    samp = torch.full((B, S), -1, dtype=torch.int32)
    for b in range(B):
        samp[b, :k] = (b * n + torch.randperm(n, generator=g)[:k]).to(torch.int32)
    samp = samp.cuda()
    cnt = torch.full((B,), counts, dtype=torch.int32).cuda() if counts is not None else None
    L = K.lib()
    loss2 = torch.zeros(2, device="cuda")
    g_loc, g_vloc = torch.empty_like(loc), torch.empty_like(vloc)
    ws = torch.empty(int(L.fastegnn_loss_ordered_ws_doubles(N, B)), dtype=torch.float64, device="cuda")
    acc = torch.zeros(3, dtype=torch.float64, device="cuda")
    a = (K.ptr(loc), K.ptr(tgt), K.ptr(vloc), K.ptr(samp))

    def atomic():
        if cnt is None:
            return L.fastegnn_loss_mse_mmd(*a, N, B, Cn, S, 1.0, 0.01, K.ptr(loss2), K.ptr(g_loc), K.ptr(g_vloc), st())
        return L.fastegnn_loss_mse_mmd_ragged(*a, K.ptr(cnt), N, B, Cn, S, 1.0, 0.01, K.ptr(loss2), K.ptr(g_loc), K.ptr(g_vloc), st())

    def ordered():
        return L.fastegnn_loss_mse_mmd_ordered(*a, K.ptr(cnt), N, B, Cn, S, 1.0, 0.01, K.ptr(loss2), K.ptr(g_loc), K.ptr(g_vloc), K.ptr(ws),
                                               ws.numel(), st())

    def evalf():
        return L.fastegnn_loss_mse_mmd_eval(*a, K.ptr(cnt), N, B, Cn, S, 1.0, 0.01, K.ptr(acc), st())
    forms = (("atomic", atomic), ("ordered", ordered), ("eval", evalf))
    calls, repeats = 2000, 7
    for _, f in forms:
        for _ in range(50):
            assert f() == 0
    torch.cuda.synchronize()
    atomic(); ref = (loss2.clone(), g_loc.clone(), g_vloc.clone())
    ordered(); torch.cuda.synchronize()
    say(f"{name}: N={N} B={B} C={Cn} S={S} counts={counts}: ordered vs atomic |d loss| {float((loss2 - ref[0]).abs().max()):.3g} "
        f"max|d g_loc| {float((g_loc - ref[1]).abs().max()):.3g} max|d g_vloc| {float((g_vloc - ref[2]).abs().max()):.3g}")
    t = {k: [] for k, _ in forms}
    for _ in range(repeats):                      # the forms alternate inside every repeat
        for k, f in forms:
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            e1.synchronize()
            t[k].append(e0.elapsed_time(e1) * 1e3 / calls)
    for k, _ in forms:
        v = sorted(t[k])
        say(f"  {k:8s} median {statistics.median(v):7.2f} us per call  (min {v[0]:.2f}, max {v[-1]:.2f}; {repeats} windows of {calls} calls, device events)")
    say(f"  ordered / atomic = {statistics.median(t['ordered']) / statistics.median(t['atomic']):.3f}   "
        f"ordered / eval = {statistics.median(t['ordered']) / statistics.median(t['eval']):.3f}")


def fit_epochs():
    gen = torch.Generator().manual_seed(5)
    ij = torch.tensor([(i, j) for i in range(5) for j in range(5) if i != j], dtype=torch.int64).t().contiguous()
    frames = []
    for _ in range(800):
        f = make_frame(5, 20, 3, 1, gen)
        f.edge_index = ij
        f.edge_attr = (f.loc_0[ij[0]] - f.loc_0[ij[1]]).norm(dim=1, keepdim=True)
        frames.append(f)
    packed = D.PackedDataset(frames, device="cuda")
    torch.manual_seed(11)
    model = fastegnn_amd.FastEGNN(2, 0, 2, 64, 3, device="cuda", n_layers=4)
    opt = FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-12, capturable=True)
    smp = MMDSampler(3)
    stream = D.PackedStream(packed, 100, shuffle=True, seed=1, graphs=model.deterministic_for)
    tmp = tempfile.mkdtemp()
    kw = dict(sampler=smp, num_sample=9, test_interval=10 ** 6)
    fastegnn_amd.fit(model, opt, stream, [], [], 1.0, 0.01, max_epochs=3, **kw)             # warm-up
    epochs = 20
    res = {"no checkpoint": [], "checkpoint every epoch": []}
    for rep in range(4):
        for name in res:
            ck = os.path.join(tmp, f"c{rep}.pt") if name.startswith("checkpoint") else None
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fastegnn_amd.fit(model, opt, stream, [], [], 1.0, 0.01, max_epochs=epochs, checkpoint_path=ck, **kw)
            torch.cuda.synchronize()
            res[name].append((time.perf_counter() - t0) / epochs * 1e3)
    size = os.path.getsize(os.path.join(tmp, "c0.pt"))
    say(f"fit(): FastEGNN hidden 64, 4 layers, C=3; 800 frames of 5 nodes, PackedStream batch 100 (8 steps per epoch), capturable FusedAdam, "
        f"MMDSampler; no evaluation epochs; checkpoint file {size} bytes")
    for name, v in res.items():
        say(f"  {name:24s} median {statistics.median(v):7.2f} ms per epoch  (min {min(v):.2f}, max {max(v):.2f}; 4 alternating runs of {epochs} epochs, host clock around a synchronise)")
    say(f"  a checkpoint per epoch costs {statistics.median(res['checkpoint every epoch']) - statistics.median(res['no checkpoint']):.2f} ms per epoch")


if __name__ == "__main__":
    say("ordered training loss (fastegnn_loss_mse_mmd_ordered) against the atomic kernels and the forward-only eval kernel; one job, one MI355X")
    loss_forms("cfg1", 5, 100, 3, 9, 5)
    loss_forms("cfg4", 100000, 1, 16, 48, None)
    fit_epochs()
    os.makedirs(os.path.dirname(os.path.abspath(OUT)), exist_ok=True)
    with open(OUT, "w") as fh:
        fh.write("\n".join(lines) + "\n")
