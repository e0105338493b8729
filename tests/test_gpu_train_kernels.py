"""-m gpu: the four kernels of the training-step closure (csrc/train.hip: augment_edge_attr, loss_mse + loss_mmd, adam) and
fastegnn_amd.train.train_step against float64 evaluations of the same operations, at the shapes the product trains at
(cfg1 / cfg2 / cfg4, the entry point's C = 256 / S = 4096 ceiling) and at their quiet edges (coincident points, underflowing
kernel values, coordinates far from the origin, repeated samples, 200 Adam steps, gradient-less steps).

Tolerances.  Loss and its gradients: the repo's rule (tests/helpers.py grad_check: 2 x the fp32 torch reference's own error
+ a floor) on every tensor, and per element |got - fp64| <= LOSS_K u s, s the element's fp32 sensitivity from
tests/helpers.py mse_mmd_fp64 (the absolute sum of its terms, weighted by what an fp32 evaluation of each can lose), so that
an element that is well-conditioned is held to a few ulp of itself, not to the largest element of its tensor.  Adam: one
step from the same fp32 state (the fp64 optimizer re-synchronised to the kernel's parameters and moments before every step)
within a few ulp of every result, and the free-running fp64 optimizer within the rounding that accumulates over the run.
With FASTEGNN_TOL_DUMP=<file> every per-element comparison is logged (as grad_check's are) and nothing fails."""
import json
import math
import os

import pytest
import torch

from fastegnn_amd.train import FusedAdam, augment_edge_attr, mse_mmd_loss, train_step
from oracle import fastegnn_ref as R
from tests.helpers import U32, grad_check, mse_mmd_fp64
from tests.test_gpu_properties import _batch, _models

pytestmark = pytest.mark.gpu

_DUMP = os.environ.get("FASTEGNN_TOL_DUMP")

# per-element loss bound |got - fp64| <= LOSS_K * u * s (tests/helpers.py mse_mmd_fp64): s is a first-order bound already
# (each term's own roundings, sqrt(n) for an n-term fp32 sum in arbitrary order), so LOSS_K stays at the order of 1.  Worst
# err / (u s) measured on an MI355X: g_vloc 1.26 (sigma = 0.05, underflow; one run with the 2^-100 rule of mse_mmd_fp64),
# g_loc 0.58 / 0.73 over two runs (C = 256, S = 4096), every other case and the loss / MSE words <= 0.51
LOSS_K = 2.0


def _elementwise(case, name, got, truth, sens, k, bad, floor=0.0):
    got = torch.as_tensor(got).detach().double().cpu()
    err = (got - truth).abs()
    assert torch.isfinite(got).all(), f"{case} {name}: non-finite"
    tol = k * U32 * sens + floor
    ratio = float((err / (U32 * sens).clamp(min=1e-300)).max()) if err.numel() else 0.0
    if _DUMP:
        with open(_DUMP, "a") as f:
            f.write(json.dumps({"case": case, "tensor": name, "elementwise_ratio": ratio, "k": k,
                                "worst_abs": float(err.max()) if err.numel() else 0.0}) + "\n")
        return
    if (err > tol).any():
        i = int((err - tol).argmax())
        bad.append(f"{name}: {int((err > tol).sum())} elements beyond {k} u s, worst err/(u s) {ratio:.2f} "
                   f"(element {i}: got {got.reshape(-1)[i].item():.9g} fp64 {truth.reshape(-1)[i].item():.9g})")


def _samples(sizes, S, g, repeat=False):
    out, off = [], 0
    for n in sizes:
        idx = torch.randint(0, n, (S,), generator=g) if repeat else torch.randperm(n, generator=g)[:S]
        out.append(idx + off)
        off += n
    return torch.stack(out) if out else torch.zeros(0, S, dtype=torch.long)


def _check_loss(case, loc, vloc, tgt, samp, sigma, weight, ref32=True):
    """HIP loss + gradients vs the fp64 mirror (per element) and vs the fp32 oracle (grad_check)"""
    a, v = loc.cuda().requires_grad_(True), vloc.cuda().requires_grad_(True)
    l, mse = mse_mmd_loss(a, v, tgt.cuda(), samp.cuda(), sigma, weight)
    l.backward()
    t = mse_mmd_fp64(loc, vloc, tgt, samp, sigma, weight)
    bad = []
    _elementwise(case, "loss", l.detach(), t["loss"], t["s_loss"], LOSS_K, bad)
    _elementwise(case, "mse", mse.detach(), t["mse"], t["s_mse"], LOSS_K, bad)
    _elementwise(case, "g_loc", a.grad, t["g_loc"], t["s_loc"], LOSS_K, bad)
    _elementwise(case, "g_vloc", v.grad, t["g_vloc"], t["s_vloc"], LOSS_K, bad)
    if ref32:
        a32, v32 = loc.clone().requires_grad_(True), vloc.clone().requires_grad_(True)
        l32, mse32 = R.loss_mse_mmd_nodes(a32, v32, tgt, samp, sigma, weight)
        l32.backward()
        grad_check(case, "loss", l.detach().reshape(1), l32.detach().reshape(1), t["loss"].reshape(1), bad)
        grad_check(case, "g_loc", a.grad, a32.grad, t["g_loc"], bad)
        grad_check(case, "g_vloc", v.grad, v32.grad, t["g_vloc"], bad)
    assert not bad, (case, bad)
    return a.grad.cpu(), v.grad.cpu()


# (graph sizes, C, S, sigma, weight, coordinate scale)
LOSS_SHAPES = {
    "cfg1": ([5] * 100, 3, 5, 1.0, 1.0, 1.0),               # 100 graphs x 5 nodes, every node sampled
    "cfg2": ([100] * 100, 3, 9, 1.5, 1.0, 1.0),             # 100 MMD workgroups, sample = 3 C
    "cfg4": ([100000], 16, 48, 1.0, 1.0, 1.0),              # the 1024-block cap of the MSE grid (300 000 elements)
    "C256_S768": ([6000], 256, 768, 1.5, 1.0, 2.0),         # sample = 3 C at the entry point's largest C
    "C256_S4096": ([6000, 4100], 256, 4096, 1.5, 1.0, 2.0),  # the ceiling: (6 C + 6 S) * 4 = 104 448 B of LDS per workgroup
    "C1": ([40, 17, 64], 1, 6, 1.0, 1.0, 1.0),
}


@pytest.mark.parametrize("name", sorted(LOSS_SHAPES))
def test_loss_shapes_vs_fp64(name):
    sizes, C, S, sigma, weight, scale = LOSS_SHAPES[name]
    g = torch.Generator().manual_seed(len(name) + C + S)
    N, B = sum(sizes), len(sizes)
    loc = torch.randn(N, 3, generator=g) * scale
    tgt = loc + 0.1 * torch.randn(N, 3, generator=g)
    vloc = torch.randn(B, 3, C, generator=g) * scale
    _check_loss(f"loss_{name}", loc, vloc, tgt, _samples(sizes, S, g), sigma, weight)


def test_loss_without_samples_has_no_nan():
    """S = 0 (the entry point allows it): l_rv is an empty sum, and its weight -2 w / (B S C) is never applied"""
    g = torch.Generator().manual_seed(5)
    loc, tgt, vloc = torch.randn(30, 3, generator=g), torch.randn(30, 3, generator=g), torch.randn(3, 3, 4, generator=g)
    _check_loss("loss_S0", loc, vloc, tgt, torch.zeros(3, 0, dtype=torch.long), 1.0, 1.0, ref32=False)


def test_loss_coincident_points_take_the_zero_subgradient():
    """Two coincident virtual nodes, and sampled real nodes placed exactly on a virtual node: those pairs have dist = 0 and
    contribute nothing to either gradient (torch.cdist's backward); nothing is NaN"""
    g = torch.Generator().manual_seed(11)
    sizes, C, S = [20, 20], 4, 5
    loc, tgt = torch.randn(40, 3, generator=g), torch.randn(40, 3, generator=g)
    vloc = torch.randn(2, 3, C, generator=g)
    vloc[0, :, 1] = vloc[0, :, 0]
    vloc[1, :, 3] = vloc[1, :, 2]
    samp = _samples(sizes, S, g)
    loc[samp[0, 0]] = vloc[0, :, 0]
    loc[samp[1, 2]] = vloc[1, :, 3]
    _check_loss("loss_coincident", loc, vloc, tgt, samp, 1.0, 1.0)
    # a graph whose every pair coincides: both MMD gradients are exactly zero
    v1 = torch.randn(1, 3, 1, generator=g).repeat(1, 1, 2)
    l1 = torch.randn(6, 3, generator=g)
    l1[2] = v1[0, :, 0]
    a, v = l1.cuda().requires_grad_(True), v1.cuda().requires_grad_(True)
    mse_mmd_loss(a, v, l1.cuda(), torch.tensor([[2, 2]]).cuda(), 1.0, 1.0)[0].backward()
    assert torch.equal(v.grad.cpu(), torch.zeros_like(v1)) and torch.equal(a.grad.cpu(), torch.zeros_like(l1))


def test_loss_repeated_samples():
    """the same node sampled twice (and three times) in one graph: both draws add their gradient to that node"""
    g = torch.Generator().manual_seed(12)
    sizes = [8, 8, 8]
    loc, tgt, vloc = torch.randn(24, 3, generator=g), torch.randn(24, 3, generator=g), torch.randn(3, 3, 3, generator=g)
    samp = torch.tensor([[1, 1, 5, 1], [8, 9, 9, 15], [16, 17, 18, 19]])
    _check_loss("loss_repeated", loc, vloc, tgt, samp, 1.0, 1.0)
    _check_loss("loss_repeated_random", loc, vloc, tgt, _samples(sizes, 12, g, repeat=True), 1.0, 1.0)


def test_loss_underflowing_kernel_values():
    """sigma = 0.05 on unit-scale coordinates: exp(-d / 0.005) underflows for most pairs"""
    g = torch.Generator().manual_seed(13)
    sizes, C, S = [50] * 4, 6, 18
    loc, vloc = torch.randn(200, 3, generator=g), torch.randn(4, 3, C, generator=g)
    vloc[:, :, 1] = vloc[:, :, 0] + 0.002                       # a few pairs stay in range
    tgt = loc + 0.1 * torch.randn(200, 3, generator=g)
    samp = _samples(sizes, S, g)
    loc[samp[:, 0]] = vloc[:, :, 0] + 0.003
    _check_loss("loss_underflow", loc, vloc, tgt, samp, 0.05, 1.0)


@pytest.mark.parametrize("offset", [1e3, -2.5e3])
def test_loss_far_from_origin(offset):
    """coordinates 1e3 from the origin: the kernel subtracts before it squares, and the MMD part dominates the loss
    (weight 50) so that its error is not hidden under the MSE's"""
    g = torch.Generator().manual_seed(14)
    sizes, C, S = [64] * 3, 5, 15
    loc = torch.randn(192, 3, generator=g) + offset
    tgt = loc + 1e-3 * torch.randn(192, 3, generator=g)
    vloc = torch.randn(3, 3, C, generator=g) + offset
    _check_loss(f"loss_offset_{offset:g}", loc, vloc, tgt, _samples(sizes, S, g), 1.5, 50.0)


# ----------------------------------------------------------------------------------------------------------------------
# Adam
# ----------------------------------------------------------------------------------------------------------------------
class _AdamMirror:
    """FusedAdam on fp32 parameters next to two torch.optim.Adam on float64 copies, fed the same fp32 gradients:
    `sync` is re-synchronised to the kernel's state before every step (one-step check, a few ulp), `free` runs on its own."""

    def __init__(self, init, lr, betas, eps, wd):
        self.p32 = [torch.nn.Parameter(t.clone().cuda()) for t in init]
        self.sync = [torch.nn.Parameter(t.double().cuda()) for t in init]
        self.free = [torch.nn.Parameter(t.double().cuda()) for t in init]
        self.opt = FusedAdam(self.p32, lr=lr, betas=betas, eps=eps, weight_decay=wd)
        kw = dict(lr=lr, betas=betas, eps=eps, weight_decay=wd, foreach=False)
        self.o_sync, self.o_free = torch.optim.Adam(self.sync, **kw), torch.optim.Adam(self.free, **kw)
        self.lr, self.b1, self.b2, self.eps, self.wd = lr, betas[0], betas[1], eps, wd
        self.steps = 0
        # EMAs of |g| + wd |p| and of its square: what the roundings of m and v scale with (g + wd p may cancel)
        self.m_abs = [torch.zeros_like(p) for p in self.free]
        self.v_abs = [torch.zeros_like(p) for p in self.free]
        self.p_acc = [torch.zeros_like(p) for p in self.free]      # the free run's bound on |p - p_fp64|, step by step

    def step(self, grads, case, bad, check_free):
        self.steps += 1
        for i, g in enumerate(grads):
            p, ps, pf = self.p32[i], self.sync[i], self.free[i]
            with torch.no_grad():
                ps.copy_(p)
                st = self.o_sync.state.get(ps)
                if st:
                    st["exp_avg"].copy_(self.opt.exp_avg[i]); st["exp_avg_sq"].copy_(self.opt.exp_avg_sq[i])
            p.grad = None if g is None else g.clone()
            ps.grad = None if g is None else g.double()
            pf.grad = None if g is None else g.double()
        before = [(ps.detach().clone(), self.o_sync.state[ps]["exp_avg"].clone() if ps in self.o_sync.state else torch.zeros_like(ps),
                   self.o_sync.state[ps]["exp_avg_sq"].clone() if ps in self.o_sync.state else torch.zeros_like(ps)) for ps in self.sync]
        self.opt.step(); self.o_sync.step(); self.o_free.step()
        b1, b2, wd = self.b1, self.b2, self.wd
        for i, g in enumerate(grads):
            if g is None:
                continue
            ga = g.double().abs() + wd * self.free[i].detach().abs()
            self.m_abs[i].mul_(b1).add_(ga, alpha=1 - b1)
            self.v_abs[i].mul_(b2).addcmul_(ga, ga, value=1 - b2)
        for i, g in enumerate(grads):
            p, m, v = self.p32[i].detach().double(), self.opt.exp_avg[i].double(), self.opt.exp_avg_sq[i].double()
            ps, st = self.sync[i].detach(), self.o_sync.state.get(self.sync[i])
            p0, m0, v0 = before[i]
            tag = f"{case} t{i} step {self.steps}"
            if g is None:      # skipped: nothing moved
                if not (torch.equal(p, p0) and torch.equal(m, m0.double()) and torch.equal(v, v0.double())):
                    bad.append(f"{tag}: a tensor without a gradient changed")
                continue
            gi = (g.double().abs() + wd * p0.abs())
            # one step from the same state: every product / sum of the update rounds once in fp32
            tol_m = 6 * U32 * (b1 * m0.abs() + (1 - b1) * gi)
            tol_v = 8 * U32 * (b2 * v0 + (1 - b2) * gi * gi) + 2.0 ** -126
            # ... and m's rounding (which may cancel) goes through lr_t / denominator into the parameter
            n = float(st["step"])
            den = (st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** n)).add_(self.eps)
            tol_p = 2 * U32 * ps.abs() + 8 * U32 * (ps - p0).abs() + self.lr / (1 - b1 ** n) * tol_m / den + 2.0 ** -140
            for nm, a, b, tol in (("p", p, ps, tol_p), ("m", m, st["exp_avg"], tol_m), ("v", v, st["exp_avg_sq"], tol_v)):
                e = (a - b).abs()
                if (e > tol).any():
                    j = int((e - tol).argmax())
                    bad.append(f"{tag} one-step {nm}: {int((e > tol).sum())} beyond, got {a.reshape(-1)[j].item():.9g} "
                               f"fp64 {b.reshape(-1)[j].item():.9g} tol {tol.reshape(-1)[j].item():.3g}")
            # the run: m and v carry the roundings of the last ~1 / (1 - beta) steps, the parameters' drift comes back into
            # them through the decay term wd p, and p sums every step's rounding and m's error (g + wd p may cancel) through
            # lr_t / denominator -- accumulated on every step, compared at the checkpoints
            pf, sf = self.free[i].detach(), self.o_free.state[self.free[i]]
            n = float(sf["step"])
            tol_m = 6 * U32 * min(n, 1 / (1 - b1)) * self.m_abs[i] + wd * self.p_acc[i] + 2.0 ** -126
            tol_v = 8 * U32 * min(n, 1 / (1 - b2)) * self.v_abs[i] + 2 * self.v_abs[i].sqrt() * wd * self.p_acc[i] + 2.0 ** -126
            den = (sf["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** n)).add_(self.eps)
            self.p_acc[i] += 2 * U32 * pf.abs() + 256 * U32 * self.lr + self.lr / (1 - b1 ** n) * tol_m / den
            tol_p = self.p_acc[i] + 2.0 ** -140
            if check_free:
                for nm, a, b, tol in (("p", p, pf, tol_p), ("m", m, sf["exp_avg"], tol_m), ("v", v, sf["exp_avg_sq"], tol_v)):
                    e = (a - b).abs()
                    if (e > tol).any():
                        j = int((e - tol).argmax())
                        bad.append(f"{tag} run {nm}: {int((e > tol).sum())} beyond, got {a.reshape(-1)[j].item():.9g} "
                                   f"fp64 {b.reshape(-1)[j].item():.9g} tol {tol.reshape(-1)[j].item():.3g}")


def _adam_tensors(g):
    """30 tensors (two launches of 24): 1-element tensors, 300 000 elements (above 64 x 256 x 4: the grid-stride loop),
    a tensor whose gradient is exactly zero, one at 1e-30 on zero parameters (eps regime), and ragged sizes"""
    sizes = [1, 300000, 1, 7, 64, 4096, 129, 1, 65537, 3, 333, 1000, 256, 1, 17, 70000, 5, 64 * 64, 1, 2,
             999, 65536, 8, 1, 31, 4097, 100, 1, 600, 12]
    init = [torch.randn(n, generator=g) for n in sizes]
    init[3].zero_()                                   # 1e-30 gradients on zero parameters
    return sizes, init


def _adam_grad(g, sizes, t):
    out = []
    for i, n in enumerate(sizes):
        x = torch.randn(n, generator=g) * (10.0 ** (i % 5 - 3))
        if i == 3:
            x = x.sign() * 1e-30
        elif i == 4 or (i == 6 and t % 7 == 0):
            x = torch.zeros(n)                        # exactly zero: only the decay term moves the moments
        elif i == 8:
            x = (x + 3.0) * 1e-2                       # a consistent sign: m / sqrt(v) near 1 throughout
        if i == 10 and t % 3 == 1:
            x = None                                   # gradient-less on every third step
        elif i == 20 and t < 5:
            x = None                                   # first gradient at step 5: its own step count starts there
        out.append(x.cuda() if x is not None else None)
    return out


@pytest.mark.parametrize("wd", [1e-12, 1e-2])
def test_adam_200_steps_vs_torch_fp64(wd):
    g = torch.Generator().manual_seed(21)
    sizes, init = _adam_tensors(g)
    mir = _AdamMirror(init, lr=1e-3, betas=(0.8, 0.99), eps=1e-8, wd=wd)
    bad = []
    for t in range(1, 201):
        mir.step(_adam_grad(g, sizes, t), f"adam_wd{wd:g}", bad, check_free=t in (1, 2, 3, 5, 6, 10, 50, 100, 200))
        assert not bad, bad[:8]


def test_adam_none_gradients_keep_their_own_step_count():
    """torch.optim.Adam keeps state['step'] per parameter and advances it only on steps where the parameter has a .grad,
    so a parameter first reached at step 2 takes the bias correction of step 1 (and one skipped at step 2 that of step 2
    at step 3)"""
    g = torch.Generator().manual_seed(22)
    init = [torch.randn(n, generator=g) for n in (5, 300, 1, 4000)]
    mir = _AdamMirror(init, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-12)
    pattern = {1: (1, 0, 1, 0), 2: (1, 1, 0, 0), 3: (1, 1, 1, 0), 4: (0, 1, 1, 1), 5: (1, 1, 1, 1), 6: (1, 0, 0, 1)}
    bad = []
    for t, has in pattern.items():
        grads = [torch.randn(p.numel(), generator=g).cuda() if h else None for p, h in zip(mir.p32, has)]
        mir.step(grads, "adam_none", bad, check_free=True)
        assert not bad, bad[:8]
    assert mir.opt.steps == [5, 4, 4, 3]


def test_adam_wide_model_parameter_list():
    """the whole parameter list of a hidden_nf = 128 FastEGNN (the wide path, more than 24 tensors) with its real gradients,
    None where the model leaves them None"""
    cfg = R.Config(2, 0, 2, 128, 4, n_layers=3)
    _, m = _models(cfg, 31)
    inp = {k: v.cuda() for k, v in _batch([60, 45], 4, 4, seed=31).items()}
    params = list(m.parameters())
    mir = _AdamMirror([p.detach().cpu() for p in params], lr=5e-4, betas=(0.9, 0.999), eps=1e-8, wd=1e-12)
    bad = []
    for t in range(1, 11):
        with torch.no_grad():
            for p, q in zip(params, mir.p32):
                p.copy_(q)
            for p in params:
                p.grad = None
        loc, vloc = m(**inp)
        (torch.nn.functional.mse_loss(loc, inp["node_loc"] + 0.3) + 0.05 * vloc.pow(2).mean()).backward()
        grads = [p.grad.detach().clone() if p.grad is not None else None for p in params]
        mir.step(grads, "adam_h128", bad, check_free=True)
        assert not bad, bad[:8]
    assert len(params) > 24


# ----------------------------------------------------------------------------------------------------------------------
# augment_edge_attr
# ----------------------------------------------------------------------------------------------------------------------
# relative error of the length per element in units of u: one rounding each of the difference, square, two sums and sqrt
# (worst measured on an MI355X: 2.35 u, 300 000 edges 1e3 from the origin)
AUG_K = 6.0


@pytest.mark.parametrize("k", [0, 1, 3])
@pytest.mark.parametrize("E,offset", [(0, 0.0), (1, 0.0), (2_000_000, 0.0), (300_000, 1e3)])
def test_augment_edge_attr_vs_fp64(k, E, offset):
    g = torch.Generator().manual_seed(k * 7 + E % 97)
    N = 100_000 if E > 1 else 10
    loc = torch.rand(N, 3, generator=g) + offset
    ei = torch.randint(0, N, (2, E), generator=g)
    if E > 1:
        ei[1, :: 50] = ei[0, :: 50]                        # self loops: length exactly 0
    ea = torch.randn(E, k, generator=g) if k else None
    out = augment_edge_attr(ea.cuda() if k else None, loc.cuda(), ei.cuda()).cpu()
    assert out.shape == (E, k + 1) and out.dtype == torch.float32
    if k:
        assert torch.equal(out[:, :k], ea)                 # copied bit for bit
    truth = R.augment_edge_attr(torch.zeros(E, 0, dtype=torch.float64), loc.double(), ei)[:, 0]
    got = out[:, k].double()
    assert torch.equal(got[ei[0] == ei[1]], torch.zeros(int((ei[0] == ei[1]).sum()), dtype=torch.float64))
    err = ((got - truth).abs() / truth.clamp(min=1e-300))[truth > 0]
    worst = float(err.max()) / U32 if err.numel() else 0.0
    if _DUMP:
        with open(_DUMP, "a") as f:
            f.write(json.dumps({"case": f"augment_k{k}_E{E}_off{offset:g}", "tensor": "length", "elementwise_ratio": worst,
                                "k": AUG_K}) + "\n")
        return
    assert worst <= AUG_K, worst


# ----------------------------------------------------------------------------------------------------------------------
# the whole training step
# ----------------------------------------------------------------------------------------------------------------------
# |loss - fp64| / |fp64 loss| per step.  Measured on an MI355X: hidden_nf = 64 (f16x2 products) at most 1.20e-5 / 9.82e-6 over two
# runs (step 3), hidden_nf = 128 (wide path) <= 4.2e-7: the loss is a mean of squared displacement errors ~0.1 while the output
# contract is 1e-5 relative to |loc| ~ 2
TRAIN_LOSS_TOL = 2e-5


@pytest.mark.parametrize("H", [64, 128])
def test_train_step_five_steps_vs_fp64_mirror(H):
    """train_step on a cfg2-like batch (100 graphs x 100 nodes, C = 3, S = 9; 10 edges per node instead of the complete
    graph, to keep the fp64 mirror's CPU time down) for 5 steps against oracle forward + loss_mse_mmd_nodes + torch Adam in
    float64 with the same samples"""
    C, S, sigma, weight, lr, wd = 3, 9, 1.5, 0.1, 5e-4, 1e-12
    cfg = R.Config(2, 0, 2, H, C, n_layers=4)
    sizes = [100] * 100
    inp = _batch(sizes, 10, C, seed=40 + H, ea=1)
    g = torch.Generator().manual_seed(41)
    samp = _samples(sizes, S, g)
    loc_t = inp["node_loc"] + 0.3 * inp["node_vel"] + 0.01 * torch.randn(inp["node_loc"].shape, generator=g)
    p0, m = _models(cfg, 40 + H)
    data = dict(loc_0=inp["node_loc"], vel_0=inp["node_vel"], loc_t=loc_t, node_feat=inp["node_feat"],
                edge_index=inp["edge_index"], edge_attr=inp["edge_attr"], batch=inp["data_batch"], loc_mean=inp["loc_mean"])
    dev = {k: v.cuda() for k, v in data.items()}
    opt = FusedAdam(m.parameters(), lr=lr, weight_decay=wd)
    names = [k for k, _ in m.named_parameters()]
    p64 = {k: p0[k].double().clone().requires_grad_(True) for k in names}
    o64 = torch.optim.Adam([p64[k] for k in names], lr=lr, weight_decay=wd, foreach=False)

    def mirror(p, dt):
        f = {k: (v.to(dt) if v.is_floating_point() else v) for k, v in data.items()}
        ea = R.augment_edge_attr(f["edge_attr"], f["loc_0"], f["edge_index"])
        loc, vloc = R.forward(p, cfg, f["node_feat"], f["loc_0"], f["vel_0"], f["edge_index"], f["batch"], f["loc_mean"],
                              edge_attr=ea)
        return R.loss_mse_mmd_nodes(loc, vloc, f["loc_t"], samp, sigma, weight)

    bad = []
    for step in range(1, 6):
        o64.zero_grad()
        l64, mse64 = mirror(p64, torch.float64)
        l64.backward()
        loss, mse = train_step(m, opt, dev, samp.cuda(), sigma, weight)
        e = abs(float(loss) - l64.item()) / abs(l64.item())
        if _DUMP:
            with open(_DUMP, "a") as f:
                f.write(json.dumps({"case": f"train_h{H}", "tensor": f"loss_step{step}", "rel": e, "tol": TRAIN_LOSS_TOL}) + "\n")
        elif e > TRAIN_LOSS_TOL or abs(float(mse) - mse64.item()) > TRAIN_LOSS_TOL * abs(mse64.item()):
            bad.append(f"step {step}: loss {float(loss):.9g} vs {l64.item():.9g}, mse {float(mse):.9g} vs {mse64.item():.9g}")
        if step == 1:
            p32 = {k: p0[k].clone().requires_grad_(True) for k in names}
            mirror(p32, torch.float32)[0].backward()
            for k, p in m.named_parameters():
                got = p.grad if p.grad is not None else torch.zeros_like(p)
                assert (p.grad is None) == (p64[k].grad is None), k
                tru = p64[k].grad if p64[k].grad is not None else torch.zeros_like(p64[k])
                ref = p32[k].grad if p32[k].grad is not None else torch.zeros_like(p32[k])
                # the hidden_nf = 128 model runs the wide path: its run-to-run band is GRAD_EXCEPTIONS' "wide_" entry
                grad_check(f"train_h{H}" if H <= 64 else f"wide_train_h{H}", k, got, ref, tru, bad)
        o64.step()
    sd = m.state_dict()
    nbad = sum(int(((sd[k].cpu().double() - p64[k].detach()).abs() > 5e-5).sum()) for k in names)
    tot = sum(p64[k].numel() for k in names)
    # Adam normalises the gradient: entries whose gradient is pure rounding noise may flip sign (tests/test_gpu_train.py)
    if nbad > 2e-4 * tot:
        bad.append(f"after 5 steps {nbad} of {tot} parameters beyond 5e-5")
    assert not bad, bad
