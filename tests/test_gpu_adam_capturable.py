"""-m gpu: FusedAdam(capturable=True) -- fastegnn_adam_step_dev / fastegnn_grad_sqnorm (csrc/train.hip): step counts, hyper-parameters,
clipping and the decision to skip on the device -- against torch.optim.Adam in float64 under the error model of
tests/test_gpu_train_kernels.py (_AdamMirror: one fp32 rounding per product or sum, accumulated over the run), against the host-side
FusedAdam, and replayed from a captured HIP graph against the same launches issued eagerly."""
import math

import pytest
import torch

from fastegnn_amd.train import FusedAdam
from tests.helpers import U32
from tests.test_gpu_train_kernels import _AdamMirror, _adam_grad, _adam_tensors

pytestmark = pytest.mark.gpu


class _DevMirror(_AdamMirror):
    """_AdamMirror driving the device-side optimizer: same fp64 references, same bounds"""

    def __init__(self, init, lr, betas, eps, wd, **kw):
        super().__init__(init, lr, betas, eps, wd)
        self.opt = FusedAdam(self.p32, lr=lr, betas=betas, eps=eps, weight_decay=wd, capturable=True, **kw)

    def set_lr(self, lr):
        self.opt.lr = lr
        self.lr = lr
        for o in (self.o_sync, self.o_free):
            o.param_groups[0]["lr"] = lr


def _torch_steps(opt, params):
    return [int(opt.state[p]["step"]) if p in opt.state else 0 for p in params]


def _state(opt):
    return [t.clone() for t in opt.params + opt.exp_avg + opt.exp_avg_sq]


def _same(a, b):
    return all(torch.equal(x, y) for x, y in zip(a, b))


def test_30_steps_vs_torch_fp64_and_host_side_optimizer():
    """30 tensors (two launches of 24; sizes 1, 7, 4097, 70 000, 300 000 among them), 30 steps, one tensor gradient-less on every
    third step and one whose first gradient arrives at step 5.  The device-side optimizer also reduces the gradient norm here
    (max_grad_norm = 1e30: the coefficient is exactly 1, so the plain Adam bounds hold unchanged)."""
    wd = 1e-2
    gd, gh = torch.Generator().manual_seed(21), torch.Generator().manual_seed(21)
    sizes, init = _adam_tensors(gd)
    _adam_tensors(gh)
    assert {1, 7, 4097, 70000, 300000} <= set(sizes) and len(sizes) == 30
    dev = _DevMirror(init, lr=1e-3, betas=(0.8, 0.99), eps=1e-8, wd=wd, max_grad_norm=1e30)
    host = _AdamMirror(init, lr=1e-3, betas=(0.8, 0.99), eps=1e-8, wd=wd)
    bad = []
    for t in range(1, 31):
        grads = _adam_grad(gd, sizes, t)
        same = _adam_grad(gh, sizes, t)
        check = t in (1, 2, 3, 5, 6, 10, 20, 30)
        dev.step(grads, "adam_dev", bad, check_free=check)
        host.step(same, "adam_host", bad, check_free=check)
        assert not bad, bad[:8]
    want = _torch_steps(dev.o_free, dev.free)
    assert dev.opt.steps == want and host.opt.steps == want
    assert want[10] == 20 and want[20] == 26 and want[0] == 30
    # device-side against host-side: both sit inside the run's bound around the same fp64 trajectory; they are held to ONE such
    # bound of each other (they differ by the fp32 rounding of lr_t and 1 / sqrt(bc2), formed on the device here and on the host there)
    b1, b2 = dev.b1, dev.b2
    for i, n in enumerate(want):
        tol_p = dev.p_acc[i] + 2.0 ** -140
        tol_m = 6 * U32 * min(n, 1 / (1 - b1)) * dev.m_abs[i] + wd * dev.p_acc[i] + 2.0 ** -126
        tol_v = 8 * U32 * min(n, 1 / (1 - b2)) * dev.v_abs[i] + 2 * dev.v_abs[i].sqrt() * wd * dev.p_acc[i] + 2.0 ** -126
        for nm, a, b, tol in (("p", dev.p32[i], host.p32[i], tol_p), ("m", dev.opt.exp_avg[i], host.opt.exp_avg[i], tol_m),
                              ("v", dev.opt.exp_avg_sq[i], host.opt.exp_avg_sq[i], tol_v)):
            e = (a.detach().double() - b.detach().double()).abs()
            assert not (e > tol).any(), (i, nm, float(e.max()))
    # the norm of the last step's gradients (30 tensors, one of them absent): see test_gradient_norm_scalar for the bound
    ref = sum(float(g.double().pow(2).sum()) for g in grads if g is not None)
    got = float(dev.opt.grad_sqnorm)
    assert abs(got - ref) <= dev.opt.n_partials * 2.0 ** -52 * 4 * ref


def test_skip_word_leaves_everything_bitwise_and_the_count_unadvanced():
    g = torch.Generator().manual_seed(23)
    sizes = [1, 7, 4097, 70000]
    init = [torch.randn(n, generator=g) for n in sizes]
    mir = _DevMirror(init, lr=1e-2, betas=(0.9, 0.999), eps=1e-8, wd=1e-2)
    word = torch.zeros(1, dtype=torch.int32, device="cuda")
    mir.opt.skip_word = word
    bad = []

    def grads():
        return [torch.randn(n, generator=g).cuda() for n in sizes]
    for _ in range(2):
        mir.step(grads(), "skip", bad, check_free=True)
    word.fill_(1)
    before, steps = _state(mir.opt), mir.opt.steps
    for p, x in zip(mir.p32, grads()):
        p.grad = x
    mir.opt.step()
    assert _same(before, _state(mir.opt)) and mir.opt.steps == steps == [2] * 4
    word.zero_()
    # the fp64 optimizers never saw the skipped call: the next step must take the bias correction of count 3
    mir.step(grads(), "after_skip", bad, check_free=True)
    assert not bad, bad[:8]
    assert mir.opt.steps == [3] * 4


def test_non_finite_gradient_norm_skips_the_step():
    g = torch.Generator().manual_seed(24)
    sizes = [1, 7, 4097, 70000]
    params = [torch.nn.Parameter(torch.randn(n, generator=g).cuda()) for n in sizes]
    opt = FusedAdam(params, lr=1e-2, weight_decay=1e-2, capturable=True, max_grad_norm=1.0)
    for p in params:
        p.grad = torch.randn(p.numel(), generator=g).cuda()
    opt.step()
    before = _state(opt)
    for bad_value in (float("inf"), float("-inf"), float("nan")):
        params[3].grad[40001] = bad_value
        opt.step()
        assert not math.isfinite(float(opt.grad_sqnorm))
        assert _same(before, _state(opt)) and opt.steps == [1] * 4
    params[3].grad[40001] = 0.5
    opt.step()
    assert opt.steps == [2] * 4 and not torch.equal(before[0], params[0])


@pytest.mark.parametrize("scale,clipped", [(1e-3, False), (50.0, True)])
def test_clipping_vs_torch_clip_grad_norm_fp64(scale, clipped):
    """torch.nn.utils.clip_grad_norm_ + torch.optim.Adam in float64, re-synchronised to the kernel's state before every step (the
    one-step check of _AdamMirror).  The gradient norm is `scale` x max_grad_norm: below it (coefficient exactly 1) and 50 x above.
    Bounds: _AdamMirror's one-step bounds, with TWO more fp32 roundings on the gradient -- the coefficient rounded to fp32 and its
    product with the gradient -- i.e. 2 u more on m (6 -> 8), 4 u more on v, which holds the gradient squared (8 -> 12), and 2 u more
    on the update (8 -> 10, half of v's through the square root)."""
    lr, b1, b2, eps, wd, max_norm = 1e-2, 0.9, 0.999, 1e-8, 1e-2, 2.0
    g = torch.Generator().manual_seed(25)
    sizes = [1, 7, 4097, 70000]
    init = [torch.randn(n, generator=g) for n in sizes]
    p32 = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    p64 = [torch.nn.Parameter(t.double().cuda()) for t in init]
    opt = FusedAdam(p32, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, capturable=True, max_grad_norm=max_norm)
    o64 = torch.optim.Adam(p64, lr=lr, betas=(b1, b2), eps=eps, weight_decay=wd, foreach=False)
    for step in range(1, 4):
        raw = [torch.randn(n, generator=g) for n in sizes]
        norm = math.sqrt(sum(float(x.double().pow(2).sum()) for x in raw))
        raw = [(x * (scale * max_norm / norm)).cuda() for x in raw]
        state0 = []
        for i, (p, q) in enumerate(zip(p32, p64)):
            with torch.no_grad():
                q.copy_(p)
                if q in o64.state:
                    o64.state[q]["exp_avg"].copy_(opt.exp_avg[i]); o64.state[q]["exp_avg_sq"].copy_(opt.exp_avg_sq[i])
            state0.append((q.detach().clone(), opt.exp_avg[i].double(), opt.exp_avg_sq[i].double()))
            p.grad, q.grad = raw[i].clone(), raw[i].double()
        total = torch.nn.utils.clip_grad_norm_(p64, max_norm)
        assert (float(total) > max_norm) == clipped
        clipped64 = [q.grad.clone() for q in p64]
        opt.step(); o64.step()
        for i, q in enumerate(p64):
            assert torch.equal(p32[i].grad, raw[i])          # the gradient buffers are not rewritten
            p0, m0, v0 = state0[i]
            st = o64.state[q]
            gi = clipped64[i].abs() + wd * p0.abs()
            tol_m = 8 * U32 * (b1 * m0.abs() + (1 - b1) * gi)
            tol_v = 12 * U32 * (b2 * v0 + (1 - b2) * gi * gi) + 2.0 ** -126
            den = (st["exp_avg_sq"].sqrt() / math.sqrt(1 - b2 ** step)).add_(eps)
            tol_p = 2 * U32 * q.detach().abs() + 10 * U32 * (q.detach() - p0).abs() + lr / (1 - b1 ** step) * tol_m / den + 2.0 ** -140
            for nm, a, b, tol in (("p", p32[i].detach().double(), q.detach(), tol_p), ("m", opt.exp_avg[i].double(), st["exp_avg"], tol_m),
                                  ("v", opt.exp_avg_sq[i].double(), st["exp_avg_sq"], tol_v)):
                e = (a - b).abs()
                assert not (e > tol).any(), (step, i, nm, float((e / tol.clamp(min=1e-300)).max()))
        assert opt.steps == [step] * 4 == [int(o64.state[q]["step"]) for q in p64]


def test_gradient_norm_scalar():
    """sum of squares of 30 gradient tensors (two launches; 1 to 300 000 elements; one absent) against float64 torch.  Every square
    is exact in fp64 (24-bit x 24-bit), so the only error is the rounding of fp64 sums: the workgroup partials are summed by one
    final workgroup, and the relative error is held below n_partials * 2^-52 * 4 (1566 partials here: 1.4e-12; measured on an
    MI355X: 0, the same double as torch's own sum).  Two runs give the same bits."""
    g = torch.Generator().manual_seed(26)
    sizes, init = _adam_tensors(g)
    params = [torch.nn.Parameter(t.cuda()) for t in init]
    opt = FusedAdam(params, lr=0.0, capturable=True, max_grad_norm=1.0)
    for i, p in enumerate(params):
        p.grad = None if i == 5 else (torch.randn(p.numel(), generator=g) * 10.0 ** (i % 5 - 2)).cuda()
    assert opt.n_partials == 24 * 64 + 6 * 5
    ref = sum(float(p.grad.double().pow(2).sum()) for p in params if p.grad is not None)
    opt.step()
    first = opt.grad_sqnorm.clone()
    rel = abs(float(first) - ref) / ref
    print(f"grad_sqnorm: {float(first)!r} vs fp64 {ref!r}: relative error {rel:.3g}, {opt.n_partials} partials")
    assert rel < opt.n_partials * 2.0 ** -52 * 4
    opt.step()
    assert torch.equal(first, opt.grad_sqnorm)


def test_replayed_step_equals_eager_step_bitwise():
    """opt.step() captured once (static gradient buffers) and replayed 12 times, lr halved after replay 6, against a second
    capturable optimizer that issues the same launches eagerly: bitwise equal -- and that one inside the fp64 bounds.  A bias
    correction or an lr frozen into the graph fails at replay 2 / 7 (the host-side FusedAdam cannot pass this: its step counts and
    lr are launch arguments)."""
    lr = 2e-3
    g = torch.Generator().manual_seed(27)
    sizes = [1, 7, 4097, 70000, 300000, 64, 12]
    init = [torch.randn(n, generator=g) for n in sizes]
    kw = dict(lr=lr, betas=(0.9, 0.999), eps=1e-8, weight_decay=1e-2, capturable=True, max_grad_norm=1e30)
    mir = _DevMirror(init, lr, (0.9, 0.999), 1e-8, 1e-2, max_grad_norm=1e30)      # the eager optimizer, with its fp64 references
    pa = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    opt = FusedAdam(pa, **kw)
    static = [None if i == 5 else torch.zeros(n, device="cuda") for i, n in enumerate(sizes)]   # tensor 5 never has a gradient
    for p, s in zip(pa, static):
        p.grad = s
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    opt.skip_word = word
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        opt.step()                                        # loads the kernels outside the capture; held by the skip word
    torch.cuda.current_stream().wait_stream(stream)
    word.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        opt.step()
    assert opt.steps == [0] * len(sizes) and all(torch.equal(p.detach().cpu(), t) for p, t in zip(pa, init))
    bad = []
    for k in range(1, 13):
        grads = [None if s is None else (torch.randn(s.numel(), generator=g) * 10.0 ** (i % 3 - 1)).cuda() for i, s in enumerate(static)]
        for s, x in zip(static, grads):
            if s is not None:
                s.copy_(x)
        graph.replay()
        mir.step(grads, "replay", bad, check_free=True)
        assert not bad, bad[:8]
        assert _same(_state(opt), _state(mir.opt)), f"replay {k} differs from the eager step"
        if k == 6:
            opt.lr = lr / 2
            mir.set_lr(lr / 2)
    assert opt.steps == mir.opt.steps == [12, 12, 12, 12, 12, 0, 12]
    assert torch.equal(pa[5].detach().cpu(), init[5])
