"""-m gpu: FusedAdam.state_dict / load_state_dict on the device (fastegnn_amd/train.py).  A run that saves after k steps and one that
loads that state into a FRESH optimizer over cloned parameters take the same m further steps bit for bit, in the host-side mode, in
the capturable mode (counts and hyper-parameters in device memory) and through a conversion to the other mode and back; a captured
``step()`` graph keeps replaying correctly after ``load_state_dict`` because the load writes in place.  The capture pattern is the one
of tests/test_gpu_adam_capturable.py: the optimizer step alone, static gradient buffers."""
import pytest
import torch

from fastegnn_amd.train import FusedAdam

pytestmark = pytest.mark.gpu

SIZES = [1, 7, 4097, 70000, 12]
KW = dict(lr=2e-3, betas=(0.8, 0.99), eps=1e-8, weight_decay=1e-2)
K_STEPS, M_STEPS = 3, 2


def _init(seed=31):
    g = torch.Generator().manual_seed(seed)
    return [torch.randn(n, generator=g) for n in SIZES]


def _grads(seed=32):
    """K_STEPS + M_STEPS gradient lists; tensor 2 has none on step 2 and tensor 4 none before step 3: per-parameter counts differ"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for t in range(1, K_STEPS + M_STEPS + 1):
        out.append([None if (i == 2 and t == 2) or (i == 4 and t < 3) else (torch.randn(n, generator=g) * 10.0 ** (i % 3 - 1)).cuda()
                    for i, n in enumerate(SIZES)])
    return out


def _make(init, capturable, **kw):
    params = [torch.nn.Parameter(t.clone().cuda()) for t in init]
    return params, FusedAdam(params, capturable=capturable, **{**KW, **kw})


def _steps(opt, params, grads):
    for gs in grads:
        for p, g in zip(params, gs):
            p.grad = g
        opt.step()


def _snapshot(opt, params):
    return [t.detach().clone() for t in params + opt.exp_avg + opt.exp_avg_sq], list(opt.steps)


def _same(a, b):
    return a[1] == b[1] and all(torch.equal(x, y) for x, y in zip(a[0], b[0]))


@pytest.mark.parametrize("capturable", [False, True])
def test_saved_state_continues_bitwise_in_a_fresh_optimizer(capturable):
    grads = _grads()
    params, opt = _make(_init(), capturable)
    _steps(opt, params, grads[:K_STEPS])
    sd, at_save = opt.state_dict(), [p.detach().clone() for p in params]
    assert [int(sd["state"][i]["step"]) for i in range(5)] == [3, 3, 2, 3, 1] == opt.steps
    _steps(opt, params, grads[K_STEPS:])
    want = _snapshot(opt, params)
    assert want[1] == [5, 5, 4, 5, 3]
    assert int(sd["state"][0]["step"]) == 3 and not torch.equal(sd["state"][0]["exp_avg"], opt.exp_avg[0])   # the saved state did not move
    params2, opt2 = _make([p.cpu() for p in at_save], capturable, lr=9.0, betas=(0.5, 0.5), weight_decay=0.0)  # other hyper-parameters: loaded
    opt2.load_state_dict(sd)
    assert opt2.steps == [3, 3, 2, 3, 1] and opt2.lr == KW["lr"] and opt2.betas == KW["betas"]
    _steps(opt2, params2, grads[K_STEPS:])
    assert _same(_snapshot(opt2, params2), want)


@pytest.mark.parametrize("capturable", [False, True])
def test_a_state_survives_the_conversion_to_the_other_mode_and_back(capturable):
    """mode A saves; a fresh optimizer of the OTHER mode loads it (moments and counts arrive bit for bit) and saves again; a fresh
    optimizer of mode A loads that and continues as the uninterrupted run does.  (The two modes' own steps differ in the last bit of the
    bias corrections, formed on the host in one and on the device in the other: tests/test_gpu_adam_capturable.py bounds that.)"""
    grads = _grads()
    params, opt = _make(_init(), capturable)
    _steps(opt, params, grads[:K_STEPS])
    sd, at_save = opt.state_dict(), [p.detach().clone() for p in params]
    _steps(opt, params, grads[K_STEPS:])
    want = _snapshot(opt, params)
    pb, other = _make([p.cpu() for p in at_save], not capturable)
    other.load_state_dict(sd)
    assert other.capturable == (not capturable) and other.steps == [3, 3, 2, 3, 1]
    for i in range(5):
        assert torch.equal(other.exp_avg[i], sd["state"][i]["exp_avg"]) and torch.equal(other.exp_avg_sq[i], sd["state"][i]["exp_avg_sq"])
    sd_other = other.state_dict()
    assert sd_other["param_groups"][0]["capturable"] == (not capturable)
    _steps(other, pb, grads[K_STEPS:])                        # the converted optimizer steps on, every count advancing as the source's
    assert other.steps == want[1]
    pc, back = _make([p.cpu() for p in at_save], capturable)
    back.load_state_dict(sd_other)
    _steps(back, pc, grads[K_STEPS:])
    assert _same(_snapshot(back, pc), want)


def test_a_captured_step_replays_on_from_a_state_loaded_in_place():
    """replay twice, save, replay twice more; put the parameters back, load_state_dict, replay the same two steps: the same bits.  The
    graph holds the addresses of the moments, the counts and the hyper-parameters: a load that re-allocated any of them would leave
    the graph stepping the old buffers."""
    g = torch.Generator().manual_seed(33)
    sizes = SIZES
    params, opt = _make(_init(), True, max_grad_norm=1e30)
    static = [None if i == 2 else torch.zeros(n, device="cuda") for i, n in enumerate(sizes)]   # tensor 2 never has a gradient
    for p, s in zip(params, static):
        p.grad = s
    word = torch.ones(1, dtype=torch.int32, device="cuda")
    opt.skip_word = word
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        opt.step()                                            # loads the kernels outside the capture; held by the skip word
    torch.cuda.current_stream().wait_stream(stream)
    word.zero_()
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        opt.step()
    fills = [[None if s is None else torch.randn(s.numel(), generator=g).cuda() for s in static] for _ in range(4)]

    def replay(fill):
        for s, x in zip(static, fill):
            if s is not None:
                s.copy_(x)
        graph.replay()
    ptrs = [t.data_ptr() for t in opt.exp_avg + opt.exp_avg_sq] + [opt._dev["steps"].data_ptr(), opt._dev["hyper"].data_ptr()]
    replay(fills[0]); replay(fills[1])
    sd, at_save = opt.state_dict(), [p.detach().clone() for p in params]
    assert opt.steps == [2, 2, 0, 2, 2]
    replay(fills[2]); replay(fills[3])
    want = _snapshot(opt, params)
    assert want[1] == [4, 4, 0, 4, 4]
    with torch.no_grad():
        for p, x in zip(params, at_save):
            p.copy_(x)
    opt.load_state_dict(sd)
    assert ptrs == [t.data_ptr() for t in opt.exp_avg + opt.exp_avg_sq] + [opt._dev["steps"].data_ptr(), opt._dev["hyper"].data_ptr()]
    assert opt.steps == [2, 2, 0, 2, 2]
    replay(fills[2]); replay(fills[3])
    assert _same(_snapshot(opt, params), want)


def test_state_is_neither_read_nor_written_inside_a_capture():
    params, opt = _make(_init(), True)
    for p in params:
        p.grad = torch.zeros_like(p)
    sd = opt.state_dict()
    stream = torch.cuda.Stream()
    stream.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(stream):
        opt.step()
    torch.cuda.current_stream().wait_stream(stream)
    before = _snapshot(opt, params)
    graph = torch.cuda.CUDAGraph()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(RuntimeError, match="stream capture"):
            opt.load_state_dict(sd)
        with pytest.raises(RuntimeError, match="stream capture"):
            opt.state_dict()
        opt.step()
    assert _same(_snapshot(opt, params), before)              # neither call touched anything, and the capture ran nothing
    graph.replay()
    assert opt.steps == [2] * 5


def test_load_state_dict_names_the_index_of_a_wrong_shape():
    params, opt = _make(_init(), True)
    sd = opt.state_dict()
    sd["state"][3]["exp_avg"] = torch.zeros(5)
    with pytest.raises(ValueError, match="exp_avg of parameter 3"):
        opt.load_state_dict(sd)
    sd = opt.state_dict()
    sd["param_groups"][0]["params"] = list(range(6))
    with pytest.raises(ValueError, match="6 parameters.*5"):
        opt.load_state_dict(sd)
