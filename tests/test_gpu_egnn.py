"""-m gpu: the EGNN baseline on the HIP kernels (fastegnn_amd/egnn.py, FASTEGNN_F_EGNN wiring) against goldens
captured from the reference's models/basic.py EGNN: outputs and every gradient; plus a mid-size oracle check."""
import pytest
import torch

import fastegnn_amd
from oracle import egnn_ref as E
from tests.helpers import grad_check, rel_err
from tests.test_egnn_oracle_cpu import EGNN_NAMES, EGNN_WIDE_NAMES, egnn_act, egnn_loss, load_egnn

pytestmark = pytest.mark.gpu


def _egnn_of_golden(g):
    """the module a golden's meta describes, before its weights are loaded (a helper of its own: tests/test_gpu_x3_build.py wraps it to run
    the same comparison on the wide-range build)"""
    meta = g["meta"]
    return fastegnn_amd.EGNN(n_layers=int(meta["L"]), in_node_nf=2, in_edge_nf=2, hidden_nf=int(meta.get("hidden", 64)), device="cuda",
                             with_v=bool(int(meta["with_v"])), norm=bool(int(meta.get("norm", 0))), flat=bool(int(meta.get("flat", 0))))


# (EGNN_WIDE_NAMES: flat=True and hidden_nf = 128 -- the sibling on the unfused wide path, fastegnn_amd/wide.py)
@pytest.mark.parametrize("name", EGNN_NAMES + EGNN_WIDE_NAMES)
def test_egnn_matches_reference_golden(name):
    g = load_egnn(name)
    with_v = bool(int(g["meta"]["with_v"]))
    norm = bool(int(g["meta"].get("norm", 0)))
    m = _egnn_of_golden(g)
    assert m._wide == (name in EGNN_WIDE_NAMES)
    assert list(m.state_dict().keys()) == list(g["p"].keys())
    m.load_state_dict(g["p"], strict=True)
    m = m.cuda()
    i = {k: v.cuda() for k, v in g["in"].items()}
    leaf = {k: i[k].clone().requires_grad_(True) for k in ("x", "h") + (("v",) if with_v else ())}
    out = m(x=leaf["x"], h=leaf["h"], edge_index=i["edge_index"], edge_fea=i["edge_fea"], v=leaf.get("v"))
    x, h = out[0], out[-1]
    assert len(out) == (3 if with_v else 2)
    assert rel_err(x, g["out"]["x"]) < 1e-5, rel_err(x, g["out"]["x"])
    assert rel_err(h, g["out"]["h"]) < 2e-5
    egnn_loss(x, h, i["target"], i["wh"]).backward()
    # fp64 truth from the oracle on the golden's fp32 weights / inputs; the reference's fp32 gradients are the goldens
    dt = torch.float64
    p64 = {k: v.to(dt).clone().requires_grad_(True) for k, v in g["p"].items()}
    l64 = {k: g["in"][k].to(dt).clone().requires_grad_(True) for k in leaf}
    x64, h64 = E.forward(p64, int(g["meta"]["L"]), l64["x"], l64["h"], g["in"]["edge_index"], g["in"]["edge_fea"].to(dt), l64.get("v"), norm=norm,
                         act=egnn_act(g))
    egnn_loss(x64, h64, g["in"]["target"].to(dt), g["in"]["wh"].to(dt)).backward()
    bad = []
    for k, p in m.named_parameters():
        got = p.grad if p.grad is not None else torch.zeros_like(p)
        tru = p64[k].grad if p64[k].grad is not None else torch.zeros_like(p64[k])
        grad_check(name, f"gp/{k}", got, g["gp"][k], tru, bad)
    for k, v in leaf.items():
        grad_check(name, f"gin/{k}", v.grad, g["gin"][k], l64[k].grad, bad)
    assert not bad, bad


def test_egnn_mid_size_vs_oracle():
    g = torch.Generator().manual_seed(3)
    N, Ed = 3000, 40000
    torch.manual_seed(5)
    m = fastegnn_amd.EGNN(n_layers=3, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    x = torch.randn(N, 3, generator=g); h = torch.rand(N, 2, generator=g); v = torch.randn(N, 3, generator=g) * 0.2
    ei = torch.randint(0, N, (2, Ed), generator=g); ea = torch.rand(Ed, 2, generator=g)
    # edge_fea is a differentiable input of the reference layer (basic.py:313): its gradient comes back in the caller's edge order
    ea_gpu = ea.cuda().requires_grad_(True)
    xo, vo, ho = m(x=x.cuda(), h=h.cuda(), edge_index=ei.cuda(), edge_fea=ea_gpu, v=v.cuda())
    (xo.pow(2).mean() + ho.pow(2).mean()).backward()
    ea32 = ea.clone().requires_grad_(True)
    xr, hr = E.forward(p, 3, x, h, ei, ea32, v)
    (xr.pow(2).mean() + hr.pow(2).mean()).backward()
    assert rel_err(xo, xr) < 1e-5 and rel_err(ho, hr) < 2e-5
    dt = torch.float64
    p64 = {k: t.detach().to(dt).clone().requires_grad_(True) for k, t in p.items()}
    ea64 = ea.to(dt).requires_grad_(True)
    x64, h64 = E.forward(p64, 3, x.to(dt), h.to(dt), ei, ea64, v.to(dt))
    (x64.pow(2).mean() + h64.pow(2).mean()).backward()
    bad = []
    for k, prm in m.named_parameters():
        grad_check("egnn_mid_size", k, prm.grad, p[k].grad, p64[k].grad, bad)
    assert ea_gpu.grad is not None and ea_gpu.grad.shape == ea.shape
    grad_check("egnn_mid_size", "gin/edge_fea", ea_gpu.grad.cpu(), ea32.grad, ea64.grad, bad)
    assert not bad, bad


@pytest.mark.parametrize("hidden", [24, 40])
def test_egnn_narrow_hidden_nf_vs_oracle(hidden):
    """--dim_hidden below 64 on the EGNN sibling (main_nbody.py:107): the parameters run zero-padded on the 64-wide tiles
    (fastegnn_pad_params with the EGNN block layout: one leading radial column in the message MLP's input), the returned h
    has the reference's width, gradients arrive in the reference's shapes."""
    g = torch.Generator().manual_seed(11)
    N, Ed = 900, 9000
    torch.manual_seed(6)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=hidden, device="cuda", with_v=True)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    x = torch.randn(N, 3, generator=g); h = torch.rand(N, 2, generator=g); v = torch.randn(N, 3, generator=g) * 0.2
    ei = torch.randint(0, N, (2, Ed), generator=g); ea = torch.rand(Ed, 2, generator=g)
    xo, vo, ho = m(x=x.cuda(), h=h.cuda(), edge_index=ei.cuda(), edge_fea=ea.cuda(), v=v.cuda())
    assert ho.shape == (N, hidden)
    (xo.pow(2).mean() + ho.pow(2).mean()).backward()
    xr, hr = E.forward(p, 2, x, h, ei, ea, v)
    (xr.pow(2).mean() + hr.pow(2).mean()).backward()
    assert rel_err(xo, xr) < 1e-5 and rel_err(ho, hr) < 2e-5
    dt = torch.float64
    p64 = {k: t.detach().to(dt).clone().requires_grad_(True) for k, t in p.items()}
    x64, h64 = E.forward(p64, 2, x.to(dt), h.to(dt), ei, ea.to(dt), v.to(dt))
    (x64.pow(2).mean() + h64.pow(2).mean()).backward()
    bad = []
    for k, prm in m.named_parameters():
        assert prm.grad is not None and prm.grad.shape == prm.shape, k
        grad_check("egnn_narrow", k, prm.grad, p[k].grad, p64[k].grad, bad)
    assert not bad, bad


@pytest.mark.parametrize("act,q", [("relu", 0.0), ("leaky_relu", 0.2), ("gelu", 0.0), ("tanh", 0.0)])
def test_egnn_other_activation_vs_oracle(act, q):
    """`activation` other than SiLU on the EGNN sibling (basic.py:324; BaseMLP :181-192 puts it behind every first layer and
    behind the message MLP): the generic-activation library on the FASTEGNN_F_EGNN wiring, forward and every gradient."""
    from oracle import fastegnn_ref as R
    from tests.gpu_util import act_module
    cfg = R.Config(2, 0, 2, 64, 0, act=act, act_param=q)
    fn = R.act_of(cfg)
    g = torch.Generator().manual_seed(17)
    N, Ed = 1500, 18000
    torch.manual_seed(8)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, activation=act_module(cfg), device="cuda", with_v=True)
    p = {k: v.detach().cpu().clone().requires_grad_(True) for k, v in m.named_parameters()}
    x = torch.randn(N, 3, generator=g); h = torch.rand(N, 2, generator=g); v = torch.randn(N, 3, generator=g) * 0.2
    ei = torch.randint(0, N, (2, Ed), generator=g); ea = torch.rand(Ed, 2, generator=g)
    xo, _, ho = m(x=x.cuda(), h=h.cuda(), edge_index=ei.cuda(), edge_fea=ea.cuda(), v=v.cuda())
    (xo.pow(2).mean() + ho.pow(2).mean()).backward()
    xr, hr = E.forward(p, 2, x, h, ei, ea, v, act=fn)
    (xr.pow(2).mean() + hr.pow(2).mean()).backward()
    assert rel_err(xo, xr) < 1e-5 and rel_err(ho, hr) < 2e-5
    dt = torch.float64
    p64 = {k: t.detach().to(dt).clone().requires_grad_(True) for k, t in p.items()}
    x64, h64 = E.forward(p64, 2, x.to(dt), h.to(dt), ei, ea.to(dt), v.to(dt), act=fn)
    (x64.pow(2).mean() + h64.pow(2).mean()).backward()
    bad = []
    for k, prm in m.named_parameters():
        grad_check(f"egnn_act_{act}", k, prm.grad, p[k].grad, p64[k].grad, bad)
    assert not bad, bad


def _egnn_vs_oracle(case, m, x, h, ei, ea, v, want_gx=False):
    """one forward + backward of the module against oracle.egnn_ref in fp32 and fp64: outputs, every parameter gradient, d loss / d x -> its g_x"""
    p = {k: t.detach().cpu().clone() for k, t in m.named_parameters()}
    L = m.n_layers
    xg = x.cuda().requires_grad_(True)
    out = m(x=xg, h=h.cuda(), edge_index=ei.cuda(), edge_fea=ea.cuda(), v=None if v is None else v.cuda())
    xo, ho = out[0], out[-1]
    m.zero_grad(set_to_none=True)
    (xo.pow(2).mean() + ho.pow(2).mean()).backward()
    res = {}
    for dt in (torch.float32, torch.float64):
        pp = {k: t.to(dt).clone().requires_grad_(True) for k, t in p.items()}
        xx = x.to(dt).clone().requires_grad_(True)
        xr, hr = E.forward(pp, L, xx, h.to(dt), ei, ea.to(dt), None if v is None else v.to(dt), norm=m.norm)
        (xr.pow(2).mean() + hr.pow(2).mean()).backward()
        res[dt] = (xr.detach(), hr.detach(), {k: (t.grad if t.grad is not None else torch.zeros_like(t)) for k, t in pp.items()}, xx.grad)
    x32, h32, g32, gx32 = res[torch.float32]
    x64, h64, g64, gx64 = res[torch.float64]
    assert rel_err(xo, x32) < 1e-5 and rel_err(ho, h32) < 2e-5, (rel_err(xo, x32), rel_err(ho, h32))
    bad = []
    grad_check(case, "out/x", xo.detach().cpu(), x32, x64, bad)
    grad_check(case, "out/h", ho.detach().cpu(), h32, h64, bad)
    for k, prm in m.named_parameters():
        got = prm.grad.cpu() if prm.grad is not None else torch.zeros_like(prm).cpu()
        grad_check(case, k, got, g32[k], g64[k], bad)
    grad_check(case, "gin/x", xg.grad.cpu(), gx32, gx64, bad)
    assert not bad, bad
    return xg.grad


def test_egnn_deterministic_vs_oracle_and_repeatable_coordinate_gradient():
    """deterministic=True on the fused EGNN wiring (FASTEGNN_F_DETERMINISTIC | FASTEGNN_F_EGNN): every gradient against the oracle at 300 nodes,
    and the coordinate gradient -- the col-keyed sum the flag orders -- bit-identical over two backward passes"""
    g = torch.Generator().manual_seed(23)
    N, Ed = 300, 2400
    torch.manual_seed(13)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
    m.deterministic = True
    x = torch.randn(N, 3, generator=g); h = torch.rand(N, 2, generator=g); v = torch.randn(N, 3, generator=g) * 0.2
    ei = torch.randint(0, N, (2, Ed), generator=g); ea = torch.rand(Ed, 2, generator=g)
    gx = [_egnn_vs_oracle("test_egnn_deterministic", m, x, h, ei, ea, v) for _ in range(2)]
    assert m._spec.flags & fastegnn_amd._lib.F_DETERMINISTIC and m._spec.flags & fastegnn_amd._lib.F_EGNN
    assert torch.equal(gx[0].view(torch.int32), gx[1].view(torch.int32))


@pytest.mark.parametrize("with_v", [True, False], ids=["v", "nov"])
def test_egnn_single_node_without_edges_vs_oracle(with_v):
    g = torch.Generator().manual_seed(29)
    torch.manual_seed(14)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=with_v)
    x = torch.randn(1, 3, generator=g); h = torch.rand(1, 2, generator=g); v = torch.randn(1, 3, generator=g) if with_v else None
    _egnn_vs_oracle("test_egnn_single_node", m, x, h, torch.zeros(2, 0, dtype=torch.long), torch.zeros(0, 2), v)


def test_egnn_isolated_nodes_vs_oracle():
    """40 nodes of which the last 10 have no edge, neither as row nor as column: their mean over no message is zero, not a division by zero"""
    g = torch.Generator().manual_seed(31)
    torch.manual_seed(15)
    m = fastegnn_amd.EGNN(n_layers=2, in_node_nf=2, in_edge_nf=2, hidden_nf=64, device="cuda", with_v=True)
    N, Ed = 40, 200
    x = torch.randn(N, 3, generator=g); h = torch.rand(N, 2, generator=g)
    # the velocity leans along the position: the velocity head's scalar bias gradient, sum_n <g_x_out[n], v[n]> with g_x_out ~ x_out, is then a sum
    # of mostly positive terms.  With an independent v the 40 terms cancel, and the one number is compared relative to itself.
    v = torch.randn(N, 3, generator=g) * 0.2 + 0.3 * x
    ei = torch.randint(0, 30, (2, Ed), generator=g); ea = torch.rand(Ed, 2, generator=g)
    _egnn_vs_oracle("test_egnn_isolated_nodes", m, x, h, ei, ea, v)
