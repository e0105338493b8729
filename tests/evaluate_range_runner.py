"""Child process of tests/test_gpu_evaluate.py: fastegnn_amd.train.evaluate on a model whose hidden features leave the operand range of
the f16x2 build (the construction of tests/wide_range_runner.py); prints one JSON line.

    python -m tests.evaluate_range_runner <scale> [golden name]
"""
import json
import os
import sys
import warnings

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def main():
    scale = float(sys.argv[1])
    name = sys.argv[2] if len(sys.argv) > 2 else "c16_two_graphs"
    from fastegnn_amd import _lib as K
    from fastegnn_amd.train import evaluate
    from oracle import fastegnn_ref as R
    from tests.gpu_util import model_from_golden
    from tests.helpers import Golden, rel_err
    g = Golden(name)
    m = model_from_golden(g, device="cuda")
    with torch.no_grad():      # hidden features of ~scale: beyond fp16's range for scale >> 65 504
        m.embedding_in.weight.mul_(scale)
        m.embedding_in.bias.mul_(scale)
    kw, target, _ = g.model_kwargs(device="cuda")
    k = g.cfg.edge_attr_nf - 1           # evaluate() appends the edge length (utils/train.py:41-43): the golden's other edge features in front
    assert k >= 0 and kw.get("node_attr") is None
    base_ea = kw["edge_attr"][:, :k].contiguous() if k else None
    B = kw["loc_mean"].size(0)
    ptr = torch.searchsorted(kw["data_batch"], torch.arange(B + 1, device="cuda"))
    data = dict(loc_0=kw["node_loc"], vel_0=kw["node_vel"], loc_t=target, node_feat=kw["node_feat"], edge_index=kw["edge_index"],
                edge_attr=base_ea, batch=kw["data_batch"], loc_mean=kw["loc_mean"], ptr=ptr)
    loader = [data, data]
    outs = []
    m.register_forward_hook(lambda mod, args, out: outs.append(out[0].detach()))
    out = dict(lib=os.path.basename(K.LIB_PATH), B=B, wide_before=bool(m._range.wide))
    m.train()
    with warnings.catch_warnings(record=True) as wlist:
        warnings.simplefilter("always")
        r = evaluate(m, loader, 1.5, 0.3)
        evaluate(m, loader, 1.5, 0.3)       # a further epoch stays on the build the last one ended on, silently
    out["warned"] = sum("wide-range" in str(w.message) for w in wlist)
    out["training_restored"] = bool(m.training)
    out["passes"] = (len(outs) - len(loader)) // len(loader)      # of the first evaluate()
    out["wide"] = bool(m._range.wide)
    out.update(mse=r["mse"], loss=r["loss"], graphs=r["graphs"])
    out["finite"] = bool(torch.isfinite(torch.tensor([r["mse"], r["loss"]])).all())
    p = {n: v.detach().cpu() for n, v in m.state_dict().items()}
    loc, ei = kw["node_loc"].cpu(), kw["edge_index"].cpu()
    ea = R.augment_edge_attr(base_ea.cpu() if k else torch.zeros(ei.size(1), 0), loc, ei)
    rl, _ = R.forward(p, g.cfg, kw["node_feat"].cpu(), loc, kw["node_vel"].cpu(), ei, kw["data_batch"].cpu(), kw["loc_mean"].cpu(),
                      edge_attr=ea)
    out["ref_finite"] = bool(torch.isfinite(rl).all())
    out["err_loc"] = rel_err(outs[2 * len(loader) - 1].cpu(), rl) if out["finite"] else None
    ref_mse = float((rl.double() - target.cpu().double()).pow(2).mean())
    out["ref_mse"] = ref_mse
    # outputs within e = 1e-4 max|loc| of the oracle's (the bound tests/test_gpu_wide_range.py holds them to at this scale) move the mean
    # of squared errors by at most 2 e sqrt(mse) + e^2
    e = 1e-4 * float(rl.abs().max())
    out["mse_bound"] = 2 * e * ref_mse ** 0.5 + e * e
    print(json.dumps(out))


if __name__ == "__main__":
    main()
