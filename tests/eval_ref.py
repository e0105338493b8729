"""float64 restatements for the forward-only tests (tests/test_inference_plan_cpu.py, tests/test_gpu_evaluate.py,
tests/test_gpu_inference.py): the reference's validation epoch, utils/train.py:23-179 with backprop=False, with the sampled node
indices passed in where the reference draws torch.randperm.
"""
import torch


def kernel(x, y, sigma):
    """utils/train.py:17-20, with the distance written out (torch.cdist's matmul form above 25 points is less accurate)"""
    dist = (x[..., :, None, :] - y[..., None, :, :]).pow(2).sum(-1).sqrt()
    return torch.exp(-dist / (2 * sigma * sigma))


def batch_loss_fp64(loc_pred, vloc, loc_t, samp, cnt, sigma, weight):
    """-> (mse, loss) of one batch in float64.  loc_pred / loc_t [N,3], vloc [B,3,C]; samp [B,S] absolute node ids or None (no MMD
    term: loss == mse, as with S == 0); cnt [B] or None.
    cnt given: the variable-size branch, utils/train.py:118-142 -- graph i contributes its cnt[i] <= S sampled nodes and l_rv is divided
    by batch_size * num_sample * C whatever the counts.  cnt None: the equal-size branch, :144-161, every row full."""
    dt = torch.float64
    x, t = loc_pred.detach().cpu().to(dt), loc_t.detach().cpu().to(dt)
    mse = torch.nn.functional.mse_loss(x, t)                              # :104
    if samp is None or samp.size(1) == 0:
        return mse, mse.clone()
    V = vloc.detach().cpu().to(dt).permute(0, 2, 1)                       # :114  [B, C, 3]
    samp = samp.detach().cpu().long()
    B, C = V.size(0), V.size(1)
    S = samp.size(1)
    if cnt is not None:
        cnt = cnt.detach().cpu().long()
        l_vv, l_rv = torch.zeros((), dtype=dt), torch.zeros((), dtype=dt)
        for i in range(B):                                                # :122-138
            nodes = x[samp[i, :int(cnt[i])]]
            l_vv = l_vv + kernel(V[i], V[i], sigma).sum()
            l_rv = l_rv + kernel(nodes, V[i], sigma).sum()
        l_vv = l_vv / B / C / C                                           # :141
        l_rv = 2 * l_rv / B / S / C                                       # :142
    else:
        nodes = x[samp.reshape(-1)].reshape(B, S, 3)                      # :153
        l_vv = kernel(V, V, sigma).sum() / B / C / C                      # :160
        l_rv = 2 * kernel(nodes, V, sigma).sum() / B / S / C              # :161
    return mse, mse + weight * (l_vv - l_rv)                              # :163-165


def acc_step(acc, n_graphs, mse, loss):
    """the recurrence of fastegnn_loss_mse_mmd_eval on a float64 [3] tensor (include/fastegnn_hip.h)"""
    acc = acc.clone()
    acc[0] += n_graphs * mse
    acc[1] += n_graphs * loss
    acc[2] += n_graphs
    return acc
