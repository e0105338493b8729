"""Device-side training-step closure around the HIP FastEGNN.

Mirrors the body of the reference harness's mini-batch loop (``utils/train.py:30-170``): edge_attr
augmentation (:41-43), model call (:52), MSE + MMD loss (:104-165, with the sampled node indices passed
in explicitly instead of ``torch.randperm``), ``backward`` (:169) and Adam (``main_nbody.py:137``) --
each piece one C-ABI call of ``libfastegnn_hip.so``.
"""
from __future__ import annotations

import ctypes as C
from typing import Iterable, Optional

import torch

from . import _lib as K
from .model import _stream


def _capturing() -> bool:
    """is the current stream being captured into a HIP graph?  (False where there is no GPU: host-side state can always be written)"""
    return torch.cuda.is_available() and torch.cuda.is_current_stream_capturing()


def augment_edge_attr(edge_attr: Optional[torch.Tensor], loc_0: torch.Tensor, edge_index: torch.Tensor) -> torch.Tensor:
    """``cat([edge_attr, ||loc_0[row]-loc_0[col]||], 1)`` (utils/train.py:41-43)."""
    E = edge_index.size(1)
    k = edge_attr.size(1) if edge_attr is not None else 0
    out = torch.empty(E, k + 1, dtype=torch.float32, device=loc_0.device)
    ea = edge_attr.contiguous().float() if k else None
    K.check(K.lib().fastegnn_augment_edge_attr(K.ptr(edge_index.contiguous()), K.ptr(loc_0.contiguous().float()),
                                               K.ptr(ea), E, k, K.ptr(out), _stream(loc_0.device)),
            "fastegnn_augment_edge_attr")
    return out


class _MseMmd(torch.autograd.Function):
    @staticmethod
    def forward(ctx, loc_pred, vloc, loc_t, sample_nodes, sigma, weight, sample_count=None, ordered=False):
        dev = loc_pred.device
        loc_pred, vloc, loc_t = loc_pred.contiguous().float(), vloc.contiguous().float(), loc_t.contiguous().float()
        N, (B, _, Cn), S = loc_pred.size(0), vloc.shape, sample_nodes.size(1)
        loss2 = torch.empty(2, dtype=torch.float32, device=dev)
        g_loc, g_vloc = torch.empty_like(loc_pred), torch.empty_like(vloc)
        samp = sample_nodes.to(torch.int32).contiguous()          # no copy when it is int32 and contiguous already
        if sample_count is not None and sample_count.numel() != B:
            raise ValueError(f"fastegnn_amd.mse_mmd_loss: sample_count has {sample_count.numel()} entries for {B} graphs")
        if ordered:   # no floating-point atomics: the sums in a fixed order, over a workspace of workgroup partials
            cnt = sample_count.to(torch.int32).contiguous() if sample_count is not None else None
            ws = torch.empty(int(K.lib().fastegnn_loss_ordered_ws_doubles(N, B)), dtype=torch.float64, device=dev)
            K.check(K.lib().fastegnn_loss_mse_mmd_ordered(K.ptr(loc_pred), K.ptr(loc_t), K.ptr(vloc), K.ptr(samp), K.ptr(cnt), N, B, Cn, S,
                                                          float(sigma), float(weight), K.ptr(loss2), K.ptr(g_loc), K.ptr(g_vloc),
                                                          K.ptr(ws), ws.numel(), _stream(dev)), "fastegnn_loss_mse_mmd_ordered")
        elif sample_count is None:
            K.check(K.lib().fastegnn_loss_mse_mmd(K.ptr(loc_pred), K.ptr(loc_t), K.ptr(vloc), K.ptr(samp), N, B, Cn, S,
                                                  float(sigma), float(weight), K.ptr(loss2), K.ptr(g_loc), K.ptr(g_vloc),
                                                  _stream(dev)), "fastegnn_loss_mse_mmd")
        else:
            cnt = sample_count.to(torch.int32).contiguous()
            K.check(K.lib().fastegnn_loss_mse_mmd_ragged(K.ptr(loc_pred), K.ptr(loc_t), K.ptr(vloc), K.ptr(samp), K.ptr(cnt),
                                                         N, B, Cn, S, float(sigma), float(weight), K.ptr(loss2), K.ptr(g_loc),
                                                         K.ptr(g_vloc), _stream(dev)), "fastegnn_loss_mse_mmd_ragged")
        ctx.save_for_backward(g_loc, g_vloc)
        ctx.mark_non_differentiable(loss2)
        return loss2[0], loss2

    @staticmethod
    def backward(ctx, g, _g2):
        g_loc, g_vloc = ctx.saved_tensors
        return g * g_loc, g * g_vloc, None, None, None, None, None, None


def mse_mmd_loss(loc_pred, vloc, loc_t, sample_nodes, sigma, weight, sample_count=None, ordered=False):
    """-> (loss, mse): ``MSE(loc_pred, loc_t) + weight * (l_vv - l_rv)`` and the plain MSE the harness logs
    (utils/train.py:104-107,163-165).  ``sample_nodes`` [B,S]: absolute indices of the sampled real nodes.
    ``sample_count`` int32 [B] (``MMDSampler.draw``'s second result): row b holds that many valid entries and the rest is never read
    -- a graph smaller than the sample contributes all its nodes while l_rv keeps the divisor ``B * S * C``, as the reference's
    variable-size branch does (utils/train.py:121-142).  ``None``: every row is full.
    ``ordered=True``: the same numbers from fastegnn_loss_mse_mmd_ordered -- no floating-point atomics, every sum in an order fixed by
    the shapes and the counts, so two calls on the same inputs give the same bits (what ``deterministic = True`` promises for the rest of
    the step).  It relies on the entries of a row being distinct nodes (``MMDSampler``, ``torch.randperm``)."""
    loss, loss2 = _MseMmd.apply(loc_pred, vloc, loc_t, sample_nodes, sigma, weight, sample_count, bool(ordered))
    return loss, loss2[1]


def mse_mmd_eval(loc_pred, vloc, loc_t, acc, sigma, weight, sample_nodes=None, sample_count=None):
    """The loss of a forward-only batch, summed on the device (fastegnn_loss_mse_mmd_eval; utils/train.py:104-108,163-165 with
    backprop=False).  ``acc``: float64 [3] on the GPU, read and advanced: ``acc[0] += B * MSE`` (what the reference logs, train.py:107),
    ``acc[1] += B * (MSE + weight * (l_vv - l_rv))``, ``acc[2] += B``, with ``B = vloc.size(0)`` (or ``B = vloc`` where ``vloc`` is an int:
    a model without virtual nodes, no MMD term).  ``sample_nodes`` / ``sample_count`` as ``mse_mmd_loss``; ``sample_nodes=None``: the MMD
    term is not evaluated and ``acc[1]`` advances by ``B * MSE``.  No gradients, no read-back, no synchronisation; capturable; two runs
    from the same ``acc`` give the same bits.  -> ``acc``."""
    if not (isinstance(acc, torch.Tensor) and acc.is_cuda and acc.dtype == torch.float64 and acc.numel() == 3 and acc.is_contiguous()):
        raise ValueError("fastegnn_amd.mse_mmd_eval: acc must be a contiguous float64 tensor of 3 elements on the GPU")
    dev = loc_pred.device
    loc_pred, loc_t = loc_pred.detach().contiguous().float(), loc_t.detach().contiguous().float()
    N = loc_pred.size(0)
    if isinstance(vloc, torch.Tensor):
        vloc = vloc.detach().contiguous().float()
        B, Cn = vloc.size(0), vloc.size(2)
    else:
        B, Cn, vloc, sample_nodes = int(vloc), 0, None, None
    samp = cnt = None
    S = 0
    if sample_nodes is not None:
        S = sample_nodes.size(1)
        samp = sample_nodes.to(torch.int32).contiguous()
        if sample_count is not None:
            if sample_count.numel() != B:
                raise ValueError(f"fastegnn_amd.mse_mmd_eval: sample_count has {sample_count.numel()} entries for {B} graphs")
            cnt = sample_count.to(torch.int32).contiguous()
    K.check(K.lib().fastegnn_loss_mse_mmd_eval(K.ptr(loc_pred), K.ptr(loc_t), K.ptr(vloc), K.ptr(samp), K.ptr(cnt), N, B, Cn, S,
                                               float(sigma), float(weight), K.ptr(acc), _stream(dev)), "fastegnn_loss_mse_mmd_eval")
    return acc


def _u64(v):
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _i64(v):
    v = _u64(v)
    return v - (1 << 64) if v >= 1 << 63 else v


class MMDSampler:
    """The reference's per-graph ``torch.randperm(n_i)[:num_sample]`` (utils/train.py:130) drawn on the device (fastegnn_mmd_sample):
    a counter-based keyed permutation, so a draw is a function of ``(seed, counter, graph, position)`` alone.  ``seed`` and the draw
    ``counter`` live in device memory (two uint64); ``draw`` reads them there and a launch behind it advances the counter, so replays
    of a captured ``draw`` keep drawing fresh samples.  The output buffers are reused while ``(B, S)`` stay the same (a captured draw
    keeps its addresses; the next draw overwrites them).  A draw with another ``(B, S)`` makes new buffers and the sampler lets go of
    the old ones: a captured draw pins its ``(B, S)``, and whoever replays it keeps the tensors that ``draw`` returned during the
    capture alive for as long as the graph is, or uses one sampler per captured shape."""

    def __init__(self, seed, device=None):
        dev = torch.device("cuda" if device is None else device)
        if dev.type != "cuda":
            raise RuntimeError("fastegnn_amd.MMDSampler: the sample is drawn by a HIP kernel; there is no CPU fallback")
        if dev.index is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.MMDSampler: build the sampler before the stream capture")
        self.device = dev
        self._state = torch.tensor([_i64(seed), 0], dtype=torch.int64).to(dev)   # the bit patterns of {seed, counter}
        self._nodes = self._count = None

    def _read(self, i):
        return _u64(self._state[i].item())

    def _write(self, i, value):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.MMDSampler: seed and counter are written between replays, not inside a stream capture")
        self._state[i:i + 1].copy_(torch.tensor([_i64(value)], dtype=torch.int64))

    @property
    def seed(self):
        """(reading copies the word back: one synchronisation)"""
        return self._read(0)

    @seed.setter
    def seed(self, value):
        self._write(0, value)

    @property
    def counter(self):
        """draws taken with ``advance=True`` so far (reading copies the word back: one synchronisation)"""
        return self._read(1)

    @counter.setter
    def counter(self, value):
        self._write(1, value)

    def state_dict(self):
        seed, counter = self._state.tolist()
        return {"seed": _u64(seed), "counter": _u64(counter)}

    def load_state_dict(self, state):
        self.seed, self.counter = state["seed"], state["counter"]

    def draw(self, ptr, S, advance=True):
        """``ptr``: the batch's ``data['ptr']`` (int64 [B+1] on the device) -> ``(sample_nodes int32 [B,S], sample_count int32 [B])``:
        ``min(S, n_b)`` distinct nodes of every graph, the rest of a row -1.  Allocates nothing and reads nothing back once the
        buffers of this ``(B, S)`` exist.  The two tensors are the sampler's own buffers: the next draw of the same ``(B, S)`` overwrites
        them, and a draw of another ``(B, S)`` replaces them (a graph that captured this draw still writes the ones returned here, so
        keep them alive with the graph)."""
        if not (isinstance(ptr, torch.Tensor) and ptr.is_cuda and ptr.dtype == torch.int64 and ptr.dim() == 1 and ptr.numel() >= 1):
            raise RuntimeError("fastegnn_amd.MMDSampler.draw: ptr must be the int64 [B+1] graph offsets on the GPU (no CPU fallback)")
        if ptr.device != self.device:
            raise RuntimeError(f"fastegnn_amd.MMDSampler.draw: ptr lives on {ptr.device}, the sampler on {self.device}")
        B, S = ptr.numel() - 1, int(S)
        if self._nodes is None or tuple(self._nodes.shape) != (B, S):
            if torch.cuda.is_current_stream_capturing():
                raise RuntimeError("fastegnn_amd.MMDSampler: the output buffers of this (B, S) do not exist yet; run one eager "
                                   "draw (advance=False leaves the counter) before capturing it")
            self._nodes = torch.full((B, S), -1, dtype=torch.int32, device=self.device)
            self._count = torch.zeros(B, dtype=torch.int32, device=self.device)
        K.check(K.lib().fastegnn_mmd_sample(K.ptr(ptr.contiguous()), B, S, K.ptr(self._state), 1 if advance else 0,
                                            K.ptr(self._nodes), K.ptr(self._count), _stream(self.device)), "fastegnn_mmd_sample")
        return self._nodes, self._count


class FusedAdam:
    """``torch.optim.Adam(params, lr, weight_decay)`` semantics (main_nbody.py:137) as multi-tensor HIP launches.

    ``capturable=True`` (as ``torch.optim.Adam(capturable=True)``): the step counts, the hyper-parameters and the decision to skip
    live in DEVICE memory (fastegnn_adam_step_dev), so ``step()`` reads nothing back, synchronises nothing and may be captured
    into a HIP graph whose replays then train:

    * ``opt.lr = x`` / ``opt.set_lr(x)`` write the device buffer with a stream-ordered copy (outside a capture); the next replay
      uses the new value, nothing is re-captured;
    * ``opt.steps`` copies the counts back (one synchronisation: tests and checkpoints);
    * ``opt.skip_word``: a device int32 tensor or the address of a device / host-mapped word; while the word is non-zero a step
      moves NOTHING (parameters, moments, counts), a loss scaler's skipped step.  ``opt.attach_guard(model)`` uses the OUT word
      of the model's RangeGuard for as long as the model runs on the f16x2 build: the step that follows an overflowed forward
      is skipped on the device, whenever the host learns of it;
    * ``max_grad_norm``: ``torch.nn.utils.clip_grad_norm_``'s coefficient, applied to the gradients as they are read (the
      ``.grad`` buffers are not rewritten); a step whose gradient norm is not finite is skipped like one with a set word.

    Which parameters have a gradient is read from ``p.grad`` when ``step()`` is CALLED: a captured step freezes that set (and the
    gradient addresses) as they were at capture time.  The default ``capturable=False`` is the host-side path, unchanged."""

    def __init__(self, params: Iterable[torch.nn.Parameter], lr=5e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0,
                 capturable=False, max_grad_norm=None):
        if max_grad_norm is not None and not capturable:
            raise ValueError("fastegnn_amd.FusedAdam: max_grad_norm needs capturable=True (the clipped step is the device-side one)")
        self.capturable = bool(capturable)
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self._dev = None                       # device buffers of the capturable path (_ensure_device)
        self._guard = None
        self._skip_keep = None
        self._skip_addr = None
        self.params = [p for p in params if p.requires_grad]
        self._lr = lr
        self.betas, self.eps, self.weight_decay = betas, eps, weight_decay
        self.exp_avg = [torch.zeros_like(p) for p in self.params]
        self.exp_avg_sq = [torch.zeros_like(p) for p in self.params]
        self.step_count = 0                    # calls of step()
        n = len(self.params)
        # torch.optim.Adam's state['step'] of each parameter: advanced only on the steps where it has a .grad, and its
        # bias correction follows its own count (a parameter first reached at step 2 is corrected as at step 1)
        self._steps = [0] * n
        self._numel = (C.c_int64 * n)(*[p.numel() for p in self.params])
        self._m = (C.c_void_p * n)(*[t.data_ptr() for t in self.exp_avg])
        self._v = (C.c_void_p * n)(*[t.data_ptr() for t in self.exp_avg_sq])
        if self.capturable and self.params and self.params[0].is_cuda:
            self._ensure_device(self.params[0].device)

    # ---- state that lives on the device when capturable ----
    @property
    def lr(self):
        return self._lr

    @lr.setter
    def lr(self, value):
        self.set_lr(value)

    def set_lr(self, value):
        self._lr = float(value)
        if self._dev is not None:
            self._write_hyper()

    @property
    def steps(self):
        """per-parameter step counts (capturable: copied back from the device, which synchronises)"""
        if self.capturable and self._dev is not None:
            return [int(v) for v in self._dev["steps"].tolist()]
        return self._steps

    @property
    def skip_word(self):
        return self._skip_keep if self._skip_keep is not None else self._skip_addr

    @skip_word.setter
    def skip_word(self, word):
        if word is not None and not self.capturable:
            raise ValueError("fastegnn_amd.FusedAdam: skip_word needs capturable=True")
        self._skip_keep, self._skip_addr = None, None
        if isinstance(word, torch.Tensor):
            if word.dtype != torch.int32 or not word.is_cuda or word.numel() < 1:
                raise ValueError("fastegnn_amd.FusedAdam: skip_word as a tensor must be an int32 tensor on the GPU")
            self._skip_keep, self._skip_addr = word, word.data_ptr()
        elif word is not None:
            self._skip_addr = word.value if isinstance(word, C.c_void_p) else int(word)

    def attach_guard(self, model):
        """skip by the OUT word of ``model``'s RangeGuard (host-mapped; allocated by the model's first eager forward)"""
        guard = getattr(model, "_range", None)
        if guard is None or not self.capturable:
            raise ValueError("fastegnn_amd.FusedAdam.attach_guard: needs capturable=True and a module with a range guard")
        self._guard = guard

    def _skip_ptr(self):
        if self._skip_addr is not None:
            return C.c_void_p(self._skip_addr)
        guard = self._guard
        # on the wide-range build no guard launch runs any more and the words are dead (OUT stays set after the switch)
        if guard is None or guard.wide:
            return None
        if guard._words is None and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.FusedAdam: the range guard's host-mapped words do not exist yet; run one eager forward "
                               "of the module before capturing the step into a HIP graph")
        return guard.word_ptr(guard.OUT)

    def _write_hyper(self):
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.FusedAdam: hyper-parameters are written between replays, not inside a stream capture")
        h = [self._lr, self.betas[0], self.betas[1], self.eps, self.weight_decay,
             self.max_grad_norm if self.max_grad_norm is not None else 0.0]
        self._dev["hyper"].copy_(torch.tensor(h, dtype=torch.float64))

    def _ensure_device(self, dev):
        d = self._dev
        if d is not None and d["hyper"].device == dev:
            return
        if torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.FusedAdam: build the capturable optimizer on the GPU parameters (or run one eager "
                               "step) before capturing it")
        n = len(self.params)
        L = K.lib()
        steps = torch.tensor(d["steps"].tolist() if d is not None else self._steps, dtype=torch.int32).reshape(n).to(dev)
        self._dev = dict(
            steps=steps, hyper=torch.zeros(6, dtype=torch.float64, device=dev),
            sqnorm=torch.zeros(1, dtype=torch.float64, device=dev),
            sqn_ws=torch.zeros(max(int(L.fastegnn_grad_sqnorm_partials(self._numel, n)), 1), dtype=torch.float64, device=dev),
            scratch=torch.zeros((int(L.fastegnn_adam_dev_scratch_bytes(n)) + 3) // 4, dtype=torch.float32, device=dev))
        self._write_hyper()

    @property
    def n_partials(self) -> int:
        """workgroup partials the gradient-norm reduction sums (fastegnn_grad_sqnorm_partials)"""
        return int(K.lib().fastegnn_grad_sqnorm_partials(self._numel, len(self.params)))

    @property
    def grad_sqnorm(self) -> torch.Tensor:
        """the device scalar (fp64) the latest clipped step reduced the squared gradient norm into"""
        return self._dev["sqnorm"]

    def zero_grad(self):
        for p in self.params:
            p.grad = None

    # ---- checkpoints: torch.optim.Adam's state_dict layout, so that either optimizer loads the other's ----
    def state_dict(self) -> dict:
        """``{"state": {i: {"step", "exp_avg", "exp_avg_sq"}}, "param_groups": [{lr, betas, eps, weight_decay, ..., "params": [0..n-1]}]}``
        as ``torch.optim.Adam.state_dict()`` lays it out (``step`` a float32 scalar tensor on the host, as torch keeps it), with
        ``max_grad_norm``, ``capturable`` and ``step_count`` added to the group: ``torch.optim.Adam(params).load_state_dict(...)`` takes it.
        Every parameter has an entry (a parameter that never had a gradient: step 0, zero moments).  The moments are copies.  In
        capturable mode the step counts are read from the device: ONE synchronisation, refused inside a stream capture."""
        if self.capturable and self._dev is not None and _capturing():
            raise RuntimeError("fastegnn_amd.FusedAdam: state_dict() reads the step counts back from the device, which a stream capture "
                               "cannot do; save between replays")
        steps = self.steps
        state = {i: {"step": torch.tensor(float(steps[i]), dtype=torch.float32),
                     "exp_avg": self.exp_avg[i].detach().clone(), "exp_avg_sq": self.exp_avg_sq[i].detach().clone()}
                 for i in range(len(self.params))}
        group = dict(lr=float(self._lr), betas=(float(self.betas[0]), float(self.betas[1])), eps=float(self.eps),
                     weight_decay=float(self.weight_decay), amsgrad=False, maximize=False, foreach=None, capturable=self.capturable,
                     differentiable=False, fused=None, decoupled_weight_decay=False, max_grad_norm=self.max_grad_norm,
                     step_count=int(self.step_count), params=list(range(len(self.params))))
        return {"state": state, "param_groups": [group]}

    def load_state_dict(self, state_dict) -> None:
        """The inverse, also of ``torch.optim.Adam.state_dict()`` over the same parameter list.  A parameter without a state entry gets
        zero state.  Everything is checked first -- one parameter group, the parameter count, every shape: a mismatch is a ``ValueError``
        that names the index and leaves the optimizer as it was -- and then written IN PLACE: ``copy_`` into the existing moment tensors
        and into the existing device buffers of the step counts and the hyper-parameters, so that the pointer tables, and a HIP graph
        that captured ``step()``, stay valid and continue from the loaded state.  ``capturable`` stays what this optimizer was built
        with (a checkpoint of either mode loads into either); ``max_grad_norm`` follows the checkpoint when it names one.  Never inside
        a stream capture."""
        if _capturing():
            raise RuntimeError("fastegnn_amd.FusedAdam: load_state_dict() writes the optimizer state between replays, not inside a "
                               "stream capture")
        groups = state_dict["param_groups"]
        if len(groups) != 1:
            raise ValueError(f"fastegnn_amd.FusedAdam.load_state_dict: {len(groups)} parameter groups; this optimizer has one")
        group, n = groups[0], len(self.params)
        ids = list(group["params"])
        if len(ids) != n:
            raise ValueError(f"fastegnn_amd.FusedAdam.load_state_dict: the state holds {len(ids)} parameters, the optimizer {n}")
        saved = state_dict.get("state", {})
        unknown = [k for k in saved if k not in ids]
        if unknown:
            raise ValueError(f"fastegnn_amd.FusedAdam.load_state_dict: state entries {unknown} name no parameter of the group")
        entries, steps = [], []
        for i, (pid, p) in enumerate(zip(ids, self.params)):
            e = saved.get(pid)
            if e is not None:
                for key in ("exp_avg", "exp_avg_sq"):
                    if tuple(e[key].shape) != tuple(p.shape):
                        raise ValueError(f"fastegnn_amd.FusedAdam.load_state_dict: {key} of parameter {i} has shape "
                                         f"{list(e[key].shape)}, the parameter {list(p.shape)}")
                step = float(e["step"])
                if step < 0 or step != int(step):
                    raise ValueError(f"fastegnn_amd.FusedAdam.load_state_dict: step of parameter {i} is {step}")
            entries.append(e)
            steps.append(int(float(e["step"])) if e is not None else 0)
        max_grad_norm = group.get("max_grad_norm", self.max_grad_norm)
        if max_grad_norm is not None and not self.capturable:
            raise ValueError("fastegnn_amd.FusedAdam.load_state_dict: the state clips at max_grad_norm, which needs capturable=True")
        with torch.no_grad():
            for i, e in enumerate(entries):
                if e is None:
                    self.exp_avg[i].zero_(); self.exp_avg_sq[i].zero_()
                else:
                    self.exp_avg[i].copy_(e["exp_avg"]); self.exp_avg_sq[i].copy_(e["exp_avg_sq"])
        self._steps[:] = steps
        self._lr = float(group["lr"])
        self.betas = (float(group["betas"][0]), float(group["betas"][1]))
        self.eps, self.weight_decay = float(group["eps"]), float(group["weight_decay"])
        self.max_grad_norm = None if max_grad_norm is None else float(max_grad_norm)
        self.step_count = int(group.get("step_count", max(steps, default=0)))
        if self._dev is not None:
            self._dev["steps"].copy_(torch.tensor(steps, dtype=torch.int32).reshape(n))
            self._write_hyper()

    def step(self):
        self.step_count += 1
        n = len(self.params)
        grads = []
        for p in self.params:
            g = p.grad
            if g is not None and (not g.is_contiguous() or g.dtype != torch.float32):
                g = g.contiguous().float()
            grads.append(g)
            if g is not None and not self.capturable:
                self._steps[len(grads) - 1] += 1
        gp = (C.c_void_p * n)(*[(g.data_ptr() if g is not None else None) for g in grads])
        dev = self.params[0].device
        # parameter pointers are read at every step: a model moved with .to() / .cuda() after the optimizer was built
        # has new storages (the moments follow the device of the parameters)
        pp = (C.c_void_p * n)(*[p.data_ptr() for p in self.params])
        for i, p in enumerate(self.params):
            if self.exp_avg[i].device != p.device:
                self.exp_avg[i], self.exp_avg_sq[i] = self.exp_avg[i].to(p.device), self.exp_avg_sq[i].to(p.device)
                self._m[i], self._v[i] = self.exp_avg[i].data_ptr(), self.exp_avg_sq[i].data_ptr()
        if self.capturable:
            return self._step_device(pp, gp, n, dev)
        steps = (C.c_int32 * n)(*self._steps)
        K.check(K.lib().fastegnn_adam_step_v2(pp, gp, self._m, self._v, self._numel, n, steps,
                                              float(self.lr), float(self.betas[0]), float(self.betas[1]),
                                              float(self.eps), float(self.weight_decay), _stream(dev)),
                "fastegnn_adam_step_v2")

    def _step_device(self, pp, gp, n, dev):
        """queue the device-side step: no host read, no synchronisation (legal inside a stream capture)"""
        self._ensure_device(dev)
        d, L, st = self._dev, K.lib(), _stream(dev)
        clip = self.max_grad_norm is not None
        if clip:
            K.check(L.fastegnn_grad_sqnorm(gp, self._numel, n, K.ptr(d["sqn_ws"]), d["sqn_ws"].numel(), K.ptr(d["sqnorm"]), st),
                    "fastegnn_grad_sqnorm")
        K.check(L.fastegnn_adam_step_dev(pp, gp, self._m, self._v, self._numel, n, K.ptr(d["steps"]), K.ptr(d["hyper"]),
                                         K.ptr(d["sqnorm"]) if clip else None, self._skip_ptr(), K.ptr(d["scratch"]),
                                         d["scratch"].numel() * 4, st), "fastegnn_adam_step_dev")


def _graph_or_edges(data):
    """what the model gets as ``edge_index``: the batch's ready ``SortedGraph`` (``data['graph']``, data.PackedLoader(graphs=...)) when
    there is one -- the model then sorts nothing -- else the int64 edge list"""
    graph = data.get("graph")
    return graph if graph is not None else data["edge_index"]


def _ordered_mode(model) -> bool:
    """is the model's ordered mode on?  ``model.deterministic`` on the fused modules, ``wide._ordered_of(model)`` on the wide path: the
    loss then takes its ordered form as well, so that the whole step is free of floating-point atomics where the model is"""
    if getattr(model, "_wide", False):
        from . import wide
        return wide._ordered_of(model) is not None
    return bool(getattr(model, "deterministic", False))


def _forward_backward(model, optimizer, data: dict, sample_nodes, sigma, weight, sample_count=None):
    """augment + forward + MSE/MMD + backward of one iteration (everything of train_step in front of the optimizer)"""
    edge_attr = augment_edge_attr(data.get("edge_attr"), data["loc_0"], data["edge_index"])
    optimizer.zero_grad()
    loc_pred, vloc = model(node_loc=data["loc_0"], node_vel=data["vel_0"], node_attr=None,
                           node_feat=data["node_feat"], edge_index=_graph_or_edges(data), loc_mean=data["loc_mean"],
                           data_batch=data["batch"], edge_attr=edge_attr)
    loss, mse = mse_mmd_loss(loc_pred, vloc, data["loc_t"], sample_nodes, sigma, weight, sample_count, ordered=_ordered_mode(model))
    loss.backward()
    return loss.detach(), mse


def train_step(model, optimizer: FusedAdam, data: dict, sample_nodes, sigma, weight, *, sampler: Optional[MMDSampler] = None,
               num_sample: Optional[int] = None):
    """One iteration of utils/train.py:30-170 for the FastEGNN branch.  ``data`` holds the collated batch
    (loc_0, vel_0, loc_t, node_feat, edge_index, edge_attr, batch, loc_mean) on the GPU.  Returns (loss, mse).
    With ``sampler`` (and ``sample_nodes=None``) the step draws its own sample on the device: ``min(num_sample, N)`` nodes per graph
    from ``data['ptr']`` (utils/train.py:116-130), a smaller graph all of its nodes, and the loss takes the per-graph counts."""
    sample_count = None
    if sampler is not None and sample_nodes is None:
        if num_sample is None:
            raise ValueError("fastegnn_amd.train_step: a sampler needs num_sample (the reference's sample * C)")
        sample_nodes, sample_count = sampler.draw(data["ptr"], min(int(num_sample), data["loc_0"].size(0)))
    elif sample_nodes is None:
        raise ValueError("fastegnn_amd.train_step: sample_nodes is None and there is no sampler to draw them")
    loss, mse = _forward_backward(model, optimizer, data, sample_nodes, sigma, weight, sample_count)
    # the range guard of the f16x2 build (fastegnn_amd.model.RangeGuard), polled without synchronisation: when THIS poll finds that a
    # pass left the fp16 operand range the module moves to the wide-range build and the update is skipped (its gradients were zeroed
    # on the device anyway), like a skipped step of a loss scaler
    guard = getattr(model, "_range", None)
    if guard is not None and guard.poll(type(model).__name__, getattr(model, "_plist", None), why="a training step"):
        return loss, mse
    optimizer.step()
    return loss, mse


def _predict(model, data, edge_attr):
    """the model call of a forward-only pass on the batch ``data`` with its augmented ``edge_attr`` -> (loc_pred, vloc); ``EGNN`` is
    called by its own signature (utils/train.py:66-68) and has no virtual nodes: vloc is None.  (``evaluate`` and ``rollout``)"""
    if type(model).__name__ == "EGNN":
        out = model(x=data["loc_0"], h=data["node_feat"], edge_index=_graph_or_edges(data), edge_fea=edge_attr, v=data["vel_0"])
        return out[0], None
    return model(node_loc=data["loc_0"], node_vel=data["vel_0"], node_attr=None, node_feat=data["node_feat"],
                 edge_index=_graph_or_edges(data), loc_mean=data["loc_mean"], data_batch=data["batch"], edge_attr=edge_attr)


def _evaluate_pass(model, loader, sigma, weight, sampler, num_sample):
    """one forward-only sweep over the loader -> the device accumulator (None for an empty loader); nothing is read back"""
    acc = None
    egnn = type(model).__name__ == "EGNN"
    for data in loader:
        loc_0 = data["loc_0"]
        if acc is None:
            acc = torch.zeros(3, dtype=torch.float64, device=loc_0.device)
        edge_attr = augment_edge_attr(data.get("edge_attr"), loc_0, data["edge_index"])
        loc_pred, vloc = _predict(model, data, edge_attr)
        if egnn:   # no virtual nodes, no MMD term
            n_graphs = data["ptr"].numel() - 1 if "ptr" in data else data["loc_mean"].size(0)
            mse_mmd_eval(loc_pred, n_graphs, data["loc_t"], acc, sigma, weight)
            continue
        nodes = count = None
        if sampler is not None:
            nodes, count = sampler.draw(data["ptr"], min(int(num_sample), loc_0.size(0)))
        mse_mmd_eval(loc_pred, vloc, data["loc_t"], acc, sigma, weight, nodes, count)
    return acc


def evaluate(model, loader, sigma, weight, *, sampler: Optional[MMDSampler] = None, num_sample: Optional[int] = None) -> dict:
    """The reference's ``train_single_epoch(..., backprop=False)`` (utils/train.py:23-179: its validation and test epochs) ->
    ``dict(mse=, loss=, graphs=)``.  ``loader`` yields the collated batches ``train_step`` takes.  The model is put into ``eval()`` (its
    previous mode is restored) and runs under ``torch.no_grad()`` -- the fused models then take their forward-only path, on one reused
    set of stage buffers -- and every batch adds its loss into three fp64 words on the device (``mse_mmd_eval``): ONE read-back, after
    the last batch.  ``mse`` is the graph-weighted mean MSE, the number the reference prints and early-stops on; ``loss`` adds the MMD
    term when a ``sampler`` (with ``num_sample``, the reference's ``sample * C``) draws the nodes for it -- without one the term is
    skipped and ``loss == mse`` (the reference computes it in these epochs and throws it away).
    After the read-back the model's range guard is polled once: if a batch left the operand range of the f16x2 build the module has
    moved to the wide-range build (one warning, fastegnn_amd.model.RangeGuard), and the loader is run ONCE more on that build and that
    result returned (a sampler draws fresh samples for it); still non-finite numbers are returned as they are."""
    if sampler is not None and num_sample is None:
        raise ValueError("fastegnn_amd.evaluate: a sampler needs num_sample (the reference's sample * C)")
    guard = getattr(model, "_range", None)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            wide_before = guard.wide if guard is not None else True
            acc = _evaluate_pass(model, loader, sigma, weight, sampler, num_sample)
            if acc is None:
                return dict(mse=float("nan"), loss=float("nan"), graphs=0)
            host = acc.tolist()   # the one synchronisation of the epoch
            if guard is not None and not wide_before:
                guard.poll(type(model).__name__, getattr(model, "_plist", None), why="a forward-only epoch (evaluate)")
                if guard.wide:    # switched by this poll or by a forward of the sweep: some batch returned non-finite outputs
                    host = _evaluate_pass(model, loader, sigma, weight, sampler, num_sample).tolist()
    finally:
        model.train(was_training)
    return dict(mse=host[0] / host[2], loss=host[1] / host[2], graphs=int(host[2]))


def train_epoch(model, optimizer: FusedAdam, loader, sigma, weight, *, sampler: Optional[MMDSampler] = None,
                num_sample: Optional[int] = None, sample_nodes=None) -> dict:
    """The reference's ``train_single_epoch(..., backprop=True)`` (utils/train.py:23-179: its training epoch) -> ``dict(mse=, loss=,
    graphs=)``.  The model is put into ``train()`` and every batch of ``loader`` -- a ``DataLoader``, ``PackedLoader`` or ``PackedStream``:
    anything that yields the batches ``train_step`` takes -- runs one ``train_step`` with the arguments given here.  Each step's
    ``(loss, mse)`` is added into three fp64 words on the device, weighted by the batch's graph count ``data['loc_mean'].size(0)``
    (fastegnn_loss_accumulate; the words of ``mse_mmd_eval``): ONE read-back, after the last batch, where a hand-written loop pays
    one ``.item()`` per batch to log its loss.  ``mse`` is the graph-weighted mean MSE of the epoch, the number the reference prints;
    ``loss`` the same mean of the full objective.  An empty loader returns NaNs and ``graphs=0``, like ``evaluate``."""
    model.train()
    acc = None
    for data in loader:
        loss, mse = train_step(model, optimizer, data, sample_nodes, sigma, weight, sampler=sampler, num_sample=num_sample)
        dev = loss.device
        if acc is None:
            acc = torch.zeros(3, dtype=torch.float64, device=dev)
        K.check(K.lib().fastegnn_loss_accumulate(K.ptr(loss), K.ptr(mse), data["loc_mean"].size(0), K.ptr(acc), _stream(dev)),
                "fastegnn_loss_accumulate")
    if acc is None:
        return dict(mse=float("nan"), loss=float("nan"), graphs=0)
    host = acc.tolist()   # the one synchronisation of the epoch
    return dict(mse=host[0] / host[2], loss=host[1] / host[2], graphs=int(host[2]))
