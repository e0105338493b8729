"""Device-side rollouts: a trained model is fed its own prediction, step after step, and every step is scored
against the trajectory's own frame.  The reference has no rollout; the semantics are the project's own and are stated once, in
include/fastegnn_hip.h ("rollouts") and DESIGN.md.

A step is: ``augment_edge_attr`` + the model's forward (its forward-only path under ``no_grad``) + the TWO launches of the state update
(csrc/rollout.hip: ``advance`` over the nodes, ``graph`` per cloud) + the batched radius graph of the new positions.  The state update
uses the rounding rules the model was trained on through ``TrajectoryLoader``: ``node_feat[:,0]`` by ``fastegnn_traj_gather``'s rule,
``loc_mean`` by ``fastegnn_traj_mean``'s.  The only synchronisation of a step is the graph build's read-back of its edge counts; the
error sums stay on the device until ``result()``.
"""
from __future__ import annotations

import ctypes as C
from typing import Optional

import numpy as np
import torch

from . import data as D
from . import train as T

_NO_CPU_ROLLOUT = "fastegnn_amd: a rollout needs device-resident state (there is no CPU fallback)"


class HipRolloutOps:
    """The device calls of a rollout on libfastegnn_hip.so (the product path): ``plan``, ``advance`` and ``graph`` are the launches of
    csrc/rollout.hip (include/fastegnn_hip.h, fastegnn_rollout_*), ``graph_moved`` is ``graph`` for a dataset with rigid motions
    (its truth rows are moved first), ``augment`` is ``train.augment_edge_attr``.  tests/rollout_ref.py
    restates them in torch, so that tests/test_rollout_cpu.py can drive the orchestration without a GPU (the ``HipTrajOps`` precedent)."""

    @staticmethod
    def plan(ids, samples, traj_row0, traj_n, traj_T, delta_t, truth_rows) -> None:
        """truth_rows int64 [steps,B] <- per step k and slot b the first row in ``pos`` of frame f + (k+1) delta_t, -1 beyond T"""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU_ROLLOUT)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_rollout_plan(K.ptr(ids), ids.numel(), K.ptr(samples), samples.size(0), K.ptr(traj_row0), K.ptr(traj_n),
                                              K.ptr(traj_T), traj_n.numel(), int(delta_t), truth_rows.size(0), K.ptr(truth_rows),
                                              _stream(ids.device)), "fastegnn_rollout_plan")

    @staticmethod
    def advance(x_new, delta_t, loc, vel, node_feat, record, flag) -> None:
        """vel, node_feat[:,0], loc <- the state after the prediction ``x_new``; ``record`` (None or [N,3]) <- x_new; ``flag`` (a
        ``FlagWord``) <- 1 when a component of x_new is not finite (that component keeps loc and gets vel 0)"""
        if not x_new.is_cuda:
            raise RuntimeError(_NO_CPU_ROLLOUT)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_rollout_advance(K.ptr(x_new), x_new.size(0), int(delta_t), K.ptr(loc), K.ptr(vel), K.ptr(node_feat),
                                                 K.ptr(record), flag.address, _stream(x_new.device)), "fastegnn_rollout_advance")

    @staticmethod
    def graph(ptr, loc, x_new, pos, truth_rows, loc_mean, sse) -> None:
        """loc_mean [B,3,C] <- per cloud the fp64 mean of ``loc``, rounded once; ``sse`` (None or float64 [B]) <- per cloud the fp64 sum
        of squares of ``x_new`` minus the rows ``truth_rows[b] ..`` of ``pos``, NaN where there is no truth frame"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_ROLLOUT)
        from . import _lib as K
        from .model import _stream
        score = sse is not None
        K.check(K.lib().fastegnn_rollout_graph(K.ptr(ptr), ptr.numel() - 1, K.ptr(loc), K.ptr(x_new) if score else None, loc.size(0),
                                               K.ptr(pos) if score else None, pos.size(0) if score else 0,
                                               K.ptr(truth_rows) if score else None, loc_mean.size(2), K.ptr(loc_mean), K.ptr(sse),
                                               _stream(ptr.device)), "fastegnn_rollout_graph")

    @staticmethod
    def graph_moved(ptr, loc, x_new, pos, truth_rows, loc_mean, sse, motion, has_t) -> None:
        """``graph`` with a score against MOVED truth: graph b's truth rows are moved by ``motion[b]`` (fp32 [B,12]: R row-major, then
        t; ``has_t`` false: no translation is added) in fp32 by the rule of ``data.apply_motion`` before the fp64 difference"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_ROLLOUT)
        B = ptr.numel() - 1
        if not (motion.is_cuda and motion.dtype == torch.float32 and tuple(motion.shape) == (B, 12) and motion.is_contiguous()):
            raise ValueError(f"fastegnn_amd: the motion rows of a rollout of {B} samples must be a contiguous device fp32 [{B},12] tensor")
        from . import _lib as K
        from .model import _stream
        score = sse is not None
        K.check(K.lib().fastegnn_rollout_graph_moved(K.ptr(ptr), B, K.ptr(loc), K.ptr(x_new) if score else None, loc.size(0),
                                                     K.ptr(pos) if score else None, pos.size(0) if score else 0,
                                                     K.ptr(truth_rows) if score else None, loc_mean.size(2), K.ptr(loc_mean), K.ptr(sse),
                                                     K.ptr(motion), int(bool(has_t)), _stream(ptr.device)), "fastegnn_rollout_graph_moved")

    @staticmethod
    def augment(edge_attr, loc_0, edge_index):
        return T.augment_edge_attr(edge_attr, loc_0, edge_index)


_ROLLOUT_OPS = HipRolloutOps


class FlagWord:
    """One int32 word the ``advance`` launch stores 1 into: on a GPU a host-mapped word of the range guard's allocator
    (fastegnn_host_words_alloc), which the host reads with a plain load once a synchronisation it pays anyway has passed; elsewhere (the
    torch restatement of the tests) a word of host memory.  Released only after a synchronisation of the device's current stream."""

    def __init__(self, device):
        self.device = torch.device(device)
        self._mapped = self.device.type == "cuda"
        if self._mapped:
            from . import _lib as K
            self._words = C.POINTER(C.c_int32)()
            K.check(K.lib().fastegnn_host_words_alloc(1, C.byref(self._words)), "fastegnn_host_words_alloc")
        else:
            self._words = (C.c_int32 * 1)()

    @property
    def address(self) -> C.c_void_p:
        return C.c_void_p(C.addressof(self._words.contents if self._mapped else self._words))

    def get(self) -> int:
        return int(self._words[0])

    def set(self, value: int) -> None:
        self._words[0] = int(value)

    def release(self) -> None:
        words, self._words = self._words, None
        if words is not None and self._mapped:
            from . import _lib as K
            torch.cuda.current_stream(self.device).synchronize()   # no launch that stores into the word may still be queued
            K.lib().fastegnn_host_words_free(words)

    def __del__(self):
        try:
            self.release()
        except Exception:
            pass


class Rollout:
    """``steps`` steps of ``model`` on the samples ``ids`` of the ``TrajectoryDataset`` ``ds`` (stride ``ds.delta_t`` >= 1, else
    ValueError), each prediction fed back as the next input.  ``ids`` are validated like ``TrajectoryDataset.batch``'s.

    * Step 0 gets exactly the node tensors and the graph of ``ds.batch(ids)``.  On a dataset with a motion table (``rotation=`` /
      ``translation=``) that batch is moved, and so is the whole rollout: the truth rows are moved by each slot's motion
      (``data.apply_motion``'s rule, in fp32) before the difference, so ``pred`` and ``per_graph`` are in the moved frame.
    * After step k the model has returned ``x_new``, its prediction of frame ``f + (k+1) delta_t``; then ``vel = (x_new - loc) *
      (1/delta_t)`` (one fp32 subtraction, one fp32 multiplication by the fp32 value ``1.0f/delta_t``), ``node_feat[:,0] = |vel|`` by the
      loader's rule, ``loc = x_new``, ``loc_mean`` by the loader's rule; ``node_feat[:,1]``, ``node_attr``, ``ptr``, ``batch`` stay.
    * ``sse[k,b]`` = the fp64 sum over cloud b's nodes and components of ``(x_new - pos[f + (k+1) delta_t])**2`` (the moved rows of
      ``pos`` on a moved dataset), NaN where the
      trajectory has no such frame; the per-graph MSE is ``sse / (3 n_b)``.
    * A non-finite component of ``x_new`` never reaches the graph build: the state keeps the old position there, with velocity 0; the
      flag is read after the next graph build's read-back and the rollout stops with ``stopped = ("non-finite", k)``, k the step that
      produced it (after the last step the flag is read in ``result()``).  The recorded prediction and ``sse`` keep the raw value.
    * ``max_edges`` (default None: no limit): a step whose graph has more edges than this is not run -- ``stopped = ("max_edges",
      k)``.  A cloud that has collapsed into one radius is n**2 edges: set it to a small multiple of the first step's edge count when
      the model is not trusted.  (The edge list itself is built before it can be counted.)

    ``.batch``: the ``Batch`` the next ``step()`` feeds the model -- collate's keys without ``loc_t``; valid until the next ``step()``
    (the state tensors are updated in place), None once the rollout has ended.  ``.step()`` -> the prediction [N,3].  ``.k``: steps
    taken.  ``.result()``: see there.  State and score buffers are allocated here, once; a step allocates what the model and the graph
    build allocate.  One device; a step is not capturable as a whole (the graph build reads its edge counts back)."""

    def __init__(self, model, ds, ids, *, steps, record=False, max_edges=None):
        if not isinstance(ds, D.TrajectoryDataset):
            raise TypeError("fastegnn_amd.Rollout: ds must be a TrajectoryDataset (Rollout.from_state takes bare tensors)")
        if ds.delta_t < 1:
            raise ValueError("fastegnn_amd.Rollout: the dataset's delta_t must be at least 1 (the stride of a step)")
        steps = self._checked_steps(steps)
        ids_dev, ids_host = ds._checked_ids(ids, "fastegnn_amd.Rollout")
        nodes = ds._assemble_nodes(ids_dev, ids_host)
        node_cnt = ds._node_cnt[ids_host]
        self._ds = ds
        self._motion = nodes.get("motion")   # None, or (the slots' motion rows [B,12], has_t)
        self._setup(model, {k: nodes[k] for k in ("loc_0", "vel_0", "node_feat", "node_attr", "loc_mean", "batch", "ptr")},
                    [0] + np.cumsum(node_cnt).tolist(), ds.radius, ds.cutoff_rate, ds.delta_t, steps, record, max_edges)
        B = len(ids_host)
        self._truth = torch.empty((steps, B), dtype=torch.int64, device=ds.device)
        _ROLLOUT_OPS.plan(ids_dev, ds.samples_dev, ds.row0, ds.n, ds.T, ds.delta_t, self._truth)
        self._sse = torch.full((steps, B), float("nan"), dtype=torch.float64, device=ds.device)
        t, f = ds.samples[ids_host, 0], ds.samples[ids_host, 1]
        self._has_truth = (f[None, :] + (np.arange(steps)[:, None] + 1) * ds.delta_t) < ds.T_host[t][None, :]   # [steps,B], host
        self._first_graph()

    @classmethod
    def from_state(cls, model, loc_0, vel_0, node_type, ptr, *, virtual_channels, radius, cutoff_rate=0.0, delta_t=1, steps, record=False,
                   max_edges=None) -> "Rollout":
        """The same stepper without a dataset and without a score (``result()['mse']`` is all NaN): B clouds back to back in ``loc_0``
        / ``vel_0`` [N,3] and ``node_type`` [N] or [N,1], ``ptr`` (a list or an int64 tensor [B+1]) their node ranges, as
        ``water3d_batch`` takes them.  ``node_feat`` is ``water3d_batch``'s expression per cloud -- ``[|vel_0|, kind / kind.max()]`` --
        computed once, here; from the first step on ``node_feat[:,0]`` and ``loc_mean`` follow the rules above, and so does the first
        ``loc_mean``."""
        ptr_host = [int(v) for v in torch.as_tensor(ptr).tolist()]
        if len(ptr_host) < 2 or ptr_host[0] != 0 or ptr_host[-1] != loc_0.size(0) or any(a >= b for a, b in zip(ptr_host, ptr_host[1:])):
            raise ValueError("fastegnn_amd.Rollout.from_state: ptr must be 0 = ptr[0] < ... < ptr[B] = N")
        delta_t, C_ = int(delta_t), int(virtual_channels)
        if delta_t < 1 or C_ < 1 or not float(radius) > 0:
            raise ValueError("fastegnn_amd.Rollout.from_state: delta_t and virtual_channels must be at least 1 and radius positive")
        steps = cls._checked_steps(steps)
        dev, B = loc_0.device, len(ptr_host) - 1
        kind = node_type.detach().to(dev, torch.float32).reshape(-1, 1).contiguous()
        vel = vel_0.detach().to(dev, torch.float32).contiguous().clone()
        counts = torch.tensor([b - a for a, b in zip(ptr_host, ptr_host[1:])], dtype=torch.int64)
        state = {"loc_0": loc_0.detach().to(dev, torch.float32).contiguous().clone(), "vel_0": vel,
                 "node_feat": torch.cat([D._node_feat(vel[a:b], kind[a:b]) for a, b in zip(ptr_host, ptr_host[1:])], 0).contiguous(),
                 "node_attr": kind, "loc_mean": torch.empty((B, 3, C_), dtype=torch.float32, device=dev),
                 "batch": torch.repeat_interleave(torch.arange(B, dtype=torch.int64), counts).to(dev),
                 "ptr": torch.tensor(ptr_host, dtype=torch.int64).to(dev)}
        self = cls.__new__(cls)
        self._ds = self._motion = None
        self._setup(model, state, ptr_host, float(radius), float(cutoff_rate), delta_t, steps, record, max_edges)
        self._truth = self._sse = self._has_truth = None
        _ROLLOUT_OPS.graph(state["ptr"], state["loc_0"], None, None, None, state["loc_mean"], None)
        self._first_graph()
        return self

    @staticmethod
    def _checked_steps(steps) -> int:
        if int(steps) != steps or int(steps) < 1:
            raise ValueError(f"fastegnn_amd.Rollout: steps must be a positive integer, got {steps!r}")
        return int(steps)

    def _setup(self, model, state, ptr_host, radius, cutoff_rate, delta_t, steps, record, max_edges):
        if max_edges is not None and int(max_edges) < 0:
            raise ValueError("fastegnn_amd.Rollout: max_edges must be None or a non-negative integer")
        self.model, self.steps, self.k, self.stopped = model, steps, 0, None
        self.max_edges = None if max_edges is None else int(max_edges)
        self._state, self._ptr_host = state, ptr_host
        self._radius, self._cutoff_rate, self._delta_t = radius, cutoff_rate, delta_t
        dev, N = state["loc_0"].device, state["loc_0"].size(0)
        self.device = dev
        self._pred = torch.full((steps, N, 3), float("nan"), dtype=torch.float32, device=dev) if record else None
        self._flag = FlagWord(dev)
        self._batch = None

    def _first_graph(self):
        self._build_graph()
        self._check_edges()

    def _build_graph(self):
        """the graphs of the state's positions: the two batched calls of the loader, one read-back (the step's only synchronisation)"""
        s = self._state
        ei, dist = D._TRAJ_OPS.edges(s["loc_0"], s["ptr"], self._ptr_host, self._radius, self._cutoff_rate)
        out = dict(s)
        out["edge_attr"], out["edge_index"] = dist.unsqueeze(-1), ei
        self._batch = D.Batch(**{k: out[k] for k in D._BATCH_KEYS if k != "loc_t"})

    def _check_edges(self):
        if self.max_edges is not None and self._batch["edge_index"].size(1) > self.max_edges:
            self.stopped, self._batch = ("max_edges", self.k), None

    @property
    def batch(self) -> Optional[D.Batch]:
        return self._batch

    def step(self) -> torch.Tensor:
        """one step: augment + forward + the two launches of the state update + the next step's graph build -> the prediction [N,3]"""
        if self.stopped is not None or self.k >= self.steps:
            raise RuntimeError(f"fastegnn_amd.Rollout.step: the rollout has ended (k = {self.k} of {self.steps}, stopped = {self.stopped})")
        ops, data, s, k = _ROLLOUT_OPS, self._batch, self._state, self.k
        with torch.no_grad():
            edge_attr = ops.augment(data.get("edge_attr"), data["loc_0"], data["edge_index"])
            x_new = T._predict(self.model, data, edge_attr)[0].detach().float().contiguous()
            if x_new.shape != s["loc_0"].shape:
                raise RuntimeError(f"fastegnn_amd.Rollout.step: the model returned {list(x_new.shape)} for {list(s['loc_0'].shape)} positions")
            ops.advance(x_new, self._delta_t, s["loc_0"], s["vel_0"], s["node_feat"], self._pred[k] if self._pred is not None else None,
                        self._flag)
            score = self._sse is not None
            if score and self._motion is not None:
                ops.graph_moved(s["ptr"], s["loc_0"], x_new, self._ds.pos, self._truth[k], s["loc_mean"], self._sse[k], *self._motion)
            else:
                ops.graph(s["ptr"], s["loc_0"], x_new if score else None, self._ds.pos if score else None,
                          self._truth[k] if score else None, s["loc_mean"], self._sse[k] if score else None)
            self.k = k + 1
            if self.k < self.steps:
                self._build_graph()          # (its read-back: the advance launch has run, the flag word is current)
                if self._flag.get():
                    self.stopped, self._batch = ("non-finite", k), None
                else:
                    self._check_edges()
            else:
                self._batch = None
        return x_new

    def result(self) -> dict:
        """``dict(mse=, per_graph=, counted=, pred=, stopped=)``: ``per_graph`` float64 [steps,B] = ``sse / (3 n_b)`` (NaN where the
        trajectory has no truth frame and for steps not reached), ``mse`` float64 [steps] = its mean over the rollouts that have a truth
        frame at that step (NaN where none has), ``counted`` int64 [steps] = how many those are (0 for steps not reached) -- host
        tensors, from ONE read-back of the error sums; ``pred`` [steps,N,3] on the device (rows not reached NaN) or None without
        ``record=True``; ``stopped`` None or ``(reason, k)``."""
        steps, B = self.steps, len(self._ptr_host) - 1
        if self._sse is not None:
            sse = self._sse.cpu()            # the one read-back
        else:
            sse = torch.full((steps, B), float("nan"), dtype=torch.float64)
            if self.device.type == "cuda":
                torch.cuda.current_stream(self.device).synchronize()
        if self.stopped is None and self._flag.get():   # the last step's prediction: no graph build came after it
            self.stopped = ("non-finite", self.k - 1)
        n = torch.tensor(np.diff(np.asarray(self._ptr_host)), dtype=torch.float64)
        per_graph = sse / (3.0 * n)[None, :]
        has = torch.zeros((steps, B), dtype=torch.bool)
        if self._has_truth is not None:
            has[:self.k] = torch.from_numpy(self._has_truth[:self.k])
        counted = has.sum(1)
        mse = torch.where(has, per_graph, torch.zeros_like(per_graph)).sum(1) / counted.double()
        mse[counted == 0] = float("nan")
        return dict(mse=mse, per_graph=per_graph, counted=counted, pred=self._pred, stopped=self.stopped)


def _run(model, ds, ids, steps, kw) -> dict:
    ro = Rollout(model, ds, ids, steps=steps, **kw)
    while ro.stopped is None and ro.k < ro.steps:
        ro.step()
    return ro.result()


def rollout(model, ds, ids, steps, **kw) -> dict:
    """``Rollout(model, ds, ids, steps=steps, **kw)`` stepped to its end -> its ``result()``.  The model is put into ``eval()`` (its
    previous mode is restored) and runs under ``torch.no_grad()``, the fused models on their forward-only path.  After the read-back
    the model's range guard is polled once, as ``evaluate`` does: if a step left the operand range of the f16x2 build -- its non-finite
    prediction has stopped the rollout -- the module has moved to the wide-range build and the rollout is run ONCE more there.
    ``FastEGNN`` / ``FastRF`` are called by keyword, ``EGNN`` by its own signature (``train._predict``); nothing but ``model(...)`` is
    called, so a wide model (hidden_nf > 64) and ``ShardedFastEGNN`` work as they do in ``evaluate``."""
    guard = getattr(model, "_range", None)
    was_training = model.training
    model.eval()
    try:
        with torch.no_grad():
            wide_before = guard.wide if guard is not None else True
            out = _run(model, ds, ids, steps, kw)
            if guard is not None and not wide_before:
                guard.poll(type(model).__name__, getattr(model, "_plist", None), why="a rollout")
                if guard.wide:
                    out = _run(model, ds, ids, steps, kw)
    finally:
        model.train(was_training)
    return out
