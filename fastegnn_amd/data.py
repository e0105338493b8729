"""Batch format and dataset readers: what sits between the on-disk data and
``FastEGNN.forward`` in the reference's training harness.

* ``Frame``  -- one graph with the fields the reference datasets put into a ``torch_geometric.data.Data``
  (``datasets/nbody/dataset.py:97-98``, ``datasets/simulation/dataset.py:92-93``).
* ``collate`` / ``Batch`` -- the mini-batch the harness reads with ``data['...']``
  (``utils/train.py:36-53``): node- and edge-level tensors concatenated, ``edge_index`` shifted by the
  cumulative node count, ``batch`` [N], ``ptr`` [B+1], ``loc_mean`` stacked to [B,3,C].  This is the
  documented behaviour of PyG 2.5.2's collate for these fields (PyG is absent here: parity unpinned).
* ``NBodySystemDataset`` -- reader for the ``.npy`` files of ``datasets/nbody/datagen``
  (``datasets/nbody/dataset.py:44-113``), pinned by tests/golden/dataset_nbody5.npz.
* ``Simulation`` -- reader for the Water-3D ``.h5`` files (``datasets/simulation/dataset.py:46-101``);
  needs ``h5py`` and builds the radius graph on the GPU through the C-ABI (graphs.py); ``water3d_batch`` and
  ``frames_per_call`` build the graphs of several frames in one device call.
* ``DataLoader`` -- ``batch_size`` / ``shuffle`` / ``drop_last`` iteration over frames (``main_nbody.py:93-96``).
* ``PackedDataset`` / ``PackedLoader`` -- the same batches from a dataset packed once into one device table per field: a batch
  is two kernel launches (csrc/collate.hip) whatever its size, with no host-to-device copy and no synchronisation.  With
  ``graphs=...`` a batch also carries its ``SortedGraph``, assembled by two more launches from per-frame indices sorted once
  (``PackedDataset.build_graphs``): the model then sorts nothing per batch.
* ``PackedStream`` -- a packed dataset of EQUAL-SIZED frames (the N-body sets) streamed through buffers allocated once: the order
  is drawn on the device and ``next()`` is two or three launches with no host work at all, the same every time (capturable).
* ``TrajectoryDataset`` / ``TrajectoryLoader`` -- trajectories (Water-3D, the protein run) kept on the device as POSITIONS: a sample is
  (trajectory, start frame), a batch's node tensors are three launches (csrc/traj.hip) and its graphs are built per batch by the
  batched calls of ``water3d_batch``.  Some thirty times fewer device bytes per sample than the stored graphs of a packed dataset.

All processing is vectorised over the systems of a file and runs on the device the caller names.
"""
from __future__ import annotations

import math
import os
from dataclasses import dataclass, fields
from typing import Iterator, List, Optional, Sequence

import numpy as np
import torch

_NODE_KEYS = ("loc_0", "loc_t", "vel_0", "node_feat", "node_attr")


@dataclass
class Frame:
    edge_index: torch.Tensor   # int64 [2,E]
    edge_attr: torch.Tensor    # [E,1] edge length at frame 0
    loc_0: torch.Tensor        # [n,3]
    loc_t: torch.Tensor        # [n,3]
    vel_0: torch.Tensor        # [n,3]
    node_feat: torch.Tensor    # [n,2]  (|vel|, charge or type / max)
    node_attr: torch.Tensor    # [n,1]
    loc_mean: torch.Tensor     # [1,3,C]

    @property
    def num_nodes(self) -> int:
        return self.node_feat.size(0)

    def to(self, device) -> "Frame":
        return Frame(**{f.name: getattr(self, f.name).to(device) for f in fields(self)})

    def __getitem__(self, key: str) -> torch.Tensor:
        return getattr(self, key)


class Batch:
    """Mini-batch with the mapping interface the harness uses (``data['ptr']``, ``data.to(device)``,
    ``data.detach()``)."""

    def __init__(self, **tensors: torch.Tensor):
        self._t = dict(tensors)

    def __getitem__(self, key: str) -> torch.Tensor:
        return self._t[key]

    def __getattr__(self, key: str) -> torch.Tensor:
        try:
            return self.__dict__["_t"][key]
        except KeyError:
            raise AttributeError(key) from None

    def get(self, key: str, default=None):
        return self._t.get(key, default)

    def keys(self):
        return self._t.keys()

    @property
    def num_graphs(self) -> int:
        return self._t["ptr"].numel() - 1

    @property
    def num_nodes(self) -> int:
        return self._t["batch"].numel()

    # a packed batch may carry its sorted graph (key "graph", a model.SortedGraph: PackedLoader(graphs=...)); it is no tensor and
    # passes through the three calls below as it is -- its arrays stay on the device they were assembled on
    def to(self, device, non_blocking: bool = False) -> "Batch":
        return Batch(**{k: v.to(device, non_blocking=non_blocking) if isinstance(v, torch.Tensor) else v for k, v in self._t.items()})

    def detach(self) -> "Batch":
        return Batch(**{k: v.detach() if isinstance(v, torch.Tensor) else v for k, v in self._t.items()})

    def pin_memory(self) -> "Batch":
        return Batch(**{k: v.pin_memory() if isinstance(v, torch.Tensor) else v for k, v in self._t.items()})

    def __repr__(self) -> str:
        return "Batch(" + ", ".join(f"{k}={list(v.shape) if isinstance(v, torch.Tensor) else type(v).__name__}"
                                    for k, v in self._t.items()) + ")"


def collate(frames: Sequence[Frame]) -> Batch:
    if len(frames) == 0:
        raise ValueError("collate: empty list of frames")
    dev = frames[0].node_feat.device
    counts = torch.tensor([f.num_nodes for f in frames], dtype=torch.int64)
    ptr = torch.zeros(len(frames) + 1, dtype=torch.int64)
    ptr[1:] = torch.cumsum(counts, 0)
    out = {k: torch.cat([getattr(f, k) for f in frames], 0) for k in _NODE_KEYS}
    out["edge_attr"] = torch.cat([f.edge_attr for f in frames], 0)
    out["edge_index"] = torch.cat([f.edge_index + int(o) for f, o in zip(frames, ptr[:-1])], 1)
    out["loc_mean"] = torch.cat([f.loc_mean for f in frames], 0)
    out["batch"] = torch.repeat_interleave(torch.arange(len(frames), dtype=torch.int64), counts).to(dev)
    out["ptr"] = ptr.to(dev)
    return Batch(**out)


def _node_feat(vel_0: torch.Tensor, kind: torch.Tensor) -> torch.Tensor:
    # [|vel|, kind / max(kind)]   (datasets/nbody/dataset.py:89-92, datasets/simulation/dataset.py:84-87)
    return torch.cat([vel_0.pow(2).sum(-1, keepdim=True).sqrt(), kind / kind.max()], -1)


def _loc_mean(loc_0: torch.Tensor, C: int) -> torch.Tensor:
    return loc_0.mean(0).unsqueeze(-1).repeat(1, C).unsqueeze(0)


class NBodySystemDataset:
    """Frames (frame_0 -> frame_T) of the charged N-body systems written by ``datasets/nbody/datagen``.

    Same constructor arguments as ``datasets/nbody/dataset.py:18``; ``rotation`` replaces the
    reference's unseeded ``random_rotate()`` of the test partition (``:77-83``): pass a [3,3] matrix, a
    callable ``i -> [3,3]`` or None.  Edges: the ``int(n(n-1)(1-cutoff_rate))`` shortest ordered pairs of the
    complete graph in ascending length (``:102-113``); the two directions of a pair have the same
    length, so when that count is odd the direction kept for the last pair is unspecified, as in the
    reference (``torch.topk`` tie order)."""

    def __init__(self, dataset_name, data_dir, virtual_channels, partition="train", max_samples=1e8, frame_0=30,
                 frame_T=40, cutoff_rate=0.0, device="cpu", rotation=None):
        self.partition, self.virtual_channels, self.cutoff_rate = partition, int(virtual_channels), float(cutoff_rate)
        suffix = f"{partition}_charged{dataset_name}"
        n_keep = int(max_samples)
        # .npy layout (generate_dataset.py:84-92): loc/vel float64 [S,T,n,3], charges [S,n,1], edges [S,n,n]
        loc = np.load(os.path.join(data_dir, f"loc_{suffix}.npy"), mmap_mode="r")[:n_keep]
        vel = np.load(os.path.join(data_dir, f"vel_{suffix}.npy"), mmap_mode="r")[:n_keep]
        charges = np.load(os.path.join(data_dir, f"charges_{suffix}.npy"))[:n_keep]
        if loc.ndim != 4 or loc.shape[-1] != 3 or vel.shape != loc.shape:
            raise ValueError(f"NBodySystemDataset: unexpected array shapes {loc.shape} / {vel.shape}")
        self.num_node_r = loc.shape[-2]
        f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a)).float().to(device)  # noqa: E731
        self.data = self._process(f32(loc[:, frame_0]), f32(vel[:, frame_0]), f32(loc[:, frame_T]), f32(charges), rotation)

    def _process(self, loc_0, vel_0, loc_t, charges, rotation) -> List[Frame]:
        S, n, _ = loc_0.shape
        if rotation is not None:
            R = torch.stack([torch.as_tensor(rotation(i) if callable(rotation) else rotation) for i in range(S)])
            R = R.to(loc_0.device, torch.float32)
            loc_0, loc_t, vel_0 = loc_0 @ R, loc_t @ R, vel_0 @ R
        k = int(n * (n - 1) * (1 - self.cutoff_rate))
        if loc_0.is_cuda and n <= 128:
            from .graphs import nbody_cutoff_edges
            # device tensors: one workgroup per system sorts its n(n-1) pairs in LDS (csrc/graphs.hip)
            ei, ea = nbody_cutoff_edges(loc_0, k)
            ea = ea.unsqueeze(-1)                                                              # [S,k,1]
        else:   # host-side dataset build (what the reference does), or systems beyond the kernel's 128 particles
            dist = torch.cdist(loc_0, loc_0, p=2) + torch.eye(n, device=loc_0.device) * 1e18
            idc = torch.topk(dist.reshape(S, n * n), k, dim=1, largest=False).indices
            ei = torch.stack([idc.div(n, rounding_mode="trunc"), idc.remainder(n)], 1).long()  # [S,2,k]
            d = loc_0.gather(1, ei[:, 0, :, None].expand(-1, -1, 3)) - loc_0.gather(1, ei[:, 1, :, None].expand(-1, -1, 3))
            ea = d.pow(2).sum(-1).sqrt().unsqueeze(-1)                                        # [S,k,1]
        return [Frame(ei[s], ea[s], loc_0[s], loc_t[s], vel_0[s], _node_feat(vel_0[s], charges[s]), charges[s],
                      _loc_mean(loc_0[s], self.virtual_channels)) for s in range(S)]

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, i: int) -> Frame:
        return self.data[i]


def water3d_frame(loc_0, vel_0, loc_t, node_type, virtual_channels, radius=0.035, cutoff_rate=0.0, rotation=None) -> Frame:
    """``get_graph_step`` (``datasets/simulation/dataset.py:71-93``) for one frame of device tensors: radius
    graph without self loops, shortest-fraction cutoff, edge length attribute, node features, loc_mean."""
    from .graphs import cutoff_edges, radius_graph
    if rotation is not None:
        R = torch.as_tensor(rotation() if callable(rotation) else rotation).to(loc_0.device, torch.float32)
        loc_0, loc_t, vel_0 = loc_0 @ R, loc_t @ R, vel_0 @ R
    ei, dist = radius_graph(loc_0, radius)
    ei, dist = cutoff_edges(ei, dist, cutoff_rate)
    return Frame(ei, dist.unsqueeze(-1), loc_0, loc_t, vel_0, _node_feat(vel_0, node_type), node_type,
                 _loc_mean(loc_0, int(virtual_channels)))


def _water3d_batch_edges(clouds, radius, cutoff_rate, rotation):
    """The shared front of ``water3d_batch`` and ``Simulation(frames_per_call > 1)``: rotates every cloud
    ``(loc_0, vel_0, loc_t)`` as ``water3d_frame`` does (a callable ``rotation`` is called once per cloud, in order) and builds
    all their graphs with the two batched calls.  Returns (rotated clouds, host ptr list, edge_index with global ids, dist,
    host edge_ptr list of the kept edges)."""
    from .graphs import _radius_graph_batch, cutoff_edges_batch, keep_ptr_of
    if rotation is not None:
        rotated = []
        for loc_0, vel_0, loc_t in clouds:
            R = torch.as_tensor(rotation() if callable(rotation) else rotation).to(loc_0.device, torch.float32)
            rotated.append((loc_0 @ R, vel_0 @ R, loc_t @ R))
        clouds = rotated
    ptr = [0]
    for loc_0, _, _ in clouds:
        ptr.append(ptr[-1] + loc_0.size(0))
    ei, dist, edge_ptr, edge_ptr_host = _radius_graph_batch(torch.cat([c[0] for c in clouds], 0), ptr, radius)
    ei, dist, _ = cutoff_edges_batch(ei, dist, edge_ptr, cutoff_rate, edge_ptr_host=edge_ptr_host)
    return clouds, ptr, ei, dist, keep_ptr_of(edge_ptr_host, cutoff_rate)


def water3d_batch(loc_0, vel_0, loc_t, node_type, ptr, virtual_channels, radius=0.035, cutoff_rate=0.0, rotation=None) -> Batch:
    """``collate([water3d_frame(...) for every cloud])`` with the graphs of all clouds built in one device call
    (graphs.radius_graph_batch / cutoff_edges_batch: one host read-back for the batch).  The node tensors hold B clouds back
    to back, ``ptr`` (a list or an int64 tensor [B+1]; on the host it costs no read-back) their node ranges; every cloud must
    hold at least one point.  Node features and ``loc_mean`` are computed per cloud by the expressions of the per-frame path,
    so the result is bit-equal to it; a callable ``rotation`` is called once per cloud."""
    ptr = [int(v) for v in torch.as_tensor(ptr).tolist()]
    if len(ptr) < 2 or ptr[0] != 0 or ptr[-1] != loc_0.size(0) or any(a >= b for a, b in zip(ptr, ptr[1:])):
        raise ValueError("water3d_batch: ptr must be 0 = ptr[0] < ... < ptr[B] = N")
    dev, spans = loc_0.device, list(zip(ptr, ptr[1:]))
    clouds, _, ei, dist, _ = _water3d_batch_edges([(loc_0[s:e], vel_0[s:e], loc_t[s:e]) for s, e in spans], radius, cutoff_rate,
                                                  rotation)
    counts = torch.tensor([e - s for s, e in spans], dtype=torch.int64)
    out = {"loc_0": torch.cat([c[0] for c in clouds], 0), "loc_t": torch.cat([c[2] for c in clouds], 0),
           "vel_0": torch.cat([c[1] for c in clouds], 0),
           "node_feat": torch.cat([_node_feat(c[1], node_type[s:e]) for c, (s, e) in zip(clouds, spans)], 0),
           "node_attr": torch.cat([node_type[s:e] for s, e in spans], 0),
           "edge_attr": dist.unsqueeze(-1), "edge_index": ei,
           "loc_mean": torch.cat([_loc_mean(c[0], int(virtual_channels)) for c in clouds], 0),
           "batch": torch.repeat_interleave(torch.arange(len(spans), dtype=torch.int64), counts).to(dev),
           "ptr": torch.tensor(ptr, dtype=torch.int64).to(dev)}
    return Batch(**out)


def read_trajectories(directory: str, partition: str):
    """Yields ``(key, position [T,n,3], particle_type [n])`` of every trajectory of a partition, in file order.

    Two containers with the same fields: the reference's ``<partition>.h5`` (one HDF5 group per trajectory holding
    ``position`` and ``particle_type``, ``datasets/simulation/dataset.py:46-56``; needs ``h5py``) and
    ``<partition>.npz`` with arrays named ``<key>/position`` and ``<key>/particle_type`` (what
    ``numpy.savez`` of the same groups gives; readable without h5py).  The ``.h5`` file wins when both exist and
    h5py is importable; a lone ``.h5`` without h5py raises."""
    h5, npz = os.path.join(directory, f"{partition}.h5"), os.path.join(directory, f"{partition}.npz")
    if os.path.exists(h5):
        try:
            import h5py
        except ImportError as e:
            if not os.path.exists(npz):
                raise ImportError(f"fastegnn_amd.data: {h5} needs h5py (absent); convert it to {npz} "
                                  "(arrays '<key>/position', '<key>/particle_type')") from e
        else:
            with h5py.File(h5, "r") as f:
                for key in list(f.keys()):
                    yield key, np.array(f[key]["position"]), np.array(f[key]["particle_type"])
            return
    if not os.path.exists(npz):
        raise FileNotFoundError(f"fastegnn_amd.data: neither {h5} nor {npz} exists")
    with np.load(npz) as z:
        keys = []
        for name in z.files:                      # file order, first appearance of each trajectory key
            k = name.rsplit("/", 1)[0]
            if k not in keys:
                keys.append(k)
        for k in keys:
            yield k, z[f"{k}/position"], z[f"{k}/particle_type"]


class Simulation:
    """Water-3D style particle trajectories (``<data_dir>/<dataset_name>/<partition>.h5`` -- or ``.npz``, see
    ``read_trajectories``: one group per trajectory with ``position`` [T,n,3] and ``particle_type`` [n]).

    Same constructor arguments as ``datasets/simulation/dataset.py:17``.  The reference draws 15 start
    frames per trajectory with the unseeded ``random.randint(0, 250)`` (``:58``) and shuffles the frames
    (``:31``); here both come from ``seed``.  Per frame: ``vel_0 = pos[f+1] - pos[f]``, target
    ``pos[f + delta_t]``, edges = radius graph (r = 0.035, no self loops) reduced to the shortest
    ``1 - cutoff_rate`` fraction, built on the GPU (graphs.radius_graph / graphs.cutoff_edges).
    ``frames_per_call`` = k > 1 builds the graphs of up to k consecutive drawn frames of a trajectory in one batched call
    (graphs.radius_graph_batch / cutoff_edges_batch: one read-back per call, not per frame); the frames are the same."""

    RADIUS = 0.035
    FRAMES_PER_TRAJECTORY = 15

    def __init__(self, dataset_name, data_dir, virtual_channels, partition="train", max_samples=1e8, delta_t=15,
                 cutoff_rate=0.0, device="cuda", rotation=None, seed=0, radius=None, frames_per_call=1):
        self.virtual_channels, self.cutoff_rate, self.delta_t = int(virtual_channels), float(cutoff_rate), int(delta_t)
        self.radius = self.RADIUS if radius is None else float(radius)
        frames_per_call = int(frames_per_call)
        if frames_per_call < 1:
            raise ValueError("Simulation: frames_per_call must be at least 1")
        rng = np.random.default_rng(seed)
        self.data: List[Frame] = []
        self.frames: List[tuple] = []      # (trajectory key, start frame) of every sample, in the order drawn
        max_samples = int(max_samples)
        for key, position, particle_type in read_trajectories(os.path.join(data_dir, dataset_name), partition):
            ptype = torch.from_numpy(np.asarray(particle_type)).float().reshape(-1, 1)
            pos = torch.from_numpy(np.asarray(position)).float()
            n_frames = min(self.FRAMES_PER_TRAJECTORY, max_samples - len(self.data))
            last = min(250, pos.size(0) - 1 - max(1, self.delta_t))
            drawn = rng.integers(0, last + 1, size=max(n_frames, 0))
            if frames_per_call == 1:
                for fr in drawn:
                    fr = int(fr)
                    self.frames.append((key, fr))
                    self.data.append(water3d_frame(pos[fr].to(device), (pos[fr + 1] - pos[fr]).to(device),
                                                   pos[fr + self.delta_t].to(device), ptype.to(device),
                                                   self.virtual_channels, self.radius, self.cutoff_rate, rotation))
            else:
                for at in range(0, len(drawn), frames_per_call):
                    group = [int(fr) for fr in drawn[at:at + frames_per_call]]
                    self.frames.extend((key, fr) for fr in group)
                    self.data.extend(self._frames_of(pos, ptype.to(device), group, device, rotation))
            if len(self.data) >= max_samples:
                break
        order = rng.permutation(len(self.data))
        self.data = [self.data[i] for i in order]
        self.frames = [self.frames[i] for i in order]

    def _frames_of(self, pos, ptype, group, device, rotation) -> List[Frame]:
        """The frames of the start frames ``group`` of one trajectory, their edges from one batched build: the global edge
        list is cut at the per-graph offsets and the node offset taken off the ids; the rest is ``water3d_frame``'s."""
        clouds = [(pos[fr].to(device), (pos[fr + 1] - pos[fr]).to(device), pos[fr + self.delta_t].to(device)) for fr in group]
        clouds, ptr, ei, dist, keep = _water3d_batch_edges(clouds, self.radius, self.cutoff_rate, rotation)
        return [Frame(ei[:, a:b] - off, dist[a:b].clone().unsqueeze(-1), loc_0, loc_t, vel_0, _node_feat(vel_0, ptype), ptype,
                      _loc_mean(loc_0, self.virtual_channels))
                for (loc_0, vel_0, loc_t), off, a, b in zip(clouds, ptr, keep, keep[1:])]

    def __len__(self) -> int:
        return len(self.data)

    def __getitem__(self, i: int) -> Frame:
        return self.data[i]


class DataLoader:
    """``batch_size`` / ``shuffle`` / ``drop_last`` iteration yielding ``Batch`` objects
    (the use of ``torch_geometric.loader.DataLoader`` at ``main_nbody.py:93-96``)."""

    def __init__(self, dataset, batch_size=1, shuffle=False, drop_last=False, generator: Optional[torch.Generator] = None,
                 device=None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last = dataset, int(batch_size), shuffle, drop_last
        self.generator, self.device = generator, device

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self) -> Iterator[Batch]:
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator).tolist() if self.shuffle else list(range(n))
        for i in range(len(self)):
            b = collate([self.dataset[j] for j in order[i * self.batch_size:(i + 1) * self.batch_size]])
            yield b.to(self.device) if self.device is not None else b

    def state_dict(self) -> dict:
        return _generator_state(self.generator)

    def load_state_dict(self, state) -> None:
        _load_generator_state(self.generator, state, "DataLoader")


def _generator_state(generator) -> dict:
    """what a loader keeps between epochs: the state of its OWN ``torch.Generator`` (a uint8 tensor), from which the next epoch's
    ``torch.randperm`` is drawn.  A loader without one draws from torch's global generator, which a checkpoint holds by itself."""
    return {"generator": None if generator is None else generator.get_state().clone()}


def _load_generator_state(generator, state, who) -> None:
    saved = state.get("generator")
    if (saved is None) != (generator is None):
        raise ValueError(f"fastegnn_amd.{who}.load_state_dict: the state was saved {'without' if saved is None else 'with'} a generator "
                         f"of the loader's own, this loader has {'none' if generator is None else 'one'}")
    if saved is not None:
        generator.set_state(saved.cpu().to(torch.uint8))


# ---- device-resident packed datasets: a batch is two launches, whatever B is (csrc/collate.hip) ----
_PACK_KEYS = _NODE_KEYS + ("edge_attr", "loc_mean", "edge_index")   # FASTEGNN_COLLATE_* order (include/fastegnn_hip.h)
_NO_CPU = "fastegnn_amd: PackedDataset.batch needs device-resident tables (there is no CPU fallback)"


class HipCollateOps:
    """The two device calls of a packed batch on libfastegnn_hip.so (the product path).  tests/packed_ref.py restates them in
    torch so that tests/test_packed_cpu.py can drive the loader's orchestration without a GPU (the ``wide.HipOps`` precedent).
    ``sort`` and ``graph`` are the two calls behind a batch's sorted graph (tests/packed_graph_ref.py restates them likewise), ``draw``
    and ``gather_uniform`` the two behind a ``PackedStream`` batch (tests/packed_stream_ref.py)."""

    @staticmethod
    def plan(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out) -> None:
        """node_ptr_out / edge_ptr_out [B+1] <- exclusive prefix sums of the node / edge counts of the frames ``ids``"""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_collate_plan(K.ptr(ids), ids.numel(), K.ptr(src_node_ptr), K.ptr(src_edge_ptr),
                                              src_node_ptr.numel() - 1, K.ptr(node_ptr_out), K.ptr(edge_ptr_out),
                                              _stream(ids.device)), "fastegnn_collate_plan")

    @staticmethod
    def gather(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out, src_tables, dst_tables, batch_out) -> None:
        """every tensor of the batch in one launch; ``src_tables`` / ``dst_tables``: the eight tensors in ``_PACK_KEYS`` order"""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU)
        import ctypes as C
        from . import _lib as K
        from .model import _stream
        n = len(_PACK_KEYS)
        src = (C.c_void_p * n)(*[t.data_ptr() or None for t in src_tables])
        dst = (C.c_void_p * n)(*[t.data_ptr() or None for t in dst_tables])
        widths = (C.c_int32 * (n - 1))(*[math.prod(t.shape[1:]) for t in src_tables[:n - 1]])
        K.check(K.lib().fastegnn_collate_gather(K.ptr(ids), ids.numel(), K.ptr(src_node_ptr), K.ptr(src_edge_ptr),
                                                src_node_ptr.numel() - 1, src_tables[0].size(0), src_tables[5].size(0),
                                                K.ptr(node_ptr_out), K.ptr(edge_ptr_out), dst_tables[0].size(0),
                                                dst_tables[5].size(0), src, dst, widths, K.ptr(batch_out), _stream(ids.device)),
                "fastegnn_collate_gather")

    @staticmethod
    def sort(edge_index, n_nodes):
        """packing time: (rowptr, erow, col, perm, cscptr, csc_eid) of one slab of frames, ``fastegnn_build_csr``'s own (int32, edge
        arrays [E])"""
        if not edge_index.is_cuda:
            raise RuntimeError(_NO_CPU)
        from .model import SortedGraph
        g, E = SortedGraph(edge_index, n_nodes, csc=True), edge_index.size(1)
        return g.rowptr, g.erow[:E], g.col[:E], g.perm[:E], g.cscptr, g.csc_eid[:E]

    @staticmethod
    def graph(ids, src_node_ptr, src_edge_ptr, node_ptr_out, edge_ptr_out, n_nodes_out, n_edges_out, src_graph, dst_graph,
              chunk_row) -> int:
        """the batch's sorted index in two launches (fastegnn_collate_graph); ``src_graph``: the packed g_rowptr, g_erow, g_col,
        g_perm, g_cscptr, g_csc_eid; ``dst_graph``: rowptr, erow, col, perm, cscptr, csc_eid (the last two None: no col-keyed
        index).  Returns n_chunks, which is host arithmetic."""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU)
        import ctypes as C
        from . import _lib as K
        from .model import _stream
        nch = C.c_int32(0)
        K.check(K.lib().fastegnn_collate_graph(K.ptr(ids), ids.numel(), K.ptr(src_node_ptr), K.ptr(src_edge_ptr),
                                               src_node_ptr.numel() - 1, src_graph[0].numel() - 1, src_graph[1].numel(),
                                               K.ptr(node_ptr_out), K.ptr(edge_ptr_out), n_nodes_out, n_edges_out,
                                               *[K.ptr(t) for t in src_graph], *[K.ptr(t) for t in dst_graph], K.ptr(chunk_row),
                                               C.byref(nch), _stream(ids.device)), "fastegnn_collate_graph")
        return nch.value

    @staticmethod
    def draw(state, batch_size, n_frames, shuffle, advance, ids_out) -> None:
        """ids_out int64 [B] <- the frame numbers of the next batch of a stream (fastegnn_collate_draw); ``state``: int64 [4] holding
        the bit patterns of {seed, epoch, cursor, reserved}, advanced on the device when ``advance``.  One launch."""
        if not ids_out.is_cuda:
            raise RuntimeError(_NO_CPU)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_collate_draw(K.ptr(state), batch_size, n_frames, 1 if shuffle else 0, 1 if advance else 0,
                                              K.ptr(ids_out), _stream(ids_out.device)), "fastegnn_collate_draw")

    @staticmethod
    def uniform_call(ids, n_frames, nodes_per_frame, edges_per_frame, src_tables, dst_tables, src_graph, dst_graph, chunk_row):
        """the ctypes arguments of one ``gather_uniform`` call, built ONCE for buffers that stay where they are (``PackedStream``)"""
        import ctypes as C
        from . import _lib as K
        n = len(_PACK_KEYS)
        src = (C.c_void_p * n)(*[t.data_ptr() or None for t in src_tables])
        dst = (C.c_void_p * n)(*[t.data_ptr() or None for t in dst_tables])
        widths = (C.c_int32 * (n - 1))(*[math.prod(t.shape[1:]) for t in src_tables[:n - 1]])
        nch = C.c_int32(0)
        graph = [K.ptr(t) for t in src_graph] + [K.ptr(t) for t in dst_graph] + [K.ptr(chunk_row)] if dst_graph is not None \
            else [None] * 13
        return [K.ptr(ids), ids.numel(), n_frames, nodes_per_frame, edges_per_frame, n_frames * nodes_per_frame,
                n_frames * edges_per_frame, src, dst, widths, *graph, C.byref(nch)], nch

    @staticmethod
    def gather_uniform(ids, n_frames, nodes_per_frame, edges_per_frame, src_tables, dst_tables, src_graph=None, dst_graph=None,
                       chunk_row=None, call=None) -> int:
        """the batch of the equal-sized frames ``ids`` in one launch, and its sorted graph with one more (fastegnn_collate_gather_uniform);
        tables as ``gather``, graph arrays as ``graph`` (``dst_graph`` None: no graph).  ``call``: ``uniform_call``'s result for these very
        tensors, which spares rebuilding the argument list.  Returns n_chunks (0 without a graph), which is host arithmetic."""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU)
        from . import _lib as K
        from .model import _stream
        args, nch = call if call is not None else HipCollateOps.uniform_call(ids, n_frames, nodes_per_frame, edges_per_frame,
                                                                             src_tables, dst_tables, src_graph, dst_graph, chunk_row)
        K.check(K.lib().fastegnn_collate_gather_uniform(*args, _stream(ids.device)), "fastegnn_collate_gather_uniform")
        return nch.value


_COLLATE_OPS = HipCollateOps

# PackedDataset.build_graphs sorts the frames in slabs of whole frames, each slab one fastegnn_build_csr call: a slab is closed before
# it would exceed any of these (a single frame beyond them is a slab of its own).  Far inside the sorted graph's own limits below, so
# that the sort workspace (28 bytes per edge) stays near a hundred megabytes.
GRAPH_SLAB_NODES = 1 << 20
GRAPH_SLAB_EDGES = 1 << 22
GRAPH_SLAB_FRAMES = 1 << 16
# the edge stages address their tables with 32-bit offsets (include/fastegnn_hip.h, fastegnn_build_csr): n * 68 and E * 8 below 2^30
_GRAPH_MAX_NODES = (1 << 30) // 68
_GRAPH_MAX_EDGES = (1 << 30) // 8 - 1
_GRAPH_KEYS = ("g_rowptr", "g_erow", "g_col", "g_perm", "g_cscptr", "g_csc_eid")


def _check_graphs(graphs) -> None:
    if not (graphs is None or graphs in ("csr", "csr+csc") or callable(graphs)):
        raise ValueError(f"fastegnn_amd: graphs must be None, 'csr', 'csr+csc' or a callable n_edges -> bool, got {graphs!r}")


def _chunk_edges() -> int:
    from . import _lib as K
    return K.lib().fastegnn_chunk_edges()


class PackedDataset:
    """The frames of a dataset (``NBodySystemDataset(...)``, ``Simulation(...)``, a list of ``Frame``) concatenated ONCE into one
    table per field on ``device`` (default: where the first frame lives), ``edge_index`` with the frames' LOCAL node ids.
    ``node_ptr`` / ``edge_ptr`` [n+1] are the prefix sums of the node / edge counts, on the device; ``node_ptr_host`` /
    ``edge_ptr_host`` the same as host int64 arrays, from which every output size is computed -- nothing is ever read back.
    ``packed[i]`` is a ``Frame`` of views into the tables, so a packed dataset can stand wherever a dataset does.
    ``batch(ids)`` is ``collate([packed[i] for i in ids])`` bit for bit, assembled by two kernel launches."""

    def __init__(self, frames, device=None):
        n = len(frames)
        if n == 0:
            raise ValueError("PackedDataset: empty sequence of frames")
        fl = [frames[i] for i in range(n)]
        first = fl[0]
        for i, f in enumerate(fl):
            for k in _PACK_KEYS:
                t, want = getattr(f, k), torch.int64 if k == "edge_index" else torch.float32
                if t.dtype != want:
                    raise ValueError(f"PackedDataset: frame {i}: {k} is {t.dtype}, expected {want}")
                if k != "edge_index" and (t.dim() != first[k].dim() or t.shape[1:] != first[k].shape[1:]):
                    raise ValueError(f"PackedDataset: frame {i}: {k} has shape {list(t.shape)}, frame 0 has {list(first[k].shape)}")
            if any(getattr(f, k).dim() != 2 or getattr(f, k).size(0) != f.num_nodes for k in _NODE_KEYS):
                raise ValueError(f"PackedDataset: frame {i}: the node tensors must be [n, width] with one n")
            if f.loc_mean.dim() != 3 or f.loc_mean.size(0) != 1 or f.loc_mean.size(1) != 3:
                raise ValueError(f"PackedDataset: frame {i}: loc_mean must be [1,3,C], got {list(f.loc_mean.shape)}")
            if f.edge_index.dim() != 2 or f.edge_index.size(0) != 2 or f.edge_attr.dim() != 2 or \
                    f.edge_attr.size(0) != f.edge_index.size(1):
                raise ValueError(f"PackedDataset: frame {i}: edge_index must be [2,E] and edge_attr [E, width]")
        self.device = torch.device(device) if device is not None else first.node_feat.device
        self.tables = {k: torch.cat([getattr(f, k) for f in fl], 1 if k == "edge_index" else 0).to(self.device).contiguous()
                       for k in _PACK_KEYS}
        self.node_ptr_host = np.concatenate([[0], np.cumsum([f.num_nodes for f in fl], dtype=np.int64)]).astype(np.int64)
        self.edge_ptr_host = np.concatenate([[0], np.cumsum([f.edge_index.size(1) for f in fl], dtype=np.int64)]).astype(np.int64)
        self.node_ptr = torch.from_numpy(self.node_ptr_host).to(self.device)
        self.edge_ptr = torch.from_numpy(self.edge_ptr_host).to(self.device)
        self._node_cnt, self._edge_cnt = np.diff(self.node_ptr_host), np.diff(self.edge_ptr_host)
        self.graph_tables = None   # the per-frame sorted indices: build_graphs(), only when a batch is asked for its graph

    def build_graphs(self) -> "PackedDataset":
        """Sorts every frame's graph ONCE, so that a batch's ``SortedGraph`` is assembled by a gather and no sort runs per batch.
        The existing ``fastegnn_build_csr`` is run over slabs of whole frames (``GRAPH_SLAB_NODES`` / ``_EDGES`` / ``_FRAMES``), a slab
        being one batch with global ids; its result is stored with ids and positions local to the frame (plain torch, one-off) in
        ``graph_tables``: ``g_rowptr`` / ``g_cscptr`` int64 [nodes + 1], ``g_erow`` / ``g_col`` / ``g_perm`` / ``g_csc_eid`` int32 [edges]
        (include/fastegnn_hip.h, fastegnn_collate_graph) -- 16 bytes per edge plus 16 per node of device memory.  A frame beyond
        the sorted graph's own limits (15.7 M nodes, 134 M edges) raises ValueError.  Idempotent; returns self."""
        if self.graph_tables is not None:
            return self
        n, dev = len(self), self.device
        for f in range(n):
            if self._node_cnt[f] > _GRAPH_MAX_NODES or self._edge_cnt[f] > _GRAPH_MAX_EDGES:
                raise ValueError(f"PackedDataset.build_graphs: frame {f} has {self._node_cnt[f]} nodes and {self._edge_cnt[f]} edges; a "
                                 f"sorted graph holds at most {_GRAPH_MAX_NODES} nodes and {_GRAPH_MAX_EDGES} edges")
        cap_n, cap_e = min(GRAPH_SLAB_NODES, _GRAPH_MAX_NODES), min(GRAPH_SLAB_EDGES, _GRAPH_MAX_EDGES)
        nodes, edges = int(self.node_ptr_host[-1]), int(self.edge_ptr_host[-1])
        ptr64 = lambda: torch.empty(nodes + 1, dtype=torch.int64, device=dev)  # noqa: E731
        idx32 = lambda: torch.empty(edges, dtype=torch.int32, device=dev)  # noqa: E731
        G = dict(g_rowptr=ptr64(), g_erow=idx32(), g_col=idx32(), g_perm=idx32(), g_cscptr=ptr64(), g_csc_eid=idx32())
        f0 = 0
        while f0 < n:
            f1 = f0 + 1   # a slab holds at least one frame
            while f1 < n and f1 - f0 < GRAPH_SLAB_FRAMES and self.node_ptr_host[f1 + 1] - self.node_ptr_host[f0] <= cap_n \
                    and self.edge_ptr_host[f1 + 1] - self.edge_ptr_host[f0] <= cap_e:
                f1 += 1
            n0, n1 = int(self.node_ptr_host[f0]), int(self.node_ptr_host[f1])
            e0, e1 = int(self.edge_ptr_host[f0]), int(self.edge_ptr_host[f1])
            # the frame of every edge of the slab: the stable sort by row keeps each frame's edges in the frame's own range of
            # positions (frames own ascending node ranges), and so does the col-keyed order, so this holds for sorted positions too
            frame_of = torch.repeat_interleave(torch.arange(f1 - f0, device=dev), self.edge_ptr[f0 + 1:f1 + 1] - self.edge_ptr[f0:f1],
                                               output_size=e1 - e0)
            node_off, edge_off = (self.node_ptr[f0:f1] - n0)[frame_of], (self.edge_ptr[f0:f1] - e0)[frame_of]
            ei = (self.tables["edge_index"][:, e0:e1] + node_off).contiguous()
            rowptr, erow, col, perm, cscptr, csc_eid = _COLLATE_OPS.sort(ei, n1 - n0)
            G["g_rowptr"][n0:n1] = rowptr[:-1].long() + e0
            G["g_cscptr"][n0:n1] = cscptr[:-1].long() + e0
            G["g_erow"][e0:e1] = erow - node_off.int()
            G["g_col"][e0:e1] = col - node_off.int()
            G["g_perm"][e0:e1] = perm - edge_off.int()
            G["g_csc_eid"][e0:e1] = csc_eid - edge_off.int()
            f0 = f1
        G["g_rowptr"][nodes] = edges
        G["g_cscptr"][nodes] = edges
        self.graph_tables = G
        return self

    def __len__(self) -> int:
        return self.node_ptr_host.size - 1

    @property
    def frame_shape(self):
        """``(nodes, edges)`` when every frame has the same node count and the same edge count (the N-body sets), else ``None``; from
        the host copies of the counts.  What ``PackedStream`` needs."""
        nodes, edges = int(self._node_cnt[0]), int(self._edge_cnt[0])
        if (self._node_cnt == nodes).all() and (self._edge_cnt == edges).all():
            return nodes, edges
        return None

    def __getitem__(self, i: int) -> Frame:
        n = len(self)
        i = int(i)
        if not -n <= i < n:
            raise IndexError(f"PackedDataset: frame {i} of {n}")
        i %= n
        a, b = int(self.node_ptr_host[i]), int(self.node_ptr_host[i + 1])
        ea, eb = int(self.edge_ptr_host[i]), int(self.edge_ptr_host[i + 1])
        T = self.tables
        return Frame(T["edge_index"][:, ea:eb], T["edge_attr"][ea:eb], *[T[k][a:b] for k in _NODE_KEYS], T["loc_mean"][i:i + 1])

    def _upload(self, ids: torch.Tensor) -> torch.Tensor:
        """host int64 ids -> device, without a synchronisation: through a FRESH pinned buffer and a non-blocking copy (the
        caching host allocator hands a pinned block out again only after the copies queued from it have completed, so no
        buffer is rewritten under a queued copy)."""
        if self.device.type != "cuda":
            return ids.to(self.device)
        staging = torch.empty(ids.numel(), dtype=torch.int64, pin_memory=True)
        staging.copy_(ids)
        return staging.to(self.device, non_blocking=True)

    def _assemble(self, ids_dev: torch.Tensor, ids_host: np.ndarray, graphs=None) -> Batch:
        """the batch of the frames ``ids_dev`` (device int64 [B]); ``ids_host``: the same ids on the host, already validated"""
        B, dev, T = int(ids_host.size), self.device, self.tables
        n_nodes, n_edges = int(self._node_cnt[ids_host].sum()), int(self._edge_cnt[ids_host].sum())
        out = {k: torch.empty((n_nodes,) + T[k].shape[1:], dtype=torch.float32, device=dev) for k in _NODE_KEYS}
        out["edge_attr"] = torch.empty((n_edges,) + T["edge_attr"].shape[1:], dtype=torch.float32, device=dev)
        out["edge_index"] = torch.empty((2, n_edges), dtype=torch.int64, device=dev)
        out["loc_mean"] = torch.empty((B,) + T["loc_mean"].shape[1:], dtype=torch.float32, device=dev)
        out["batch"] = torch.empty(n_nodes, dtype=torch.int64, device=dev)
        out["ptr"] = torch.empty(B + 1, dtype=torch.int64, device=dev)
        edge_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
        _COLLATE_OPS.plan(ids_dev, self.node_ptr, self.edge_ptr, out["ptr"], edge_ptr)
        _COLLATE_OPS.gather(ids_dev, self.node_ptr, self.edge_ptr, out["ptr"], edge_ptr, [T[k] for k in _PACK_KEYS],
                            [out[k] for k in _PACK_KEYS], out["batch"])
        if graphs is not None:
            out["graph"] = self._assemble_graph(ids_dev, out["ptr"], edge_ptr, n_nodes, n_edges, graphs)
        return Batch(**out)

    def _assemble_graph(self, ids_dev, node_ptr_out, edge_ptr_out, n_nodes: int, n_edges: int, graphs):
        """the batch's ``SortedGraph`` from the per-frame indices (two launches, sizes from the host counts: nothing is read back)"""
        from .model import SortedGraph
        csc = bool(graphs(n_edges)) if callable(graphs) else graphs == "csr+csc"
        G = self.build_graphs().graph_tables
        i32 = dict(dtype=torch.int32, device=self.device)
        arr = [torch.empty(n_nodes + 1, **i32)] + [torch.empty(max(n_edges, 1), **i32) for _ in range(3)]   # rowptr, erow, col, perm
        arr += [torch.empty(n_nodes + 1, **i32), torch.empty(max(n_edges, 1), **i32)] if csc else [None, None]
        chunk_row = torch.empty(n_edges // _chunk_edges() + 2, **i32)   # fastegnn_chunk_rows(E)
        n_chunks = _COLLATE_OPS.graph(ids_dev, self.node_ptr, self.edge_ptr, node_ptr_out, edge_ptr_out, n_nodes, n_edges,
                                      [G[k] for k in _GRAPH_KEYS], arr, chunk_row)
        return SortedGraph.from_arrays(*arr, chunk_row, n_chunks, n_nodes, n_nodes, n_edges)

    def batch(self, ids, graphs=None) -> Batch:
        """``collate([self[i] for i in ids])``: same keys in the same order, every tensor fresh and contiguous.  ``ids``: a host
        sequence, numpy array or CPU tensor of frame numbers in ``[0, len(self))`` (any order, repeats allowed), checked on the
        host: an id outside raises IndexError.  Two kernel launches and the upload of ``ids``; nothing is read back.
        ``graphs``: None (default) -- exactly that; ``"csr"`` / ``"csr+csc"`` / a callable ``n_edges -> bool`` (does this batch need the
        col-keyed index?  e.g. ``model.deterministic_for``) -- the batch gains one key, ``"graph"``: the ``SortedGraph`` of its
        ``edge_index``, element for element what the model would have sorted, assembled from indices sorted once
        (``build_graphs``, run on first use) by two more launches.  Pass it to the model as ``edge_index=``."""
        _check_graphs(graphs)
        if isinstance(ids, torch.Tensor):
            if ids.is_cuda:
                raise ValueError("PackedDataset.batch: ids must live on the host")
            ids = ids.numpy()
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0:
            raise ValueError("PackedDataset.batch: ids must be a non-empty 1-D sequence")
        if ids.dtype.kind not in "iu":
            raise ValueError(f"PackedDataset.batch: ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= len(self):
            raise IndexError(f"PackedDataset.batch: ids span [{ids.min()}, {ids.max()}] but there are {len(self)} frames")
        return self._assemble(self._upload(torch.from_numpy(ids)), ids, graphs)


class PackedLoader:
    """``DataLoader`` over a ``PackedDataset``: same batching, same ``torch.randperm(n, generator=...)`` order (equal generators
    give the same batches in the same order).  The epoch's order is uploaded ONCE, through pinned memory with a non-blocking
    copy; every batch hands the kernels a slice of that device tensor, so a batch is two launches and no copy.
    ``graphs`` (see ``PackedDataset.batch``): every batch also carries its ``SortedGraph`` under ``"graph"``, two more launches; the
    dataset's frames are sorted once, when the first batch is drawn."""

    def __init__(self, packed: PackedDataset, batch_size=1, shuffle=False, drop_last=False,
                 generator: Optional[torch.Generator] = None, graphs=None):
        _check_graphs(graphs)
        self.packed, self.batch_size, self.shuffle, self.drop_last = packed, int(batch_size), shuffle, drop_last
        self.generator, self.graphs = generator, graphs

    def __len__(self) -> int:
        n = len(self.packed)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self) -> Iterator[Batch]:
        n = len(self.packed)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        ids_dev, order_host = self.packed._upload(order), order.numpy()
        for i in range(len(self)):
            a, b = i * self.batch_size, min((i + 1) * self.batch_size, n)
            yield self.packed._assemble(ids_dev[a:b], order_host[a:b], self.graphs)

    def state_dict(self) -> dict:
        return _generator_state(self.generator)

    def load_state_dict(self, state) -> None:
        _load_generator_state(self.generator, state, "PackedLoader")


def _u64(v) -> int:
    return int(v) & 0xFFFFFFFFFFFFFFFF


def _i64(v) -> int:
    v = _u64(v)
    return v - (1 << 64) if v >= 1 << 63 else v


class PackedStream:
    """Batches of a ``PackedDataset`` whose frames all have the same node and edge counts (``packed.frame_shape``: the N-body sets),
    with NO host work per batch.  Every full batch then has the same shapes, so the stream allocates ONCE -- every tensor of the
    ``Batch`` (``ptr``, ``batch`` and the edge offsets never change and are written here), the frame numbers ``ids`` and, with
    ``graphs`` (``None`` / ``"csr"`` / ``"csr+csc"`` / a callable ``n_edges -> bool`` evaluated once with ``B * edges``, as
    ``PackedDataset.batch``), the arrays of one ``SortedGraph``; ``build_graphs()`` runs here.  The order is drawn on the device: a
    keyed permutation of the frames per epoch (include/fastegnn_hip.h, fastegnn_collate_draw) from ``{seed, epoch, cursor}`` in device
    memory -- not ``torch.randperm``'s order; ``shuffle=False`` walks the frames in order.

    ``next()`` issues two launches on the current stream (three with a graph): the draw, one gather over every table (and graph
    array), the graph's chunk rows.  It allocates nothing, uploads nothing, reads nothing back, and is the same launch sequence every
    time, so it may be captured into a HIP graph; replays walk on through the epochs.  It returns the SAME ``Batch`` object each time,
    its tensors overwritten: a batch is valid until the next ``next()``.  Whoever keeps an autograd graph, or any tensor of a batch,
    across iterations holds data that the next batch replaces -- call ``backward()`` before the next ``next()`` (``train_step`` does)
    or clone what must survive.  ``stream.ids`` is the device tensor of the current batch's frame numbers.

    ``len(stream)`` is ``len(packed) // batch_size``: full batches only; under shuffle the frames left over differ per epoch, as with
    ``DataLoader(drop_last=True)``.  Iterating yields ``len(stream)`` times ``next()``.  ``state_dict()`` / ``load_state_dict()`` hold
    ``{seed, epoch, cursor}`` (reading them back is one synchronisation); a resumed stream continues the same sequence.  The batch has
    ``collate``'s keys in ``collate``'s order, plus ``"graph"`` when asked: ``train_step`` / ``evaluate`` take it unchanged.  Ragged
    datasets, and a short last batch, are ``PackedLoader``'s."""

    def __init__(self, packed: PackedDataset, batch_size, shuffle=True, seed=0, graphs=None):
        _check_graphs(graphs)
        shape, n, B = packed.frame_shape, len(packed), int(batch_size)
        if shape is None:
            raise ValueError("PackedStream: the frames differ in their node or edge counts; a ragged dataset takes PackedLoader")
        if B < 1 or B > n:
            raise ValueError(f"PackedStream: batch_size = {B} with {n} frames: a stream yields full batches only (1 <= batch_size <= "
                             f"frames); PackedLoader yields a short batch")
        dev, T = packed.device, packed.tables
        if dev.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.PackedStream: build the stream before the stream capture")
        nodes, edges = shape
        N, E = B * nodes, B * edges
        self.packed, self.batch_size, self.shuffle, self.graphs = packed, B, bool(shuffle), graphs
        self.frame_shape, self.device = shape, dev
        out = {k: torch.zeros((N,) + T[k].shape[1:], dtype=torch.float32, device=dev) for k in _NODE_KEYS}
        out["edge_attr"] = torch.zeros((E,) + T["edge_attr"].shape[1:], dtype=torch.float32, device=dev)
        out["edge_index"] = torch.zeros((2, E), dtype=torch.int64, device=dev)
        out["loc_mean"] = torch.zeros((B,) + T["loc_mean"].shape[1:], dtype=torch.float32, device=dev)
        out["batch"] = torch.repeat_interleave(torch.arange(B, dtype=torch.int64), nodes).to(dev)
        out["ptr"] = (torch.arange(B + 1, dtype=torch.int64) * nodes).to(dev)
        self.edge_ptr = (torch.arange(B + 1, dtype=torch.int64) * edges).to(dev)
        self.ids = torch.zeros(B, dtype=torch.int64, device=dev)
        self._state = torch.tensor([_i64(seed), 0, 0, 0], dtype=torch.int64).to(dev)   # the bit patterns of {seed, epoch, cursor, -}
        self._src, self._dst = [T[k] for k in _PACK_KEYS], [out[k] for k in _PACK_KEYS]
        self._src_graph = self._dst_graph = self._chunk_row = None
        if graphs is not None:
            from .model import SortedGraph
            csc = bool(graphs(E)) if callable(graphs) else graphs == "csr+csc"
            G = packed.build_graphs().graph_tables
            i32 = dict(dtype=torch.int32, device=dev)
            arr = [torch.zeros(N + 1, **i32)] + [torch.zeros(max(E, 1), **i32) for _ in range(3)]   # rowptr, erow, col, perm
            arr += [torch.zeros(N + 1, **i32), torch.zeros(max(E, 1), **i32)] if csc else [None, None]
            self._chunk_row = torch.zeros(E // _chunk_edges() + 2, **i32)   # fastegnn_chunk_rows(E)
            self._src_graph, self._dst_graph = [G[k] for k in _GRAPH_KEYS], arr
            out["graph"] = SortedGraph.from_arrays(*arr, self._chunk_row, E // _chunk_edges() + 1, N, N, E)
        self._batch = Batch(**out)
        self._call = None
        if dev.type == "cuda":   # the argument list of the gather never changes: the buffers stay where they are
            self._call = HipCollateOps.uniform_call(self.ids, n, nodes, edges, self._src, self._dst, self._src_graph, self._dst_graph,
                                                    self._chunk_row)

    def __len__(self) -> int:
        return len(self.packed) // self.batch_size

    def next(self) -> Batch:
        """draws the next batch's frames and assembles them into the stream's buffers -> the stream's one ``Batch`` (see the class)"""
        ops, (nodes, edges) = _COLLATE_OPS, self.frame_shape
        ops.draw(self._state, self.batch_size, len(self.packed), self.shuffle, True, self.ids)
        ops.gather_uniform(self.ids, len(self.packed), nodes, edges, self._src, self._dst, self._src_graph, self._dst_graph,
                           self._chunk_row, call=self._call if ops is HipCollateOps else None)
        return self._batch

    def __iter__(self) -> Iterator[Batch]:
        for _ in range(len(self)):
            yield self.next()

    def state_dict(self) -> dict:
        """(copies the words back: one synchronisation)"""
        seed, epoch, cursor, _ = self._state.tolist()
        return {"seed": _u64(seed), "epoch": _u64(epoch), "cursor": _u64(cursor)}

    def load_state_dict(self, state) -> None:
        if self.device.type == "cuda" and torch.cuda.is_current_stream_capturing():
            raise RuntimeError("fastegnn_amd.PackedStream: the state is written between replays, not inside a stream capture")
        self._state[:3].copy_(torch.tensor([_i64(state["seed"]), _i64(state["epoch"]), _i64(state["cursor"])], dtype=torch.int64))


# ---- device-resident trajectories: only positions and kinds are stored, a batch's graphs are built per batch (csrc/traj.hip) ----
_BATCH_KEYS = _NODE_KEYS + ("edge_attr", "edge_index", "loc_mean", "batch", "ptr")   # collate's keys in collate's order
_TRAJ_SLOT_WORDS = 4   # FASTEGNN_TRAJ_SLOT_WORDS (include/fastegnn_hip.h)
_NO_CPU_TRAJ = "fastegnn_amd: TrajectoryDataset.batch needs device-resident tables (there is no CPU fallback)"


def _upload_ids(ids: torch.Tensor, device) -> torch.Tensor:
    """host int64 ids -> device without a synchronisation (``PackedDataset._upload``'s way: a fresh pinned buffer, a non-blocking copy)"""
    if device.type != "cuda":
        return ids.to(device)
    staging = torch.empty(ids.shape, dtype=torch.int64, pin_memory=True)
    staging.copy_(ids)
    return staging.to(device, non_blocking=True)


class HipTrajOps:
    """The device calls of a trajectory batch on libfastegnn_hip.so (the product path): ``plan``, ``gather`` and ``mean`` are the three
    launches of its node side (include/fastegnn_hip.h, fastegnn_traj_*), ``edges`` the two batched graph calls ``water3d_batch`` makes;
    ``gather_moved`` and ``mean_of`` replace ``gather`` and ``mean`` for a batch with a rigid motion per slot (tests/motion_ref.py).
    tests/trajectory_ref.py restates the first three in torch, so that tests/test_trajectory_cpu.py can drive the orchestration
    without a GPU (the ``HipCollateOps`` precedent)."""

    @staticmethod
    def plan(ids, samples, traj_row0, traj_n, traj_T, traj_kind0, delta_t, ptr_out, slots_out) -> None:
        """ptr_out [B+1] <- exclusive prefix sums of the node counts of the samples ``ids``; slots_out [B,4] <- per slot the first
        row in ``pos`` of frames f, f+1, f+delta_t and the first row in ``kind``"""
        if not ids.is_cuda:
            raise RuntimeError(_NO_CPU_TRAJ)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_traj_plan(K.ptr(ids), ids.numel(), K.ptr(samples), samples.size(0), K.ptr(traj_row0), K.ptr(traj_n),
                                           K.ptr(traj_T), K.ptr(traj_kind0), traj_n.numel(), int(delta_t), K.ptr(ptr_out),
                                           K.ptr(slots_out), _stream(ids.device)), "fastegnn_traj_plan")

    @staticmethod
    def gather(ptr, slots, n_nodes, pos, kind, kind_scaled, loc_0, loc_t, vel_0, node_feat, node_attr, batch_out) -> None:
        """the six node-level tensors of the batch in one launch over its ``n_nodes`` nodes"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_TRAJ)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_traj_gather(K.ptr(ptr), K.ptr(slots), ptr.numel() - 1, int(n_nodes), K.ptr(pos), pos.size(0),
                                             K.ptr(kind), K.ptr(kind_scaled), kind.size(0), K.ptr(loc_0), K.ptr(loc_t), K.ptr(vel_0),
                                             K.ptr(node_feat), K.ptr(node_attr), K.ptr(batch_out), _stream(ptr.device)),
                "fastegnn_traj_gather")

    @staticmethod
    def mean(ptr, slots, pos, loc_mean) -> None:
        """loc_mean [B,3,C] <- per slot the fp64 mean of its frame-f rows of ``pos``, rounded once, repeated C times"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_TRAJ)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_traj_mean(K.ptr(ptr), K.ptr(slots), ptr.numel() - 1, K.ptr(pos), pos.size(0), loc_mean.size(2),
                                           K.ptr(loc_mean), _stream(ptr.device)), "fastegnn_traj_mean")

    @staticmethod
    def gather_moved(ptr, slots, n_nodes, pos, kind, kind_scaled, loc_0, loc_t, vel_0, node_feat, node_attr, batch_out, motion,
                     has_t) -> None:
        """``gather`` with the rigid motion ``motion[b]`` (fp32 [B,12]: R row-major, then t) applied to slot b in the same launch, by
        the rule of ``apply_motion``; ``has_t`` false: no translation is added (the t values are not used)"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_TRAJ)
        B = ptr.numel() - 1
        if not (motion.is_cuda and motion.dtype == torch.float32 and tuple(motion.shape) == (B, 12) and motion.is_contiguous()):
            raise ValueError(f"fastegnn_amd: the motion rows of a batch of {B} samples must be a contiguous device fp32 [{B},12] tensor")
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_traj_gather_moved(K.ptr(ptr), K.ptr(slots), B, int(n_nodes), K.ptr(pos), pos.size(0), K.ptr(kind),
                                                   K.ptr(kind_scaled), kind.size(0), K.ptr(loc_0), K.ptr(loc_t), K.ptr(vel_0),
                                                   K.ptr(node_feat), K.ptr(node_attr), K.ptr(batch_out), K.ptr(motion), int(bool(has_t)),
                                                   _stream(ptr.device)), "fastegnn_traj_gather_moved")

    @staticmethod
    def mean_of(ptr, loc, loc_mean) -> None:
        """loc_mean [B,3,C] <- per slot the fp64 mean of the rows ``ptr[b] .. ptr[b+1]`` of ``loc`` [N,3], by ``mean``'s rule (the
        graph launch of csrc/rollout.hip without a score)"""
        if not ptr.is_cuda:
            raise RuntimeError(_NO_CPU_TRAJ)
        from . import _lib as K
        from .model import _stream
        K.check(K.lib().fastegnn_rollout_graph(K.ptr(ptr), ptr.numel() - 1, K.ptr(loc), None, loc.size(0), None, 0, None,
                                               loc_mean.size(2), K.ptr(loc_mean), None, _stream(ptr.device)), "fastegnn_rollout_graph")

    @staticmethod
    def edges(loc_0, ptr, ptr_host, radius, cutoff_rate):
        """(edge_index with global ids, dist) of the clouds ``loc_0[ptr[b]:ptr[b+1]]``: the two calls of ``_water3d_batch_edges``, in
        its order.  ``ptr`` is the device tensor the plan wrote and ``ptr_host`` the same offsets from the host's node counts: the
        device copy is handed on, so nothing is uploaded, and the calls cost their one read-back (the edge counts)."""
        from .graphs import _radius_graph_batch, cutoff_edges_batch
        ei, dist, edge_ptr, edge_ptr_host = _radius_graph_batch(loc_0, ptr, radius)
        ei, dist, _ = cutoff_edges_batch(ei, dist, edge_ptr, cutoff_rate, edge_ptr_host=edge_ptr_host)
        return ei, dist


_TRAJ_OPS = HipTrajOps


def _as_host_tensor(a) -> torch.Tensor:
    return a.detach() if isinstance(a, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(a))


def apply_motion(x: torch.Tensor, R, t=None) -> torch.Tensor:
    """The rigid-motion rule of include/fastegnn_hip.h ("rigid motions") in torch: for the rows of ``x`` [n,3]

        q[:, j] = (x[:, 0] * R[0, j] + x[:, 1] * R[1, j]) + x[:, 2] * R[2, j]           then  q + t  when ``t`` is given

    -- the reference's ``x @ R (+ t)`` in one fixed evaluation order.  Every product and sum is one eager elementwise fp32 operation,
    rounded by itself, so the result has the bits of ``fastegnn_traj_gather_moved`` / ``fastegnn_rollout_graph_moved`` on either
    device (``x @ R`` has not: a matrix product may fuse and reorder).  A position is moved with ``t``, a velocity without.  ``R``
    [3,3] and ``t`` [3]: arrays or tensors, taken to ``x``'s device as fp32."""
    R = torch.as_tensor(R).to(x.device, torch.float32)
    q = (x[:, 0:1] * R[0] + x[:, 1:2] * R[1]) + x[:, 2:3] * R[2]
    if t is not None:
        q = q + torch.as_tensor(t).to(x.device, torch.float32)
    return q


def _host_array(a, who: str) -> np.ndarray:
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    if a.dtype.kind not in "fiu" or not np.isfinite(a).all():
        raise ValueError(f"TrajectoryDataset: {who} must be finite numbers")
    return a.astype(np.float64)


def _axis_rotations(deg: np.ndarray, axis: int) -> np.ndarray:
    """fp64 [S,3,3]: the rotation by ``deg`` degrees about coordinate axis ``axis`` in the reference's sign convention
    (``utils/rotate.py``: about x and z the ``-sin`` stands above the diagonal, about y below it)"""
    th = np.radians(deg.astype(np.float64))
    c, s = np.cos(th), np.sin(th)
    a, b = [(1, 2), (2, 0), (0, 1)][axis]
    M = np.zeros((deg.size, 3, 3))
    M[:, axis, axis] = 1.0
    M[:, a, a], M[:, b, b], M[:, a, b], M[:, b, a] = c, c, -s, s
    return M


def _motion_table(S: int, rotation, translation, motion_seed):
    """(fp32 host array [S,12] = R row-major then t, has_t) of ``TrajectoryDataset(rotation=, translation=, motion_seed=)``, or
    (None, False) without either.  One generator, ``default_rng(motion_seed)``: first the angles of every sample (integer degrees
    from ``integers(0, 361)``: the reference's ``randint(0, 360)`` includes both ends), then the translations' ``standard_normal``."""
    if rotation is None and translation is None:
        return None, False
    rng = np.random.default_rng(motion_seed)
    if rotation is None:
        R = np.broadcast_to(np.eye(3), (S, 3, 3))
    elif isinstance(rotation, str):
        if rotation == "y":
            R = _axis_rotations(rng.integers(0, 361, size=S), 1)
        elif rotation == "xyz":
            deg = rng.integers(0, 361, size=(S, 3))
            R = _axis_rotations(deg[:, 0], 0) @ _axis_rotations(deg[:, 1], 1) @ _axis_rotations(deg[:, 2], 2)
        else:
            raise ValueError(f"TrajectoryDataset: rotation must be None, 'y', 'xyz' or a [3,3] / [S,3,3] array, got {rotation!r}")
    else:
        R = _host_array(rotation, "rotation")
        if R.shape not in ((3, 3), (S, 3, 3)):
            raise ValueError(f"TrajectoryDataset: a rotation array must be [3,3] or [{S},3,3], got {list(R.shape)}")
        R = np.broadcast_to(R, (S, 3, 3))
    table = np.zeros((S, 12), dtype=np.float32)
    table[:, :9] = R.reshape(S, 9)   # built in fp64, rounded once
    if translation is not None:
        if isinstance(translation, (np.ndarray, torch.Tensor)):   # values, applied as given
            t = _host_array(translation, "translation")
            if t.shape not in ((3,), (S, 3)):
                raise ValueError(f"TrajectoryDataset: a translation array must be [3] or [{S},3], got {list(t.shape)}")
            t = np.broadcast_to(t, (S, 3))
        else:                                                     # a scale: python numbers
            scale = _host_array(translation, "translation")
            if scale.shape not in ((), (3,)):
                raise ValueError(f"TrajectoryDataset: a translation scale must be a number or three, got {translation!r}")
            t = rng.standard_normal((S, 3)) * scale
        table[:, 9:] = t
    return table, translation is not None


class TrajectoryDataset:
    """Trajectories -- a fixed set of particles observed over T frames -- kept on ``device`` as what they are: ONE fp32 table ``pos``
    [rows,3] with every trajectory frame after frame, the particle kinds ``kind`` [sum n,1] and ``kind_scaled`` = ``kind / kind.max()``
    per trajectory, and per trajectory ``row0`` (its first row in ``pos``), ``n``, ``T`` and ``kind0`` (its first row in ``kind``) as
    int64 device tensors and as host arrays (``row0_host`` ...).  Every offset is 64-bit.  A sample is a pair (trajectory, start frame
    f) and stands for the graph of ``get_graph_step`` (``datasets/simulation/dataset.py:71-93``; ``datasets/protein/dataset.py:81-173``
    is the same recipe): ``loc_0 = pos[f]``, ``vel_0 = pos[f+1] - pos[f]``, ``loc_t = pos[f+delta_t]``, the radius graph of ``loc_0``
    reduced to its shortest ``1 - cutoff_rate`` fraction, edge length as edge attribute, node features ``[|vel|, kind / max kind]``.
    Nothing of that is stored: 12 bytes per particle and frame, against 48 per node plus 20 per edge and sample of a ``PackedDataset``.

    ``trajectories``: any iterable of ``(key, position [T,n,3], kind [n] or [n,1])`` -- what ``read_trajectories`` yields -- of numpy
    arrays or tensors; they may differ in n and T.  ``samples``: ``"all"`` (every start frame f with ``f + max(1, delta_t) <= T - 1``,
    trajectory by trajectory) or an integer array [S,2] of (trajectory index, start frame), validated here: the first pair outside
    raises ValueError.  ``len(ds)`` = S, ``ds.samples`` the host array, ``ds.frames`` the list of (trajectory key, start frame).

    ``ds[i]`` is the ``Frame`` that ``water3d_frame`` makes of the sample's slices (so ``collate`` and ``DataLoader`` work on the
    dataset).  ``ds.batch(ids)`` is the ``Batch`` of the samples ``ids``, with ``collate``'s keys in ``collate``'s order: the node
    tensors by three launches whatever the batch size (csrc/traj.hip), the graphs by the two batched calls of ``water3d_batch``,
    whose one read-back is the batch's only one.  ``vel_0`` and the copies are bit-equal to the per-sample path; ``node_feat[:,0]`` is
    ``sqrt((vx*vx + vy*vy) + vz*vz)`` with every operation rounded by itself, and ``loc_mean`` an fp64 sum in a fixed order rounded
    once (include/fastegnn_hip.h) -- within a unit in the last place of torch's reductions, not bit-equal to them.

    Rigid motions: the reference rotates and shifts its test partitions before it builds their graphs
    (``datasets/simulation/dataset.py:71-77``, ``datasets/protein/dataset.py:131-142``).  ``rotation``: None, ``"y"`` (a rotation about
    y by a whole number of degrees from [0, 360] per sample: ``random_rotate_y``), ``"xyz"`` (``random_rotate``: about x, then y, then
    z) or an array / tensor ``[3,3]`` (every sample) or ``[S,3,3]`` (per sample), applied as given.  ``translation``: None, a SCALE
    given as python numbers -- a float, or a tuple / list of three, one per axis: ``t = standard_normal(3) * scale`` per sample, the
    reference's ``randn(3) * box / 2`` with ``scale = box / 2`` -- or an ARRAY / tensor ``[3]`` or ``[S,3]`` of values, applied as
    given.  Non-finite or mis-shaped input raises ValueError.  The drawn forms use ``np.random.default_rng(motion_seed)``: the angles
    of all samples first, then the translations.  ``ds.motion``: the table fp32 ``[S,12]`` (R row-major, then t) on the device, built
    and uploaded once, or None.  With a table, ``batch`` / ``TrajectoryLoader`` / ``Rollout`` / ``ds[i]`` give the MOVED clouds
    (``apply_motion``'s rule, applied inside the gather, before the graph build: four launches for the node side); without one, exactly
    what they gave before."""

    def __init__(self, trajectories, virtual_channels, delta_t, radius, cutoff_rate=0.0, samples="all", device="cuda", rotation=None,
                 translation=None, motion_seed=0):
        self.virtual_channels, self.delta_t = int(virtual_channels), int(delta_t)
        self.radius, self.cutoff_rate, self.device = float(radius), float(cutoff_rate), torch.device(device)
        if self.device.type == "cuda" and self.device.index is None:   # (so that a tensor's device compares equal to it)
            self.device = torch.device("cuda", torch.cuda.current_device())
        if self.virtual_channels < 1 or self.delta_t < 0 or not self.radius > 0:
            raise ValueError("TrajectoryDataset: virtual_channels must be at least 1, delta_t at least 0 and radius positive")
        self.keys, pos_parts, kinds, scaled, n_of, T_of = [], [], [], [], [], []
        for key, position, kind in trajectories:
            p, k = _as_host_tensor(position), _as_host_tensor(kind)
            if p.dim() != 3 or p.size(2) != 3 or p.size(0) < 1:
                raise ValueError(f"TrajectoryDataset: trajectory {key!r}: position must be [T,n,3] with T >= 1, got {list(p.shape)}")
            if p.size(1) < 1:
                raise ValueError(f"TrajectoryDataset: trajectory {key!r} is an empty cloud (position {list(p.shape)})")
            if k.numel() != p.size(1):
                raise ValueError(f"TrajectoryDataset: trajectory {key!r}: {k.numel()} kinds for {p.size(1)} particles")
            k = k.to(self.device, torch.float32).reshape(-1, 1)
            self.keys.append(key)
            pos_parts.append(p)
            kinds.append(k)
            scaled.append(k / k.max())   # _node_feat's expression, once per trajectory
            n_of.append(p.size(1))
            T_of.append(p.size(0))
        if not self.keys:
            raise ValueError("TrajectoryDataset: no trajectory")
        self.n_host, self.T_host = np.asarray(n_of, dtype=np.int64), np.asarray(T_of, dtype=np.int64)
        self.row0_host = np.concatenate([[0], np.cumsum(self.n_host * self.T_host)[:-1]]).astype(np.int64)
        self.kind0_host = np.concatenate([[0], np.cumsum(self.n_host)[:-1]]).astype(np.int64)
        self.pos = torch.empty((int((self.n_host * self.T_host).sum()), 3), dtype=torch.float32, device=self.device)
        for p, r0 in zip(pos_parts, self.row0_host):   # one trajectory at a time: no second copy of the whole set anywhere
            self.pos[int(r0):int(r0) + p.size(0) * p.size(1)].copy_(p.reshape(-1, 3))
        del pos_parts
        self.kind, self.kind_scaled = torch.cat(kinds, 0).contiguous(), torch.cat(scaled, 0).contiguous()
        self.row0, self.n, self.T, self.kind0 = (torch.from_numpy(a).to(self.device) for a in
                                                 (self.row0_host, self.n_host, self.T_host, self.kind0_host))
        step = max(1, self.delta_t)
        if isinstance(samples, str):
            if samples != "all":
                raise ValueError(f"TrajectoryDataset: samples must be 'all' or an integer array [S,2], got {samples!r}")
            samples = np.asarray([(t, f) for t, T in enumerate(self.T_host) for f in range(int(T) - step)], dtype=np.int64).reshape(-1, 2)
        else:
            samples = samples.detach().cpu().numpy() if isinstance(samples, torch.Tensor) else np.asarray(samples)
            if samples.ndim != 2 or samples.shape[1] != 2 or samples.dtype.kind not in "iu":
                raise ValueError(f"TrajectoryDataset: samples must be an integer array [S,2], got {samples.dtype} {list(samples.shape)}")
            samples = samples.astype(np.int64)
        if samples.shape[0] == 0:
            raise ValueError("TrajectoryDataset: no sample (every trajectory is shorter than max(1, delta_t) + 1 frames?)")
        t, f = samples[:, 0], samples[:, 1]
        in_range = (t >= 0) & (t < len(self.keys))
        bad = ~in_range | (f < 0) | (f + step > self.T_host[np.where(in_range, t, 0)] - 1)
        if bad.any():
            i = int(np.argmax(bad))
            raise ValueError(f"TrajectoryDataset: sample {i} = (trajectory {int(t[i])}, start frame {int(f[i])}) is outside the data: "
                             f"{len(self.keys)} trajectories, and a start frame f needs 0 <= f and f + {step} <= T - 1")
        self.samples = np.ascontiguousarray(samples)
        self.samples_dev = torch.from_numpy(self.samples).to(self.device)
        self._node_cnt = self.n_host[t]
        self.frames = [(self.keys[int(a)], int(b)) for a, b in self.samples]
        table, self._has_t = _motion_table(self.samples.shape[0], rotation, translation, motion_seed)
        self.motion = None if table is None else torch.from_numpy(table).to(self.device)   # built once, uploaded once

    @classmethod
    def from_directory(cls, dataset_name, data_dir, virtual_channels, partition="train", max_samples=1e8, delta_t=15, cutoff_rate=0.0,
                       device="cuda", seed=0, radius=None, rotation=None, translation=None, motion_seed=0) -> "TrajectoryDataset":
        """The samples ``Simulation(dataset_name, data_dir, ..., seed=seed)`` draws, without building their graphs: the same
        ``read_trajectories`` pass and the same generator calls in the same order -- ``FRAMES_PER_TRAJECTORY`` start frames per
        trajectory from ``[0, min(250, T - 1 - max(1, delta_t))]``, cut at ``max_samples``, then one permutation -- so ``ds.frames``
        equals ``Simulation(...).frames`` and ``ds[i]`` equals ``Simulation(...)[i]``.  ``rotation`` / ``translation`` / ``motion_seed``
        are the constructor's; ``rotation="reference"`` is the reference's protocol for these sets (``datasets/simulation/dataset.py:71-77``):
        ``"y"`` for the ``test`` partition, none for the others."""
        if isinstance(rotation, str) and rotation == "reference":
            rotation = "y" if partition == "test" else None
        rng = np.random.default_rng(seed)
        delta_t, max_samples = int(delta_t), int(max_samples)
        trajectories, samples = [], []
        for key, position, particle_type in read_trajectories(os.path.join(data_dir, dataset_name), partition):
            n_frames = min(Simulation.FRAMES_PER_TRAJECTORY, max_samples - len(samples))
            last = min(250, np.asarray(position).shape[0] - 1 - max(1, delta_t))
            drawn = rng.integers(0, last + 1, size=max(n_frames, 0))
            samples.extend((len(trajectories), int(fr)) for fr in drawn)
            trajectories.append((key, position, particle_type))
            if len(samples) >= max_samples:
                break
        order = rng.permutation(len(samples))
        samples = np.asarray(samples, dtype=np.int64).reshape(-1, 2)[order]
        return cls(trajectories, virtual_channels, delta_t, Simulation.RADIUS if radius is None else radius, cutoff_rate, samples, device,
                   rotation=rotation, translation=translation, motion_seed=motion_seed)

    def __len__(self) -> int:
        return self.samples.shape[0]

    def __getitem__(self, i: int) -> Frame:
        S = len(self)
        i = int(i)
        if not -S <= i < S:
            raise IndexError(f"TrajectoryDataset: sample {i} of {S}")
        t, f = (int(v) for v in self.samples[i % S])
        n, r0, k0 = int(self.n_host[t]), int(self.row0_host[t]), int(self.kind0_host[t])
        at = lambda frame: self.pos[r0 + frame * n:r0 + (frame + 1) * n]  # noqa: E731
        loc_0, vel_0, loc_t = at(f), at(f + 1) - at(f), at(f + self.delta_t)
        if self.motion is not None:   # the clouds ``batch`` sees: the same rule, restated in torch
            R, t = self.motion[i % S, :9].view(3, 3), self.motion[i % S, 9:] if self._has_t else None
            loc_0, vel_0, loc_t = apply_motion(loc_0, R, t), apply_motion(vel_0, R), apply_motion(loc_t, R, t)
        return water3d_frame(loc_0, vel_0, loc_t, self.kind[k0:k0 + n], self.virtual_channels, self.radius, self.cutoff_rate)

    def _motion_rows(self, ids_dev: torch.Tensor, motion):
        """(device fp32 [B,12], has_t) of the batch ``ids_dev`` -- the rows of the dataset's table (one ``index_select`` on the device,
        nothing uploaded) or ``batch``'s explicit ``motion`` -- or (None, False) for an unmoved batch"""
        B = ids_dev.numel()
        if motion is None:
            return (None, False) if self.motion is None else (self.motion.index_select(0, ids_dev), self._has_t)
        who = "TrajectoryDataset.batch: motion"
        if isinstance(motion, (tuple, list)):
            if len(motion) != 2:
                raise ValueError(f"{who} must be a [B,12] tensor or a pair (R [B,3,3], t [B,3] or None)")
            R, t = motion
            R = torch.as_tensor(R).to(self.device, torch.float32)
            if tuple(R.shape) != (B, 3, 3):
                raise ValueError(f"{who}: R must be [{B},3,3], got {list(R.shape)}")
            has_t = t is not None
            t = torch.as_tensor(t).to(self.device, torch.float32) if has_t else torch.zeros((B, 3), dtype=torch.float32, device=self.device)
            if tuple(t.shape) != (B, 3):
                raise ValueError(f"{who}: t must be [{B},3], got {list(t.shape)}")
            rows = torch.cat([R.reshape(B, 9), t], 1)
        else:
            rows, has_t = torch.as_tensor(motion), True
            if tuple(rows.shape) != (B, 12) or rows.dtype != torch.float32:
                raise ValueError(f"{who} must be fp32 [{B},12] (R row-major, then t), got {rows.dtype} {list(rows.shape)}")
            rows = rows.to(self.device)   # (a tensor already there is used where it is)
        if not bool(torch.isfinite(rows).all()):   # (one read-back for a device tensor: non-finite positions must not reach the graph build)
            raise ValueError(f"{who} must be finite")
        return rows.contiguous(), has_t

    def _assemble_nodes(self, ids_dev: torch.Tensor, ids_host: np.ndarray, motion=None) -> dict:
        """the node side of the batch of the samples ``ids_dev`` (device int64 [B]; ``ids_host``: the same on the host, already
        validated): three device calls, sizes from the host's node counts, nothing uploaded or read back.  A moved batch (the
        dataset's table, or ``motion`` as ``batch`` takes it) is four: plan, the selection of the motion rows, the moved gather, the
        mean of the moved ``loc_0``; its dict also holds ``"motion"`` = (the rows fp32 [B,12], has_t)."""
        B, dev, C = int(ids_host.size), self.device, self.virtual_channels
        N = int(self._node_cnt[ids_host].sum())
        f32 = lambda *shape: torch.empty(shape, dtype=torch.float32, device=dev)  # noqa: E731
        out = {"loc_0": f32(N, 3), "loc_t": f32(N, 3), "vel_0": f32(N, 3), "node_feat": f32(N, 2), "node_attr": f32(N, 1),
               "loc_mean": f32(B, 3, C), "batch": torch.empty(N, dtype=torch.int64, device=dev),
               "ptr": torch.empty(B + 1, dtype=torch.int64, device=dev)}
        slots = torch.empty((B, _TRAJ_SLOT_WORDS), dtype=torch.int64, device=dev)
        ops = _TRAJ_OPS
        ops.plan(ids_dev, self.samples_dev, self.row0, self.n, self.T, self.kind0, self.delta_t, out["ptr"], slots)
        rows, has_t = self._motion_rows(ids_dev, motion)
        if rows is None:
            ops.gather(out["ptr"], slots, N, self.pos, self.kind, self.kind_scaled, *[out[k] for k in _NODE_KEYS], out["batch"])
            ops.mean(out["ptr"], slots, self.pos, out["loc_mean"])
        else:
            ops.gather_moved(out["ptr"], slots, N, self.pos, self.kind, self.kind_scaled, *[out[k] for k in _NODE_KEYS], out["batch"],
                             rows, has_t)
            ops.mean_of(out["ptr"], out["loc_0"], out["loc_mean"])
            out["motion"] = (rows, has_t)
        return out

    def _assemble(self, ids_dev: torch.Tensor, ids_host: np.ndarray, motion=None) -> Batch:
        out = self._assemble_nodes(ids_dev, ids_host, motion)
        ptr_host = [0] + np.cumsum(self._node_cnt[ids_host]).tolist()
        ei, dist = _TRAJ_OPS.edges(out["loc_0"], out["ptr"], ptr_host, self.radius, self.cutoff_rate)
        out["edge_attr"], out["edge_index"] = dist.unsqueeze(-1), ei
        return Batch(**{k: out[k] for k in _BATCH_KEYS})

    def batch(self, ids, motion=None) -> Batch:
        """The ``Batch`` of the samples ``ids``: a sequence of ints, a numpy array, or an int64 tensor on either side, with values in
        ``[0, len(self))`` (any order, repeats allowed), checked on the host as ``PackedDataset.batch`` does -- an id outside raises
        IndexError.  Host ids are uploaded through pinned memory; a device tensor is used where it is, and checking it costs one
        read-back (``TrajectoryLoader`` keeps both copies and pays neither).  ``motion`` overrides the dataset's motion table for this
        call: fp32 ``[B,12]`` (per slot R row-major, then t) or a pair ``(R [B,3,3], t [B,3] or None)``, on either device, finite
        (checked: one read-back when it lives on the device)."""
        return self._assemble(*self._checked_ids(ids), motion)

    def _checked_ids(self, ids, who: str = "TrajectoryDataset.batch"):
        """``batch``'s validation of ``ids`` -> (the ids on the device, the same as a host int64 array)"""
        ids_dev = None
        if isinstance(ids, torch.Tensor):
            if ids.device == self.device and ids.dtype == torch.int64 and ids.dim() == 1:
                ids_dev = ids.contiguous()
            ids = ids.detach().cpu().numpy()
        ids = np.asarray(ids)
        if ids.ndim != 1 or ids.size == 0:
            raise ValueError(f"{who}: ids must be a non-empty 1-D sequence")
        if ids.dtype.kind not in "iu":
            raise ValueError(f"{who}: ids must be integers, got {ids.dtype}")
        ids = ids.astype(np.int64)
        if ids.min() < 0 or ids.max() >= len(self):
            raise IndexError(f"{who}: ids span [{ids.min()}, {ids.max()}] but there are {len(self)} samples")
        if ids_dev is None or self.device.type != "cuda":
            ids_dev = _upload_ids(torch.from_numpy(ids), self.device)
        return ids_dev, ids


class TrajectoryLoader:
    """``DataLoader`` over a ``TrajectoryDataset``, as ``PackedLoader`` is over a packed one: same batching, same
    ``torch.randperm(n, generator=...)`` order (equal generators give the samples of ``DataLoader(ds, ...)``'s batches in the same
    order).  The epoch's order is uploaded ONCE, through pinned memory with a non-blocking copy; every batch hands the kernels a slice
    of that device tensor.  A batch is the three launches of its node side plus the batched graph build, whose read-back of the edge
    counts is the only synchronisation.  ``state_dict`` / ``load_state_dict`` hold the generator, so ``save_checkpoint(loaders=...)``
    and ``fit(resume=True)`` take the loader as they take the others."""

    def __init__(self, ds: TrajectoryDataset, batch_size=1, shuffle=False, drop_last=False, generator: Optional[torch.Generator] = None):
        self.dataset, self.batch_size, self.shuffle, self.drop_last, self.generator = ds, int(batch_size), shuffle, drop_last, generator

    def __len__(self) -> int:
        n = len(self.dataset)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self) -> Iterator[Batch]:
        n = len(self.dataset)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        ids_dev, order_host = _upload_ids(order, self.dataset.device), order.numpy()
        for i in range(len(self)):
            a, b = i * self.batch_size, min((i + 1) * self.batch_size, n)
            yield self.dataset._assemble(ids_dev[a:b], order_host[a:b])

    def state_dict(self) -> dict:
        return _generator_state(self.generator)

    def load_state_dict(self, state) -> None:
        _load_generator_state(self.generator, state, "TrajectoryLoader")
