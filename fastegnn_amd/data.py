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
  is two kernel launches (csrc/collate.hip) whatever its size, with no host-to-device copy and no synchronisation.

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

    def to(self, device, non_blocking: bool = False) -> "Batch":
        return Batch(**{k: v.to(device, non_blocking=non_blocking) for k, v in self._t.items()})

    def detach(self) -> "Batch":
        return Batch(**{k: v.detach() for k, v in self._t.items()})

    def pin_memory(self) -> "Batch":
        return Batch(**{k: v.pin_memory() for k, v in self._t.items()})

    def __repr__(self) -> str:
        return "Batch(" + ", ".join(f"{k}={list(v.shape)}" for k, v in self._t.items()) + ")"


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


# ---- device-resident packed datasets: a batch is two launches, whatever B is (csrc/collate.hip) ----
_PACK_KEYS = _NODE_KEYS + ("edge_attr", "loc_mean", "edge_index")   # FASTEGNN_COLLATE_* order (include/fastegnn_hip.h)
_NO_CPU = "fastegnn_amd: PackedDataset.batch needs device-resident tables (there is no CPU fallback)"


class HipCollateOps:
    """The two device calls of a packed batch on libfastegnn_hip.so (the product path).  tests/packed_ref.py restates them in
    torch so that tests/test_packed_cpu.py can drive the loader's orchestration without a GPU (the ``wide.HipOps`` precedent)."""

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


_COLLATE_OPS = HipCollateOps


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

    def __len__(self) -> int:
        return self.node_ptr_host.size - 1

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

    def _assemble(self, ids_dev: torch.Tensor, ids_host: np.ndarray) -> Batch:
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
        return Batch(**out)

    def batch(self, ids) -> Batch:
        """``collate([self[i] for i in ids])``: same keys in the same order, every tensor fresh and contiguous.  ``ids``: a host
        sequence, numpy array or CPU tensor of frame numbers in ``[0, len(self))`` (any order, repeats allowed), checked on the
        host: an id outside raises IndexError.  Two kernel launches and the upload of ``ids``; nothing is read back."""
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
        return self._assemble(self._upload(torch.from_numpy(ids)), ids)


class PackedLoader:
    """``DataLoader`` over a ``PackedDataset``: same batching, same ``torch.randperm(n, generator=...)`` order (equal generators
    give the same batches in the same order).  The epoch's order is uploaded ONCE, through pinned memory with a non-blocking
    copy; every batch hands the kernels a slice of that device tensor, so a batch is two launches and no copy."""

    def __init__(self, packed: PackedDataset, batch_size=1, shuffle=False, drop_last=False,
                 generator: Optional[torch.Generator] = None):
        self.packed, self.batch_size, self.shuffle, self.drop_last = packed, int(batch_size), shuffle, drop_last
        self.generator = generator

    def __len__(self) -> int:
        n = len(self.packed)
        return n // self.batch_size if self.drop_last else math.ceil(n / self.batch_size)

    def __iter__(self) -> Iterator[Batch]:
        n = len(self.packed)
        order = torch.randperm(n, generator=self.generator) if self.shuffle else torch.arange(n)
        ids_dev, order_host = self.packed._upload(order), order.numpy()
        for i in range(len(self)):
            a, b = i * self.batch_size, min((i + 1) * self.batch_size, n)
            yield self.packed._assemble(ids_dev[a:b], order_host[a:b])
