"""Graph construction on the GPU: what the Water-3D dataset does per frame on
the host (``datasets/simulation/dataset.py:80,96-101``) -- ``radius_graph(r)`` without self loops and the
"keep the shortest (1 - cutoff_rate) fraction" cutoff -- as C-ABI calls of ``libfastegnn_hip.so``."""
from __future__ import annotations

import ctypes as C
from typing import Tuple

import torch

from . import _lib as K
from .model import _stream


def radius_graph(loc: torch.Tensor, r: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """All ordered pairs (i, j != i) with ||loc_i - loc_j|| <= r (decided on the fp32 squared distance).
    Returns (edge_index int64 [2,E] grouped by edge_index[0] with ascending edge_index[1], dist fp32 [E])."""
    assert loc.is_cuda and loc.dim() == 2 and loc.size(1) == 3
    loc = loc.contiguous().float()
    N, dev = loc.size(0), loc.device
    L = K.lib()
    nbytes = L.fastegnn_radius_graph_ws_bytes(N)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    E = C.c_int64(0)
    st = _stream(dev)
    K.check(L.fastegnn_radius_graph_count(K.ptr(loc), N, float(r), K.ptr(ws), nbytes, C.byref(E), st),
            "fastegnn_radius_graph_count")
    ei = torch.empty(2, E.value, dtype=torch.int64, device=dev)
    dist = torch.empty(E.value, dtype=torch.float32, device=dev)
    K.check(L.fastegnn_radius_graph_fill(K.ptr(loc), N, float(r), K.ptr(ws), nbytes, E.value, K.ptr(ei), K.ptr(dist),
                                         st), "fastegnn_radius_graph_fill")
    return ei, dist


def cutoff_edges(edge_index: torch.Tensor, dist: torch.Tensor, cutoff_rate: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """Keep the ``int(E * (1 - cutoff_rate))`` shortest edges, in ascending length (cutoff_edge of the
    reference datasets); equal lengths keep their input order."""
    E = edge_index.size(1)
    keep = int(E * (1 - cutoff_rate))
    dev = edge_index.device
    out = torch.empty(2, keep, dtype=torch.int64, device=dev)
    dout = torch.empty(keep, dtype=torch.float32, device=dev)
    if keep:
        L = K.lib()
        nbytes = L.fastegnn_cutoff_tmp_bytes(E)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        K.check(L.fastegnn_cutoff_edges(K.ptr(edge_index.contiguous()), K.ptr(dist.contiguous()), E, keep, K.ptr(out),
                                        K.ptr(dout), K.ptr(tmp), nbytes, _stream(dev)), "fastegnn_cutoff_edges")
    return out, dout


def _device_ptr(ptr, dev) -> torch.Tensor:
    return torch.as_tensor(ptr, dtype=torch.int64).to(dev).contiguous()


def _radius_graph_batch(loc: torch.Tensor, ptr, r: float):
    """radius_graph_batch plus the host copy of edge_ptr that its one read-back delivered (a list of B+1 ints)."""
    if not (isinstance(loc, torch.Tensor) and loc.is_cuda):
        raise RuntimeError("fastegnn_amd: radius_graph_batch needs a device tensor (there is no CPU fallback)")
    if loc.dim() != 2 or loc.size(1) != 3:
        raise RuntimeError(f"fastegnn_amd: radius_graph_batch: loc must be [N,3], got {list(loc.shape)}")
    loc = loc.contiguous().float()
    N, dev = loc.size(0), loc.device
    ptr = _device_ptr(ptr, dev)
    if ptr.dim() != 1 or ptr.numel() < 1:
        raise RuntimeError("fastegnn_amd: radius_graph_batch: ptr must be int64 [B+1]")
    B = ptr.numel() - 1
    L = K.lib()
    nbytes = L.fastegnn_radius_graph_batch_ws_bytes(N, B)
    ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
    host = (C.c_int64 * (B + 1))()
    st = _stream(dev)
    K.check(L.fastegnn_radius_graph_batch_count(K.ptr(loc), K.ptr(ptr), N, B, float(r), K.ptr(ws), nbytes, host, st),
            "fastegnn_radius_graph_batch_count")
    E = host[B]
    ei = torch.empty(2, E, dtype=torch.int64, device=dev)
    dist = torch.empty(E, dtype=torch.float32, device=dev)
    edge_ptr = torch.empty(B + 1, dtype=torch.int64, device=dev)
    K.check(L.fastegnn_radius_graph_batch_fill(K.ptr(loc), K.ptr(ptr), N, B, float(r), K.ptr(ws), nbytes, E, K.ptr(ei),
                                               K.ptr(dist), K.ptr(edge_ptr), st), "fastegnn_radius_graph_batch_fill")
    return ei, dist, edge_ptr, list(host)


def radius_graph_batch(loc: torch.Tensor, ptr, r: float) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``radius_graph`` of B ragged clouds in one call (the counterpart of ``torch_cluster.radius_graph(x, r, batch)``):
    ``loc`` [N,3] holds the clouds back to back, ``ptr`` int64 [B+1] (tensor on either side, or a list) their node ranges,
    ``0 = ptr[0] <= ... <= ptr[B] = N``.  Returns (edge_index int64 [2,E] with global node ids, dist fp32 [E], edge_ptr int64
    [B+1] on the device): graph b owns the edges ``edge_ptr[b] .. edge_ptr[b+1]``, which are ``radius_graph(loc[ptr[b]:ptr[b+1]],
    r)`` shifted by ``ptr[b]``; no edge joins two graphs.  One host read-back for the whole batch; a malformed ``ptr`` raises."""
    return _radius_graph_batch(loc, ptr, r)[:3]


def keep_ptr_of(edge_ptr_host, cutoff_rate: float) -> list:
    """Prefix sums of the per-graph keep counts ``int(E_b * (1 - cutoff_rate))`` (Python floats, as the reference computes them)."""
    keep = [0]
    for a, b in zip(edge_ptr_host, edge_ptr_host[1:]):
        keep.append(keep[-1] + int((b - a) * (1 - cutoff_rate)))
    return keep


def cutoff_edges_batch(edge_index: torch.Tensor, dist: torch.Tensor, edge_ptr, cutoff_rate: float,
                       edge_ptr_host=None) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """``cutoff_edges`` per graph of a batched edge list: graph b keeps its ``int(E_b * (1 - cutoff_rate))`` shortest edges in
    ascending length, equal lengths in their input order.  Returns (edge_index, dist, edge_ptr of the kept list).  The keep
    counts are computed on the host from the per-graph edge counts: pass them as ``edge_ptr_host`` (a list of B+1 ints, or
    give ``edge_ptr`` as a CPU tensor) and the call reads nothing back; a device ``edge_ptr`` alone costs one read-back."""
    if not (isinstance(edge_index, torch.Tensor) and edge_index.is_cuda and dist.is_cuda):
        raise RuntimeError("fastegnn_amd: cutoff_edges_batch needs device tensors (there is no CPU fallback)")
    dev = edge_index.device
    if edge_ptr_host is None:
        edge_ptr_host = torch.as_tensor(edge_ptr).tolist()
    eph = [int(v) for v in edge_ptr_host]
    B, E = len(eph) - 1, edge_index.size(1)
    if B < 0 or eph[0] != 0 or eph[B] != E or any(a > b for a, b in zip(eph, eph[1:])):
        raise RuntimeError("fastegnn_amd: cutoff_edges_batch: edge_ptr is not 0 = edge_ptr[0] <= ... <= edge_ptr[B] = E")
    keep = keep_ptr_of(eph, cutoff_rate)
    keep_total = keep[-1]
    keep_ptr = torch.tensor(keep, dtype=torch.int64).to(dev)
    out = torch.empty(2, keep_total, dtype=torch.int64, device=dev)
    dout = torch.empty(keep_total, dtype=torch.float32, device=dev)
    if keep_total:
        L = K.lib()
        edge_ptr = _device_ptr(edge_ptr, dev)
        nbytes = L.fastegnn_cutoff_batch_tmp_bytes(E, B)
        tmp = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        K.check(L.fastegnn_cutoff_edges_batch(K.ptr(edge_index.contiguous()), K.ptr(dist.contiguous().float()), K.ptr(edge_ptr),
                                              K.ptr(keep_ptr), B, E, keep_total, K.ptr(out), K.ptr(dout), K.ptr(tmp), nbytes,
                                              _stream(dev)), "fastegnn_cutoff_edges_batch")
    return out, dout, keep_ptr


NBODY_MAX_PARTICLES = 128


def nbody_cutoff_edges(loc: torch.Tensor, k: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """For each system of ``loc`` [S,n,3] (n <= 128) the ``k`` shortest ordered pairs of the complete graph without self
    loops, in ascending length (``datasets/nbody/dataset.py:102-113``: cdist + cutoff_edge on the host).  Returns
    (edge_index int64 [S,2,k] with ids local to the system, dist fp32 [S,k]); equal lengths come in ascending i*n+j."""
    assert loc.is_cuda and loc.dim() == 3 and loc.size(2) == 3
    loc = loc.contiguous().float()
    S, n, dev = loc.size(0), loc.size(1), loc.device
    ei = torch.empty(S, 2, k, dtype=torch.int64, device=dev)
    dist = torch.empty(S, k, dtype=torch.float32, device=dev)
    K.check(K.lib().fastegnn_nbody_cutoff_edges(K.ptr(loc), S, n, k, K.ptr(ei), K.ptr(dist), _stream(dev)),
            "fastegnn_nbody_cutoff_edges")
    return ei, dist
