"""Times one epoch of data.DataLoader (per batch: B slices, eight torch.cat calls, two copies from pageable memory) against one
epoch of data.PackedLoader (per batch: two launches of csrc/collate.hip) over the SAME device-resident frames on one GPU.  Host
wall clock around an epoch that ends in one device synchronise; both loaders warmed up, then alternated in one process; the
median of EPOCHS epochs with min, max and inter-quartile range (the box's epoch-to-epoch spread).  Each shape twice: the loader
alone (every batch is dropped as soon as it is built), and the loader with train_step on every batch.  Three shapes from seeds:
cfg1-like and cfg2-like N-body frames at batch size 100, Water-3D-like clouds (r = 0.035 graphs of graphs.radius_graph_batch)
at batch size 20.  The batches of the two loaders are compared with torch.equal first.  A third loader,
PackedLoader(graphs=model.deterministic_for), hands every batch over with its sorted graph assembled from indices sorted once
(PackedDataset.build_graphs), so that train_step sorts nothing: its graphs are compared with the model's own first, and it
alternates with the other two.  Prints what profiles/packed_loader_graphs.txt holds (profiles/packed_loader.txt: the same without
the third loader).  At the two N-body shapes, whose frames are equal-sized, a fourth loader alternates with them:
data.PackedStream(graphs=model.deterministic_for) -- static buffers, the order drawn on the device, three launches per batch -- whose
yardstick is the third loader in the same call; its gather (+ chunk launch) is timed under the library's events against the third
loader's gather + graph launches and a copy_ of the same bytes (profiles/packed_stream.txt).

    python tools/gpu_loader_timing.py [output file]
"""
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import fastegnn_amd  # noqa: E402
from fastegnn_amd import data as D  # noqa: E402
from fastegnn_amd.graphs import radius_graph_batch  # noqa: E402
from fastegnn_amd.train import FusedAdam, MMDSampler, train_step  # noqa: E402

EPOCHS, WARM, C = 15, 2, 3


def _frame(loc_0, ei, gen):
    n = loc_0.size(0)
    vel = torch.randn(n, 3, generator=gen) * 0.01
    kind = torch.randint(0, 2, (n, 1), generator=gen).float() + 1.0
    ea = (loc_0[ei[0]] - loc_0[ei[1]]).norm(dim=1, keepdim=True)
    return D.Frame(ei, ea, loc_0, loc_0 + 10 * vel, vel, D._node_feat(vel, kind), kind, D._loc_mean(loc_0, C))


def nbody_frames(n_frames, n, seed):
    gen = torch.Generator().manual_seed(seed)
    ij = torch.tensor([(i, j) for i in range(n) for j in range(n) if i != j], dtype=torch.int64).t().contiguous()
    return [_frame(torch.randn(n, 3, generator=gen), ij, gen).to("cuda") for _ in range(n_frames)]


def water_frames(n_frames, seed, per_call=15):
    gen = torch.Generator().manual_seed(seed)
    frames = []
    for at in range(0, n_frames, per_call):
        sizes = torch.randint(7600, 8401, (min(per_call, n_frames - at),), generator=gen).tolist()
        clouds = [torch.rand(n, 3, generator=gen) * 0.42 for n in sizes]
        ptr = [0]
        for n in sizes:
            ptr.append(ptr[-1] + n)
        ei, _, ep = radius_graph_batch(torch.cat(clouds, 0).cuda(), ptr, 0.035)
        ei, ep = ei.cpu(), ep.tolist()
        frames += [_frame(c, ei[:, a:b] - o, gen).to("cuda") for c, o, a, b in zip(clouds, ptr, ep, ep[1:])]
    return frames


def gather_kernel_us(packed, ids, runs=20):
    """the gather launch of one batch by itself: outputs allocated once, the plan run once, then `runs` launches under the
    library's per-launch HIP events (fastegnn_profile_enable) -> (mean microseconds, launches counted)"""
    from fastegnn_amd import _lib as K
    b = packed.batch(ids)
    ids_dev = ids.cuda()
    edge_ptr = torch.empty_like(b["ptr"])
    ops, T = D._COLLATE_OPS, packed.tables
    ops.plan(ids_dev, packed.node_ptr, packed.edge_ptr, b["ptr"], edge_ptr)
    args = (ids_dev, packed.node_ptr, packed.edge_ptr, b["ptr"], edge_ptr, [T[k] for k in D._PACK_KEYS],
            [b[k] for k in D._PACK_KEYS], b["batch"])
    for _ in range(3):
        ops.gather(*args)
    torch.cuda.synchronize()
    K.lib().fastegnn_profile_enable(1)
    K.profile_collect()
    for _ in range(runs):
        ops.gather(*args)
    K.lib().fastegnn_profile_enable(0)
    ms, n = K.profile_collect()["misc"]
    return ms / n * 1e3, n


def _misc_us(call, runs):
    """`runs` calls of `call` under the library's per-launch HIP events -> (microseconds per call, event pairs counted)"""
    from fastegnn_amd import _lib as K
    for _ in range(3):
        call()
    torch.cuda.synchronize()
    K.lib().fastegnn_profile_enable(1)
    K.profile_collect()
    for _ in range(runs):
        call()
    K.lib().fastegnn_profile_enable(0)
    ms, n = K.profile_collect()["misc"]
    return ms / runs * 1e3, n


def _graph_arrays(g):
    return [g.rowptr, g.erow, g.col, g.perm, g.cscptr, g.csc_eid]


def _batch_bytes(batch):
    """bytes read + written by the assembly of a batch with its graph: every output once in, once out (ptr / batch are written only
    by the ragged gather and not at all by the uniform one: left out on both sides); rowptr / cscptr are read as int64"""
    out = sum(batch[k].numel() * batch[k].element_size() for k in D._PACK_KEYS)
    arrays = [a for a in _graph_arrays(batch["graph"]) if a is not None]
    out += sum(a.numel() * 4 for a in arrays)
    extra = sum(a.numel() * 4 for a in (batch["graph"].rowptr, batch["graph"].cscptr) if a is not None)
    return 2 * out + extra


def ragged_gather_graph_us(packed, ids, graphs, runs=20):
    """PackedLoader's gather + graph launches of one batch (outputs allocated once, the plan run once) -> (us per batch, event pairs)"""
    b = packed.batch(ids, graphs=graphs)
    ids_dev, g = ids.cuda(), b["graph"]
    edge_ptr = torch.empty_like(b["ptr"])
    ops, T, G = D._COLLATE_OPS, packed.tables, packed.graph_tables
    ops.plan(ids_dev, packed.node_ptr, packed.edge_ptr, b["ptr"], edge_ptr)
    n_edges = b["edge_index"].size(1)

    def call():
        ops.gather(ids_dev, packed.node_ptr, packed.edge_ptr, b["ptr"], edge_ptr, [T[k] for k in D._PACK_KEYS],
                   [b[k] for k in D._PACK_KEYS], b["batch"])
        ops.graph(ids_dev, packed.node_ptr, packed.edge_ptr, b["ptr"], edge_ptr, b.num_nodes, n_edges, [G[k] for k in D._GRAPH_KEYS],
                  _graph_arrays(g), g.chunk_row)
    return _misc_us(call, runs)


def uniform_gather_us(stream, runs=20):
    """PackedStream's gather + chunk launches of one batch, the ids of its latest draw -> (us per batch, event pairs)"""
    nodes, edges = stream.frame_shape
    stream.next()

    def call():
        D._COLLATE_OPS.gather_uniform(stream.ids, len(stream.packed), nodes, edges, stream._src, stream._dst, stream._src_graph,
                                      stream._dst_graph, stream._chunk_row, call=stream._call)
    return _misc_us(call, runs)


def spread(ts):
    return f"[{min(ts) * 1e3:.3f} .. {max(ts) * 1e3:.3f}] ms"


def copy_us(nbytes, runs=20):
    """a plain device-to-device copy of nbytes (torch's copy kernel), device events around `runs` of them -> microseconds each"""
    src = torch.rand(nbytes // 4, device="cuda")
    dst = torch.empty_like(src)
    for _ in range(3):
        dst.copy_(src)
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(runs):
        dst.copy_(src)
    b.record()
    b.synchronize()
    return a.elapsed_time(b) / runs * 1e3


def epoch_times(loaders, body):
    """alternates the loaders: EPOCHS timed epochs each after WARM warm-ups -> {name: [seconds]}"""
    ts = {name: [] for name, _ in loaders}
    for it in range(WARM + EPOCHS):
        for name, loader in loaders:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for batch in loader:
                body(batch)
            torch.cuda.synchronize()
            if it >= WARM:
                ts[name].append(time.perf_counter() - t0)
    return ts


def line(name, ts, n_batches):
    q = statistics.quantiles(ts, n=4)
    med = statistics.median(ts)
    return (f"    {name:<12} median {med * 1e3:9.3f} ms per epoch ({med / n_batches * 1e6:9.1f} us per batch)   min {min(ts) * 1e3:9.3f}  "
            f"max {max(ts) * 1e3:9.3f}  IQR {(q[2] - q[0]) * 1e3:8.3f} ms   of {len(ts)} epochs after {WARM} warm-ups")


def main():
    out = [f"device: {torch.cuda.get_device_name(0)}; host wall clock around one epoch ending in one device synchronise; "
           f"the loaders alternate in one process"]
    shapes = [("cfg1-like: 2000 frames x 5 nodes x 20 edges, batch size 100", lambda: nbody_frames(2000, 5, 1), 100),
              ("cfg2-like: 500 frames x 100 nodes x 9900 edges, batch size 100", lambda: nbody_frames(500, 100, 2), 100),
              ("Water-3D-like: 60 frames x 7600..8400 nodes, r = 0.035 in a 0.42^3 box, batch size 20", lambda: water_frames(60, 3), 20)]
    for name, make, bs in shapes:
        frames = make()
        packed = D.PackedDataset(frames)
        old = D.DataLoader(frames, batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(9))
        new = D.PackedLoader(packed, batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(9))
        same = all(list(a.keys()) == list(b.keys()) and all(torch.equal(a[k], b[k]) for k in a.keys()) for a, b in zip(new, old))
        nb = len(new)
        first = next(iter(new))
        bytes_moved = 2 * sum(first[k].numel() * first[k].element_size() for k in first.keys())
        out.append(f"{name}")
        out.append(f"  {nb} batches per epoch; first batch: {first.num_nodes} nodes, {first['edge_index'].size(1)} edges, "
                   f"{bytes_moved / 1e6:.2f} MB read + written; PackedLoader batches equal DataLoader's (torch.equal, every key): {same}")
        # the gather kernel by itself on the first batch (device events around the two launches, outputs allocated outside)
        ids = torch.randperm(len(frames), generator=torch.Generator().manual_seed(4))[:bs]
        ev = []
        for _ in range(23):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            packed.batch(ids)
            b.record()
            b.synchronize()
            ev.append(a.elapsed_time(b))
        ev = ev[3:]
        out.append(f"  PackedDataset.batch (id upload + plan + gather, device events): median {statistics.median(ev) * 1e3:.1f} us "
                   f"(min {min(ev) * 1e3:.1f}, max {max(ev) * 1e3:.1f}) of 20 after 3 warm-ups = "
                   f"{bytes_moved / statistics.median(ev) / 1e6:.0f} GB/s read + written at the median")
        us, n = gather_kernel_us(packed, ids)
        out.append(f"  the gather launch alone (HIP events around the launch, the library's profiler): {us:.1f} us mean of {n} = "
                   f"{bytes_moved / us / 1e3:.0f} GB/s read + written;  a torch copy_ of the same bytes: "
                   f"{bytes_moved / copy_us(bytes_moved // 2) / 1e3:.0f} GB/s")
        model = fastegnn_amd.FastEGNN(node_feat_nf=2, node_attr_nf=0, edge_attr_nf=2, hidden_nf=64, virtual_channels=C,
                                      device="cuda", n_layers=4)
        # the third loader: every batch with the sorted graph the model would build (the same edge-backward form: deterministic_for)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        packed.build_graphs()
        torch.cuda.synchronize()
        t_pack = time.perf_counter() - t0
        g_bytes = sum(t.numel() * t.element_size() for t in packed.graph_tables.values())
        gl = D.PackedLoader(packed, batch_size=bs, shuffle=True, generator=torch.Generator().manual_seed(9), graphs=model.deterministic_for)
        arrays = ("rowptr", "erow", "col", "perm", "cscptr", "csc_eid")
        same_g = True
        for b in gl:
            want, got = model.sorted_graph(b["edge_index"], b.num_nodes), b["graph"]
            same_g &= got.n_chunks == want.n_chunks and (got.cscptr is None) == (want.cscptr is None)
            same_g &= all(torch.equal(getattr(got, k), getattr(want, k)) for k in arrays if getattr(want, k) is not None)
            same_g &= torch.equal(got.chunk_row[:got.n_chunks + 1], want.chunk_row[:want.n_chunks + 1])
        model._graph_cache.clear()
        out.append(f"  build_graphs (once per dataset): {t_pack * 1e3:.1f} ms, {g_bytes / 1e6:.2f} MB of per-frame sorted indices; "
                   f"col-keyed index in the first batch: {model.deterministic_for(first['edge_index'].size(1))}; assembled graphs "
                   f"equal the model's own (torch.equal, every array, every batch): {same_g}")
        loaders = [("DataLoader", old), ("PackedLoader", new), ("Packed+graph", gl)]
        stream = None
        if packed.frame_shape is not None:   # equal-sized frames: the stream, with the graph the third loader carries
            stream = D.PackedStream(packed, bs, shuffle=True, seed=9, graphs=model.deterministic_for)
            loaders.append(("PackedStream", stream))
            sb = stream.next()
            want = D.collate([packed[int(i)] for i in stream.ids.tolist()])
            same_s = all(torch.equal(sb[k], want[k]) for k in want.keys())
            wg, got = model.sorted_graph(sb["edge_index"], sb.num_nodes), sb["graph"]
            same_s &= all(torch.equal(getattr(got, k), getattr(wg, k)) for k in arrays if getattr(wg, k) is not None)
            model._graph_cache.clear()
            nbytes = _batch_bytes(sb)
            us_u, n_u = uniform_gather_us(stream)
            us_r, n_r = ragged_gather_graph_us(packed, ids, model.deterministic_for)
            out.append(f"  PackedStream: {len(stream)} full batches per epoch; its batch equals collate of its ids and its graph the model's "
                       f"own (torch.equal): {same_s}")
            out.append(f"  one batch with its graph, {nbytes / 1e6:.2f} MB read + written, the library's event pairs (mean of 20 batches): "
                       f"uniform gather + chunk launch {us_u:.1f} us ({n_u} pairs) = {nbytes / us_u / 1e3:.0f} GB/s;  PackedLoader's gather + graph "
                       f"launches {us_r:.1f} us ({n_r} pairs) = {nbytes / us_r / 1e3:.0f} GB/s;  a torch copy_ of the same bytes: "
                       f"{nbytes / copy_us(nbytes // 2) / 1e3:.0f} GB/s")
        out.append("  loader alone:")
        ts = epoch_times(loaders, lambda batch: None)
        out += [line(k, ts[k], nb) for k, _ in loaders]
        if stream is not None:
            below = max(ts["PackedStream"]) < min(ts["Packed+graph"])
            out.append(f"    PackedStream {spread(ts['PackedStream'])} against Packed+graph {spread(ts['Packed+graph'])}: wholly below: {below}")
        opt = FusedAdam(model.parameters(), lr=5e-4, weight_decay=1e-12)
        smp = MMDSampler(0)
        out.append("  loader + train_step (FastEGNN hidden 64, 4 layers, C = 3, device-side MMD sample):")
        ts = epoch_times(loaders, lambda batch: train_step(model, opt, batch, None, sigma=1.0, weight=0.01, sampler=smp,
                                                           num_sample=3 * C))
        out += [line(k, ts[k], nb) for k, _ in loaders]
        if stream is not None:
            below = max(ts["PackedStream"]) < min(ts["Packed+graph"])
            out.append(f"    PackedStream {spread(ts['PackedStream'])} against Packed+graph {spread(ts['Packed+graph'])}: wholly below: {below}")
        del frames, packed, old, new, gl, stream, model, opt
        torch.cuda.empty_cache()
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
