"""Times the batched graph build (graphs.radius_graph_batch + cutoff_edges_batch: one call for B clouds) against the per-frame
loop (graphs.radius_graph + cutoff_edges, one call per cloud) on one GPU: HIP events around the Python entry points, workspace
allocation included, median of 20 runs after 3 warm-ups, each pair twice (the second pass shows the run-to-run band).
Two shapes: 15 Water-3D-sized frames and 20 protein backbones.  Prints what profiles/graphs_batch.txt holds.

    python tools/gpu_graphs_batch_timing.py [output file]
"""
import os
import statistics
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from fastegnn_amd import _lib as K  # noqa: E402
from fastegnn_amd.graphs import (_radius_graph_batch, cutoff_edges, cutoff_edges_batch, radius_graph,  # noqa: E402
                                 radius_graph_batch)

SHAPES = [("water3d 15 x 8000, r=0.035, box 0.42^3", 15, 8000, 0.035, 0.42, 0.25),
          ("backbone 20 x 855, r=10, box 36^3", 20, 855, 10.0, 36.0, 0.25)]


def timed(fn, warm=3, runs=20):
    for _ in range(warm):
        fn()
    ts = []
    for _ in range(runs):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return statistics.median(ts), min(ts), max(ts)


def main():
    out = []
    for name, B, n, r, box, rate in SHAPES:
        g = torch.Generator().manual_seed(1)
        clouds = [(torch.rand(n, 3, generator=g) * box).cuda() for _ in range(B)]
        loc = torch.cat(clouds, 0)
        ptr = [i * n for i in range(B + 1)]
        ptr_dev = torch.tensor(ptr).cuda()

        def batched():
            ei, d, ep, eph = _radius_graph_batch(loc, ptr_dev, r)
            return cutoff_edges_batch(ei, d, ep, rate, edge_ptr_host=eph)

        def loop():
            return [cutoff_edges(*radius_graph(c, r), rate) for c in clouds]

        bb, ll = batched(), loop()
        same = (torch.equal(bb[0], torch.cat([x[0] + o for x, o in zip(ll, ptr)], 1))
                and torch.equal(bb[1], torch.cat([x[1] for x in ll])))
        L = K.lib()
        E = radius_graph_batch(loc, ptr_dev, r)[0].shape[1]
        out.append(f"{name}: E = {E} before the cutoff, kept {bb[0].shape[1]}; batched result equals the per-frame loop's: {same}")
        out.append(f"  workspace bytes: batched radius graph {L.fastegnn_radius_graph_batch_ws_bytes(B * n, B)} (one call), "
                   f"single cloud {L.fastegnn_radius_graph_ws_bytes(n)} (per frame); cutoff tmp batched "
                   f"{L.fastegnn_cutoff_batch_tmp_bytes(E, B)}, single {L.fastegnn_cutoff_tmp_bytes(E // B)} (per frame, mean E)")
        for label, fn in [("(a) batched radius graph + cutoff", batched), ("(b) per-frame loop radius graph + cutoff", loop),
                          ("(a') batched radius graph alone", lambda: radius_graph_batch(loc, ptr_dev, r)),
                          ("(b') per-frame radius graph alone", lambda: [radius_graph(c, r) for c in clouds]),
                          ("(a) again", batched), ("(b) again", loop)]:
            med, lo, hi = timed(fn)
            out.append(f"  {label}: median {med:.3f} ms  (min {lo:.3f}, max {hi:.3f}) of 20 runs after 3 warm-ups")
    text = "\n".join(out)
    print(text)
    if len(sys.argv) > 1:
        with open(sys.argv[1], "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
