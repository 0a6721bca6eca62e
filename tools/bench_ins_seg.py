"""Measure the instance pseudo-label path (muscle_amd/ins_seg.py, csrc/irn_ins.hip) for one 375 x 500 image (one GPU, one process):

  * device time of every step between HIP events, median [min..max] over --rounds: centroids (300 iterations, 94 x 125: the
    field is staged in LDS), the weak map, mx_ccl at 94 x 125 and at 375 x 500, the id compression, the split, both walks, the
    finish (mx_irn_up_max + mx_irn_ins_finish), the segment statistics and the map;
  * the whole of instances_from_field per image (wall clock, synchronised: it reads I, n and the segment table back), dense and stencil walk;
  * K = 2 classes on the synthetic attractor / swirl field of tests/ins_seg_ref.py (I is what that field gives, about 5);
  * the numpy + scipy restatement of the same steps on the host (scipy.ndimage.label for the components), walk excluded.

    python tools/bench_ins_seg.py [--rounds 9] [--out profiles/ins_seg_bench.txt]

Without a GPU the file says "not measured" and lists what is open.  Synthetic inputs.  Nothing here fixes a time.
"""
from __future__ import annotations

import argparse
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

h, w, H, W = 94, 125, 375, 500
KEYS = (3, 11)
ITER = 300

OPEN = ["device time per kernel: mx_irn_centroids (300 iterations), mx_irn_weak, mx_ccl at 94 x 125 and 375 x 500, mx_id_mark / rank / apply,",
        "  mx_irn_ins_split, mx_irn_up_max + mx_irn_ins_finish at C = K * I, mx_seg_stats, mx_seg_map",
        "instances_from_field per 375 x 500 image with the dense and the stencil walk, K = 2, I about 5",
        "the share of the three small read-backs (I, n with the maximum, the [3,n] table), and of the single-workgroup prefix sum at 187 501 entries",
        "the host restatement (numpy + scipy.ndimage.label) of the same steps, for scale",
        "the centroid kernel staged in LDS against the same kernel reading through L2 (46 workgroups of one per CU either way)"]


def fmt(ts):
    ts = np.asarray(ts)
    return f"{np.median(ts):9.3f} [{ts.min():.3f}..{ts.max():.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ins_seg_bench.txt"))
    args = ap.parse_args()
    import torch
    lines = [f"instance pseudo-labels, one {H} x {W} image ({h} x {w} at the IRN's stride), K = {len(KEYS)}, {ITER} centroid iterations",
             "(tools/bench_ins_seg.py; synthetic attractor / swirl field)", ""]
    if not torch.cuda.is_available():
        lines += ["not measured: no GPU where this file was written.  Open:"] + ["  - " + s if not s.startswith("  ") else "  " + s for s in OPEN]
        lines += ["", "run `python tools/bench_ins_seg.py` on an MI355X to fill this file in."]
        open(args.out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return 0
    import ins_seg_ref as R
    from scipy import ndimage
    import muscle_amd
    from muscle_amd import indexing, ins_seg, ops, synth
    from muscle_amd._lib import call, ptr, stream
    dev = torch.device("cuda:0")
    dp_np = R.attractors(h, w, 0, swirl=True)
    dp = torch.from_numpy(dp_np).to(dev)
    edge = torch.from_numpy((0.9 * synth.uniform(7, "bench_ins_edge", (1, h, w)) ** 3).astype(np.float32)).to(dev)
    cam = synth.irn_cam_dict(H, W, 4, classes=KEYS)
    cams = torch.from_numpy(np.stack([cam[k] for k in KEYS])).to(dev)
    down = ops.resize_planar_halfpixel(cams, h, w)

    def timed(fn):
        fn()
        ts = []
        for _ in range(args.rounds):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            fn()
            b.record()
            torch.cuda.synchronize()
            ts.append(a.elapsed_time(b))
        return ts

    cent = muscle_amd.find_centroids(dp, ITER)
    cluster, I = muscle_amd.cluster_centroids(cent, dp)
    x = ins_seg.split_instances(down, cluster, I)
    weak = torch.empty(h, w, dtype=torch.int32, device=dev)
    call("mx_irn_weak", ptr(dp), h, w, 2.5, ptr(weak), stream())
    root = muscle_amd.connected_components(weak)
    meta = torch.zeros(3, dtype=torch.int32, device=dev)
    lines.append(f"I = {I} clusters, C = {len(KEYS) * I} channels")
    rows = [("mx_irn_centroids (LDS-staged field)", lambda: muscle_amd.find_centroids(dp, ITER)),
            ("mx_irn_weak", lambda: call("mx_irn_weak", ptr(dp), h, w, 2.5, ptr(weak), stream())),
            (f"mx_ccl {h} x {w} (+ 2 allocations)", lambda: muscle_amd.connected_components(weak)),
            ("mx_id_mark + mx_id_rank", lambda: ins_seg._compress(root, cent, meta)),
            ("mx_irn_ins_split", lambda: ins_seg.split_instances(down, cluster, I))]
    res = {}
    for method in indexing.WALK_METHODS:
        rw = indexing.propagate_to_edge(x, edge, beta=8, exp_times=6, radius=5, method=method)
        res[method] = rw
        rows.append((f"propagate_to_edge {method}", lambda m=method: indexing.propagate_to_edge(x, edge, beta=8, exp_times=6, radius=5, method=m)))
    rw = res["dense"]
    label, win, scratch = ins_seg.finish_instances(rw, H, W, 0.25)
    root6 = muscle_amd.connected_components(label)
    rows += [("mx_irn_up_max + mx_irn_ins_finish", lambda: ins_seg.finish_instances(rw, H, W, 0.25)),
             (f"mx_ccl {H} x {W} (+ 2 allocations)", lambda: muscle_amd.connected_components(label)),
             (f"mx_id_mark + mx_id_rank, {H * W + 1} entries", lambda: ins_seg._compress(root6, None, meta))]
    lines += ["", "device time per step (HIP events around the Python call):"]
    for name, fn in rows:
        lines.append(f"  {name:48s} {fmt(timed(fn))}")
    lines += ["", "per image, wall clock with synchronisation (three small read-backs inside: I, n with the maximum, the [3,n] table):"]
    for method in indexing.WALK_METHODS:
        def whole(m=method):
            return ins_seg.instances_from_field(edge, dp, cam, H, W, iterations=ITER, method=m)
        ins = whole()
        ts = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            whole()
            torch.cuda.synchronize()
            ts.append(1e3 * (time.perf_counter() - t0))
        lines.append(f"  instances_from_field, {method:8s} {fmt(ts)}   n = {len(ins)} segments, areas {ins.area.tolist()}")
    lines.append(f"  label_segments alone (step 6)  {fmt(timed(lambda: ins_seg.label_segments(label, win, KEYS, I, scratch)))}")
    # the host restatement, walk excluded
    t0 = time.perf_counter()
    c_ref = R.find_centroids(dp_np, ITER)
    t1 = time.perf_counter()
    ndimage.label(R.weak_map(dp_np))
    cl_ref, I_ref = R.cluster_centroids(c_ref, dp_np)
    t2 = time.perf_counter()
    lab_ref, win_ref, _, _ = R.finish(rw.reshape(-1, h, w).cpu().numpy(), H, W, 0.25)
    t3 = time.perf_counter()
    ndimage.label(lab_ref > 0)
    R.segments(lab_ref, win_ref, KEYS, I_ref)
    t4 = time.perf_counter()
    lines += ["", "host restatement (numpy + scipy.ndimage.label, one thread of this host; walk excluded):",
              f"  centroids {1e3 * (t1 - t0):.1f} ms, clusters {1e3 * (t2 - t1):.1f} ms, finish with the [C,H,W] array {1e3 * (t3 - t2):.1f} ms, "
              f"segments {1e3 * (t4 - t3):.1f} ms",
              f"  centroids equal: {np.array_equal(c_ref, cent.cpu().numpy())}; clusters equal: {np.array_equal(cl_ref, cluster.cpu().numpy())}"]
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
