"""Measure the boundary evaluation (muscle_amd/evaluation.py `BoundaryEval`, csrc/boundary_eval.hip) for one 375 x 500 pair with
K = 21 classes and dmax = 16 (one GPU, one process):

  * device time of the three mx_label_edge_dist launches of one image (gt without / with the image edge, pred with it), of the
    mx_boundary_counts launch, and of the whole `BoundaryEval.add`: HIP events around --calls back-to-back calls, divided by their
    number; one warm-up window, then the median [min..max] of --rounds windows;
  * `BoundaryEval.add` per image on the wall clock, synchronised;
  * the host way in the same run: tests/boundary_ref.py's scipy restatement (per-class erosions for the three maps, then the
    masks of the six rows), one thread of this host, once;
  * what `--val_boundary 1` adds to a validation sweep: `validate_seg` of a B7 decoder over --images synthetic 375 x 500 images,
    without and with the evaluator, alternated --sweeps times in this process (skipped with --images 0);
  * the tables are compared with the restatement before anything is timed.

    python tools/bench_boundary_eval.py [--rounds 9] [--calls 200] [--images 24] [--sweeps 3] [--out profiles/boundary_eval_bench.txt]

Without a GPU the file says "not measured".  Synthetic inputs (tests/boundary_ref.py).  Nothing here fixes a time.
"""
from __future__ import annotations

import argparse
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

H, W, K, DMAX = 375, 500, 21, 16


def fmt(ts, unit="us"):
    ts = np.asarray(ts)
    return f"{np.median(ts):9.2f} [{ts.min():.2f}..{ts.max():.2f}] {unit}"


def _tree(root, n):
    """n synthetic 375 x 500 images and label maps in the layout of a VOC tree."""
    import PIL.Image
    import boundary_ref as R
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClass"))
    rng = np.random.default_rng(3)
    yy, xx = np.mgrid[0:H, 0:W].astype(np.float64)
    names = [f"img{i:03d}" for i in range(n)]
    for i, nm in enumerate(names):
        img = np.stack([127 + 100 * np.sin(xx / (14.0 + c) + i) * np.cos(yy / (16.0 - c)) for c in range(3)], -1) + rng.normal(0, 12, (H, W, 3))
        PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(os.path.join(root, "JPEGImages", nm + ".jpg"), quality=92)
        PIL.Image.fromarray(R.blobs(H, W, 12, K, seed=100 + i, void_rows=(7,))).save(os.path.join(root, "SegmentationClass", nm + ".png"))
    return names


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--images", type=int, default=24)
    ap.add_argument("--sweeps", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "boundary_eval_bench.txt"))
    args = ap.parse_args()
    import torch
    lines = [f"boundary evaluation of one {H} x {W} pair, K = {K}, dmax = {DMAX} (tools/bench_boundary_eval.py; synthetic label maps)", ""]
    if not torch.cuda.is_available():
        lines += ["not measured: no GPU where this file was written.",
                  "run `python tools/bench_boundary_eval.py` on an MI355X to fill this file in."]
        open(args.out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return 0
    import boundary_ref as R
    from muscle_amd import ops
    from muscle_amd._lib import call, ptr, stream
    from muscle_amd.evaluation import BoundaryEval, boundary_radius, validate_seg
    dev = torch.device("cuda:0")

    def device_us(fn):
        ts = []
        for r in range(args.rounds + 1):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            for _ in range(args.calls):
                fn()
            b.record()
            torch.cuda.synchronize()
            if r:                                                             # the first window is the warm-up
                ts.append(1e3 * a.elapsed_time(b) / args.calls)
        return ts

    def wall_us(fn):
        fn()
        ts = []
        for _ in range(args.rounds):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            fn()
            torch.cuda.synchronize()
            ts.append(1e6 * (time.perf_counter() - t0))
        return ts

    gt = R.blobs(H, W, 12, K, seed=1, void_rows=(7, 200))
    pred = np.roll(np.roll(gt, 3, axis=0), 5, axis=1)
    pred[pred == 255] = 0
    g, p = torch.from_numpy(gt).to(dev), torch.from_numpy(pred).to(dev)
    d = torch.empty(3, H, W, dtype=torch.uint8, device=dev)
    ev = BoundaryEval(dev, K, DMAX)
    d_img = boundary_radius(H, W, ev.ratio, DMAX)

    def maps():
        ops.label_edge_dist(g, DMAX, 0, out=d[0])
        ops.label_edge_dist(g, DMAX, 1, out=d[1])
        ops.label_edge_dist(p, DMAX, 1, out=d[2])

    def counts():
        call("mx_boundary_counts", ptr(p), ptr(g), ptr(d[0]), ptr(d[1]), ptr(d[2]), K, H, W, DMAX, d_img, ptr(ev.hist), ptr(ev.ratio_counts),
             stream())

    t0 = time.perf_counter()
    rh, rr = R.tables_erosion(pred, gt, K, DMAX)
    t_host = time.perf_counter() - t0
    ev.add(p, g)
    hist, rat = ev.tables()
    band = int(R.within(rh, d_img)[3].sum())
    lines += [f"tables equal the scipy restatement: {np.array_equal(hist, rh)}, {np.array_equal(rat, rr)}; per-image radius {d_img}; "
              f"{band} of {int((gt != 255).sum())} counted pixels lie in the ground-truth band of that radius",
              "device time per image (HIP events around %d calls):" % args.calls,
              f"  3 x mx_label_edge_dist            {fmt(device_us(maps))}",
              f"  mx_boundary_counts                {fmt(device_us(counts))}",
              f"  BoundaryEval.add (4 launches)     {fmt(device_us(lambda: ev.add(p, g)))}",
              f"BoundaryEval.add per image, wall clock, synchronised: {fmt(wall_us(lambda: ev.add(p, g)))}",
              f"host: tests/boundary_ref.py tables_erosion (scipy binary_erosion per class and radius, then the six rows; one thread, once): "
              f"{1e3 * t_host:.1f} ms", ""]
    if args.images > 0:
        import muscle_amd
        torch.manual_seed(1)
        model = muscle_amd.MuSCLe(21, "efficientnet-b7", layers=3, last_pooling=True, mode="dec").to(dev).eval()
        with tempfile.TemporaryDirectory() as root:
            names = _tree(root, args.images)
            validate_seg(model, names[:2], root, dev, K)                         # warm-up
            off, on = [], []
            for _ in range(args.sweeps):
                for ts, bev in ((off, None), (on, BoundaryEval(dev, K, DMAX))):
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    validate_seg(model, names, root, dev, K, boundary=bev)
                    if bev is not None:
                        bev.tables()
                    torch.cuda.synchronize()
                    ts.append(1e3 * (time.perf_counter() - t0) / args.images)
        lines += [f"validate_seg, B7 decoder with random weights, {args.images} synthetic images, batch 1, alternated {args.sweeps} times (wall clock per image):",
                  f"  without the evaluator             {fmt(off, 'ms')}",
                  f"  with boundary=BoundaryEval        {fmt(on, 'ms')}",
                  f"  difference of the medians         {1e3 * (np.median(on) - np.median(off)):9.1f} us per image "
                  f"({100 * (np.median(on) / np.median(off) - 1):+.2f} %)", ""]
    else:
        lines += ["validate_seg with / without the evaluator: not measured (--images 0)", ""]
    lines += ["not measured here: the kernels alone under a profiler, other image sizes and radii, a sweep over the real validation list."]
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
