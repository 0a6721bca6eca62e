"""Measure the pair-table kernels of the instance evaluation (muscle_amd/ins_eval.py, csrc/ins_eval.hip) for one 375 x 500 image
(one GPU, one process), at n = 30 predictions / m = 5 objects (a 186-cell table: LDS tile) and n = 300 / m = 40 (12 341 cells:
global integer atomics):

  * device time per call of mx_label_pair_counts (from the seg_map) and mx_mask_pair_counts (from the bool [n,H,W] stack): HIP
    events around --calls back-to-back calls, divided by their number; one warm-up window, then the median [min..max] of
    --rounds windows.  The two memsets each entry enqueues are inside;
  * pair_table per image (wall clock, synchronised: the upload of G, the kernel, the one read-back), both forms; the mask form
    from a host stack also uploads n * H * W bytes;
  * the numpy way in the same run: n * m boolean ANDs and ORs over the image, one thread of this host;
  * the tables of both forms are compared with the numpy restatement before anything is timed.

    python tools/bench_ins_eval.py [--rounds 9] [--calls 200] [--out profiles/ins_eval_bench.txt]

Without a GPU the file says "not measured".  Synthetic inputs (tests/ins_eval_ref.py).  Nothing here fixes a time.
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

H, W = 375, 500
SIZES = ((30, 5), (300, 40))


def fmt(ts, unit="us"):
    ts = np.asarray(ts)
    return f"{np.median(ts):9.2f} [{ts.min():.2f}..{ts.max():.2f}] {unit}"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "ins_eval_bench.txt"))
    args = ap.parse_args()
    import torch
    lines = [f"instance evaluation, pair tables of one {H} x {W} image (tools/bench_ins_eval.py; synthetic rectangles)", ""]
    if not torch.cuda.is_available():
        lines += ["not measured: no GPU where this file was written.",
                  "run `python tools/bench_ins_eval.py` on an MI355X to fill this file in."]
        open(args.out, "w").write("\n".join(lines) + "\n")
        print("\n".join(lines))
        return 0
    import ins_eval_ref as R
    from muscle_amd import ins_eval
    from muscle_amd.ins_seg import InstanceLabels
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
            ts.append(1e6 * (time.perf_counter() - t0))
        return ts

    for n, m in SIZES:
        seg = R.blobs(H, W, n, 1)
        G = R.blobs(H, W, m, 2).astype(np.uint8)
        masks = seg[None] == np.arange(1, n + 1, dtype=np.int32)[:, None, None]
        seg_d, G_d, masks_d = (torch.from_numpy(x).to(dev) for x in (seg, G, masks))
        ins = InstanceLabels(seg_d, np.zeros(n, np.float32), np.zeros(n, np.int64), np.zeros(n, np.int32))
        cells = (n + 1) * (m + 1)
        out = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        ok_l = np.array_equal(ins_eval.pair_table(ins, G_d, m), R.label_table(seg, G, n, m)[0])
        ok_m = np.array_equal(ins_eval.pair_table(masks_d, G_d, m), R.mask_table(masks, G, m)[0])
        lines += [f"n = {n} predictions, m = {m} objects: table of {cells} cells ({'LDS tile' if cells <= 8192 else 'global atomics'}); "
                  f"label-map input {seg.nbytes + G.nbytes} bytes, mask input {masks.nbytes + G.nbytes} bytes; "
                  f"tables equal the restatement: {ok_l}, {ok_m}",
                  "  device time per call (HIP events around %d calls, memsets included):" % args.calls,
                  f"    mx_label_pair_counts            {fmt(device_us(lambda: ins_eval.label_pair_counts(seg_d, G_d, n, m, out[:-1], out[-1:])))}",
                  f"    mx_mask_pair_counts             {fmt(device_us(lambda: ins_eval.mask_pair_counts(masks_d, G_d, m, out[:-1], out[-1:])))}",
                  "  pair_table per image (wall clock; G on the device, one read-back):",
                  f"    InstanceLabels (label map)      {fmt(wall_us(lambda: ins_eval.pair_table(ins, G_d, m)))}",
                  f"    mask stack on the device        {fmt(wall_us(lambda: ins_eval.pair_table(masks_d, G_d, m)))}",
                  f"    mask stack on the host (upload) {fmt(wall_us(lambda: ins_eval.pair_table(masks, G_d, m)))}"]

        def numpy_way():
            g = [G == j + 1 for j in range(m)]
            iou = np.zeros((n, m))
            for p in range(n):
                for j in range(m):
                    iou[p, j] = (masks[p] & g[j]).sum() / max((masks[p] | g[j]).sum(), 1)
            return iou

        t0 = time.perf_counter()
        ref_iou = numpy_way()
        t1 = time.perf_counter()
        same = np.array_equal(ref_iou, ins_eval.mask_iou(ins_eval.pair_table(ins, G_d, m), False))
        lines += [f"  numpy, n * m = {n * m} boolean ANDs and ORs over the image (one thread of this host, once): {1e3 * (t1 - t0):.1f} ms; "
                  f"IoU matrix equal to mask_iou of the table: {same}", ""]
    open(args.out, "w").write("\n".join(lines) + "\n")
    print("\n".join(lines))
    return 0


if __name__ == "__main__":
    sys.exit(main())
