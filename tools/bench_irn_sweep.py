"""Measure the infer_irn grid sweep (muscle_amd/irn_sweep.py) against the same grid done with the existing calls, one 375 x 500
synthetic image on the device, no file I/O, one GPU, one process.

  * the default grid: betas 6 8 10 12, exp_times 4..8, 20 thresholds 0.15..0.53 = 400 grid points;
  * one EdgeDisplacement forward; its edge map feeds both sides;
  * sweep: IrnSweep.add_field (upload of the kept CAMs, resize, per beta the weights, one walk with snapshots, the maxima, one
    counting launch);
  * loop: per grid point what infer_irn(..., method="stencil") does after its forward (cam_stack upload, resize,
    propagate_to_edge, finish_semseg) plus SegEval.add; and the same loop with the upload and resize hoisted out of it, the
    tighter yardstick;
  * the three tables are compared first, integer for integer; then the sides alternate round by round, hipEvent times that end in
    a synchronise, median [min..max].

    python tools/bench_irn_sweep.py [--rounds 9] [--out profiles/irn_sweep_bench.txt]

Without a GPU the file says so and holds no figure.  Synthetic inputs.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

HI, WI = 375, 500


def fmt(ts):
    ts = np.asarray(ts)
    return f"{np.median(ts):10.3f} [{ts.min():.3f}..{ts.max():.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irn_sweep_bench.txt"))
    args = ap.parse_args()
    if args.rounds < 5:
        ap.error("--rounds must be at least 5")
    import torch
    lines = ["tools/bench_irn_sweep.py - the (beta, exp_times, threshold) grid of infer_irn scored by muscle_amd.irn_sweep against a loop of the existing calls", ""]
    ok = True
    if not torch.cuda.is_available():
        lines += ["STATUS: NOT MEASURED.  No GPU was available where this file was written: it holds no figure.  Run", "",
                  "    python tools/bench_irn_sweep.py", "", "on an MI355X; that rewrites this file."]
    else:
        measured, ok = measure(torch, args.rounds)
        lines += measured
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if ok else 1


def measure(torch, rounds):
    import muscle_amd
    from muscle_amd import indexing, ops, synth
    from muscle_amd.evaluation import SegEval
    from muscle_amd.irn import cam_stack
    from muscle_amd.irn_sweep import DEFAULT_BETAS, DEFAULT_EXP_TIMES, DEFAULT_THRESHOLDS, IrnSweep
    dev = torch.device("cuda:0")
    betas, ets, thr = DEFAULT_BETAS, DEFAULT_EXP_TIMES, DEFAULT_THRESHOLDS

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    sd = synth.irn_state_dict(1)
    m = muscle_amd.EdgeDisplacement()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    img = torch.from_numpy(synth.irn_image_pair(HI, WI, 1)).to(dev)
    cam = synth.irn_cam_dict(HI, WI, 1)
    yy, xx = np.mgrid[0:HI, 0:WI]
    gt_h = ((yy // 40 * 13 + xx // 40) % 21).astype(np.uint8)
    gt_h[synth.uniform(1, "sweep_ignore", (HI, WI)) < 0.05] = 255
    gt = torch.from_numpy(gt_h).to(dev)
    edge, _ = m(img)
    edge = edge.detach()
    h, w = edge.shape[-2:]

    def sweep():
        sw = IrnSweep(dev, betas, ets, thr)
        sw.add_field(edge, cam, gt, HI, WI)
        return sw.table

    def loop(hoisted):
        out = torch.zeros(len(betas), len(ets), len(thr), 21, 3, dtype=torch.int64, device=dev)
        down = ops.resize_planar_halfpixel(cam_stack(cam, HI, WI, dev), h, w) if hoisted else None
        for bi, b in enumerate(betas):
            for ei, et in enumerate(ets):
                for ti, t in enumerate(thr):
                    d = down if hoisted else ops.resize_planar_halfpixel(cam_stack(cam, HI, WI, dev), h, w)
                    rw = indexing.propagate_to_edge(d, edge, beta=b, exp_times=et, radius=5, method="stencil")
                    e = SegEval(dev, 21)
                    e.add(indexing.finish_semseg(rw, HI, WI, t), gt)
                    out[bi, ei, ti] = e.counts
        return out

    a, b, c = sweep(), loop(False), loop(True)                       # warm-up and the comparison
    same = bool(torch.equal(a, b)) and bool(torch.equal(a, c))
    fg = int(a[..., 1:, 1].sum())
    ts = {"sweep": [], "loop": [], "hoisted": []}
    for _ in range(rounds):
        ts["sweep"].append(ev(sweep)[0])
        ts["loop"].append(ev(lambda: loop(False))[0])
        ts["hoisted"].append(ev(lambda: loop(True))[0])
    tf = [ev(lambda: m(img))[0] for _ in range(rounds + 1)][1:]
    npts = len(betas) * len(ets) * len(thr)
    med = {k: float(np.median(v)) for k, v in ts.items()}
    out = [f"MEASURED on {torch.cuda.get_device_name(0)}, one process, {rounds} rounds, the three sides alternated round by round, hipEvent times,",
           f"median [min..max]; one {HI} x {WI} image ({h} x {w} at 1/4 resolution), {len(cam)} classes in the CAM dict, radius 5;",
           f"grid betas {list(betas)} x exp_times {list(ets)} x {len(thr)} thresholds {thr[0]}..{thr[-1]} = {npts} grid points.", "",
           f"tables (int64 [{len(betas)},{len(ets)},{len(thr)},21,3]) of the three sides equal, integer for integer: {'yes' if same else 'NO'}"
           f"   (foreground predictions summed over the grid: {fg})", "",
           f"  sweep   IrnSweep.add_field, whole grid                                   {fmt(ts['sweep'])}",
           f"  loop    per grid point: cam_stack + resize + walk + finish + SegEval.add  {fmt(ts['loop'])}   ({med['loop'] / npts:.3f} ms per grid point)",
           f"  loop with the CAM upload and resize hoisted out                          {fmt(ts['hoisted'])}   ({med['hoisted'] / npts:.3f} ms per grid point)",
           f"  one EdgeDisplacement forward (both sides need one per image)             {fmt(tf)}", "",
           f"loop minimum / sweep median: {min(ts['loop']) / med['sweep']:.1f}x; hoisted loop minimum / sweep median: {min(ts['hoisted']) / med['sweep']:.1f}x",
           f"per image with the forward: sweep {med['sweep'] + float(np.median(tf)):.2f} ms against {med['loop'] + float(np.median(tf)):.2f} ms for the loop",
           "(the scripts add file I/O on top of the loop: one PNG write and one PNG read per image and grid point; none is timed here)."]
    return out, same


if __name__ == "__main__":
    sys.exit(main())
