"""Measure the IRN network on the HIP path (one GPU, one process):

  * every 3x3 convolution shape of the network at batch 2 / 512 x 512: microseconds, TFLOP/s against the 157.3 TFLOP/s fp32-MFMA
    peak and against the shape's HBM bound (input + output + packed weight once, at 8 TB/s);
  * the whole EdgeDisplacement forward for one 375 x 500 pair;
  * the same network as torch ops on the same device (tests/irn_net_ref.py moved to the GPU: MIOpen, what a user would
    otherwise run);
  * infer_irn per image at the script's defaults, with the network's share and propagate_to_edge's time.

    python tools/bench_irn_net.py [--reps 20] [--no-walk]

Warm-up first, hipEvent timing, `reps` repetitions, median and min-max spread reported.  Synthetic weights and inputs.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PEAK_TFLOPS, HBM_TBS = 157.3, 8.0
SHAPES = [(128, 64, 1), (128, 128, 2), (64, 128, 1), (64, 256, 2), (32, 256, 1), (32, 512, 1)]      # H = W, Cin = Cout, stride


def timed(fn, reps, warmup=3):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b) * 1e3)
    ts = np.array(ts)
    return float(np.median(ts)), float(ts.min()), float(ts.max())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--no-walk", action="store_true")
    args = ap.parse_args()
    import muscle_amd
    from muscle_amd import indexing, ops, synth
    from muscle_amd.irn import infer_irn
    import irn_net_ref as R
    dev = torch.device("cuda:0")
    print(f"# GEMM mode {muscle_amd.get_gemm_mode()} (1x1 convolutions; the 3x3 kernel is exact fp32 always), reps {args.reps}")
    print("# 3x3 convolution, batch 2:  H  C stride |  us (median, min-max) | TFLOP/s  % of 157.3 | HBM bound us  x bound")
    for H, C, s in SHAPES:
        x = torch.randn(2, H, H, C, device=dev)
        wp = ops.conv3x3_pack(torch.randn(C, C, 3, 3, device=dev) * 0.02)
        b = torch.zeros(C, device=dev)
        med, lo, hi = timed(lambda: ops.conv3x3(x, wp, bias=b, stride=s, relu=True), args.reps)
        Ho = (H - 1) // s + 1
        flop = 2.0 * 2 * Ho * Ho * C * C * 9
        byts = 4.0 * (x.numel() + 2 * Ho * Ho * C + wp.numel())
        bound = byts / (HBM_TBS * 1e12) * 1e6
        tf = flop / med / 1e6
        print(f"conv3x3 {H:4d} {C:4d} {s} | {med:8.1f} ({lo:.1f}-{hi:.1f}) | {tf:6.1f} {100 * tf / PEAK_TFLOPS:5.1f}% | {bound:6.2f} {med / bound:6.1f}x")

    Hi, Wi = 375, 500
    sd = synth.irn_state_dict(1)
    m = muscle_amd.EdgeDisplacement()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    x = torch.from_numpy(synth.irn_image_pair(Hi, Wi, 1)).to(dev)
    net = timed(lambda: m(x), args.reps)
    print(f"EdgeDisplacement forward, one {Hi}x{Wi} pair (HIP): {net[0] / 1e3:.2f} ms ({net[1] / 1e3:.2f}-{net[2] / 1e3:.2f})")
    sdt = R.to_dtype(sd, torch.float32, dev)
    with torch.no_grad():
        tr = timed(lambda: R.edge_displacement(sdt, x, 512), args.reps)
    print(f"the same network as torch ops on the device (MIOpen): {tr[0] / 1e3:.2f} ms ({tr[1] / 1e3:.2f}-{tr[2] / 1e3:.2f})"
          f"  -> HIP path {tr[0] / net[0]:.2f}x")
    if not args.no_walk:
        cam = synth.irn_cam_dict(Hi, Wi, 1)
        edge, _ = m(x)
        cams = torch.rand(20, edge.shape[1], edge.shape[2], device=dev)
        reps = max(2, args.reps // 10)
        walk = timed(lambda: indexing.propagate_to_edge(cams, edge, beta=8, exp_times=6, radius=5), reps, warmup=1)
        full = timed(lambda: infer_irn(m, x, cam), reps, warmup=1)
        print(f"propagate_to_edge, {edge.shape[1]}x{edge.shape[2]}, beta 8, exp_times 6: {walk[0] / 1e3:.1f} ms ({walk[1] / 1e3:.1f}-{walk[2] / 1e3:.1f})")
        print(f"infer_irn per image: {full[0] / 1e3:.1f} ms ({full[1] / 1e3:.1f}-{full[2] / 1e3:.1f}); network share {100 * net[0] / full[0]:.2f}%;"
              f" network / propagate_to_edge = {100 * net[0] / walk[0]:.2f}% (required <= 5%)")
        assert net[0] <= 0.05 * walk[0], "the network forward exceeds 5 % of propagate_to_edge"


if __name__ == "__main__":
    main()
