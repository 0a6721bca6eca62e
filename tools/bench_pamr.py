"""Pixel-adaptive mask refinement (muscle_amd.pamr): cost per 375 x 500 image, timed with device events.
  time    the affinity, one step and the whole call (10 iterations, the default dilations) at C = 2 and C = 21, ms; beside it,
          alternating in the same process, the same computation in torch ops on the GPU (replicate F.pad, shifted slices, std,
          softmax: what a user would write without the kernels); the achieved bytes/s of a step against its algorithmic traffic
          (w read once, the mask read once and written once); and the 22.5 ms of infer_seg --crf 2 (profiles/crf_bench.txt) for scale
  ratios  max|gpu - fp64| over e32 = max|float32 numpy - fp64| for w and for the output on the shapes of tests/test_gpu_pamr.py, with
          the restatement of tests/pamr_ref.py
  trace   a few whole calls and nothing else: the program of a `rocprofv3 --kernel-trace --stats` run of its own
Writes what it prints to --out as well.  Not the contract bench."""
import argparse
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch
import torch.nn.functional as F

from muscle_amd import PAMR, pamr_affinity, pamr_apply

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["all", "time", "ratios", "trace"])
ap.add_argument("--reps", type=int, default=50)
ap.add_argument("--rounds", type=int, default=3, help="alternation rounds")
ap.add_argument("--height", type=int, default=375)
ap.add_argument("--width", type=int, default=500)
ap.add_argument("--iters", type=int, default=10)
ap.add_argument("--out", default=None, help="also write the lines to this file")
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_pamr needs the GPU"
dev = torch.device("cuda:0")
H, W, DIL = a.height, a.width, (1, 2, 4, 8, 12, 24)
P = 8 * len(DIL)
CRF2_MS = 22.5                                              # infer_seg --crf 2 per image, profiles/crf_bench.txt
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def photo(seed):
    """A blocky noisy image."""
    g = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    img[:, :W // 3] = [200, 30, 30]
    img[H // 4:3 * H // 4, W // 3:4 * W // 5] = [20, 180, 60]
    img[:, 4 * W // 5:] = [30, 40, 200]
    return np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def taps(x, centre):
    r = max(DIL)
    xp = F.pad(x, (r, r, r, r), mode="replicate")
    return [xp[..., r + d * dy:r + d * dy + H, r + d * dx:r + d * dx + W]
            for d in DIL for dy in (-1, 0, 1) for dx in (-1, 0, 1) if centre or (dy, dx) != (0, 0)]


def torch_affinity(I):
    std = torch.stack(taps(I, True), dim=0).std(dim=0, unbiased=True)
    aff = torch.stack([-(I - t).abs() / (1e-8 + 0.1 * std) for t in taps(I, False)], dim=0).mean(dim=2)
    return torch.softmax(aff, dim=0)                         # [P,1,H,W]


def torch_step(w, m):
    return sum(w[p][:, None] * t for p, t in enumerate(taps(m, False)))


def fmt(ts):
    return " / ".join(f"{t:.4f}" for t in ts)


img = photo(3)
img_d = torch.from_numpy(img).to(dev)
planar = img_d.permute(2, 0, 1).float().contiguous()[None]
say(f"PAMR, {H}x{W}, dilations {DIL} (P = {P}), {a.iters} iterations; {a.reps} calls per figure, {a.rounds} rounds, alternating")

if a.part == "trace":
    m = torch.rand(21, H, W, device=dev)
    pamr = PAMR(a.iters, DIL)
    for _ in range(3):
        pamr(img_d, m)
    torch.cuda.synchronize()
    say("trace: 3 whole calls at C = 21")

if a.part in ("all", "time"):
    w = pamr_affinity(img_d, DIL)
    with torch.no_grad():
        tw = torch_affinity(planar)
    say(f"w against the torch-op formulation (fp32): max-abs difference {float((tw[:, 0] - w).abs().max()):.3e}")
    for C in (2, 21):
        m = torch.rand(C, H, W, device=dev)
        pamr = PAMR(a.iters, DIL)
        one = lambda: pamr_apply(w, m, 1, DIL)  # noqa: E731
        with torch.no_grad():
            for _ in range(2):
                pamr(img_d, m), pamr_affinity(img_d, DIL), one(), torch_affinity(planar), torch_step(tw, m[None])
            d_step = float((torch_step(tw, m[None])[0] - one()).abs().max())
            t = {k: [] for k in ("aff", "step", "call", "taff", "tstep")}
            for _ in range(a.rounds):
                t["aff"].append(events(lambda: pamr_affinity(img_d, DIL), a.reps))
                t["taff"].append(events(lambda: torch_affinity(planar), max(1, a.reps // 10)))
                t["step"].append(events(one, a.reps))
                t["tstep"].append(events(lambda: torch_step(tw, m[None]), max(1, a.reps // 10)))
                t["call"].append(events(lambda: pamr(img_d, m), a.reps))
        traffic = (P + 2 * C) * H * W * 4
        best = min(t["step"])
        say(f"C = {C}: affinity {fmt(t['aff'])} ms (torch ops {fmt(t['taff'])} ms); one step {fmt(t['step'])} ms (torch ops "
            f"{fmt(t['tstep'])} ms, max-abs difference of the results {d_step:.3e}); the whole call, affinity + {a.iters} steps, "
            f"{fmt(t['call'])} ms (torch ops, best affinity + {a.iters} x best step: {min(t['taff']) + a.iters * min(t['tstep']):.3f} ms)")
        say(f"C = {C}: a step's algorithmic traffic is {traffic / 1e6:.2f} MB (w {P * H * W * 4 / 1e6:.2f} MB read, the mask "
            f"{C * H * W * 4 / 1e6:.2f} MB read and written); best step {best * 1e3:.1f} us = {traffic / best / 1e6:.0f} GB/s achieved; "
            f"the {P} gathers per channel ask the caches for {P * C * H * W * 4 / 1e6:.1f} MB")
        say(f"C = {C}: the whole call is {min(t['call']):.3f} ms per image; infer_seg --crf 2 is {CRF2_MS} ms per image "
            f"(profiles/crf_bench.txt), {CRF2_MS / min(t['call']):.0f}x that")

if a.part in ("all", "ratios"):
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import test_gpu_pamr as TG
    say("max|gpu - fp64| / e32, e32 = max|float32 numpy - fp64| on the same input (tests/test_gpu_pamr.py asks for <= 4 e32 + 1e-7):")
    for name in sorted(TG.CASES):
        im, mask, dil, w64, out64, e32w, e32o = TG._case(name)
        wg = pamr_affinity(torch.from_numpy(im).to(dev), dil).cpu().numpy().astype(np.float64)
        og = PAMR(10, dil)(torch.from_numpy(im).to(dev), torch.from_numpy(mask).to(dev)).cpu().numpy().astype(np.float64)
        ew, eo = float(np.abs(wg - w64).max()), float(np.abs(og - out64).max())
        say(f"  {name:14s} {tuple(mask.shape)} D={len(dil)}: w {ew:.2e} / {e32w:.2e} = {ew / e32w if e32w else float('nan'):.2f}; "
            f"out after 10 iterations {eo:.2e} / {e32o:.2e} = {eo / e32o if e32o else float('nan'):.2f}")

if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
