"""Dense-CRF energy loss (muscle_amd.crf_loss): cost at the decoder-training shape, N = 16, K = 21, 448 x 448, the defaults (sxy 80,
srgb 15, scale 4, trunc 2: 112 x 112 cells, kernel width 20 cells, R = 40), timed with device events.
  alone   forward (staging + message pass + reduction) and backward of the loss by themselves, ms per call, next to the bound
          of the f32 matrix pipe for the message pass: the tiles walk whole 32 x 8 source tiles, every pair of a walked tile is
          one row of a 32x32x2 MFMA (64 FLOP) at 157.3 TFLOP/s;
  step    muscle_step on EfficientNet-B7 (train_muscle.py's loop body, synthetic soft labels, lamb 0.05) with the term off and on,
          alternated off / on / off / on in one process, ms per step.  The "off" rows are the step as it was before the term.
Writes what it prints to --out as well.  Not the contract bench."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import muscle_amd
from muscle_amd import crf_loss, synth

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["all", "alone", "step"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--steps", type=int, default=20, help="timed muscle_steps per arm and round")
ap.add_argument("--rounds", type=int, default=3, help="off/on rounds")
ap.add_argument("--model", default="efficientnet-b7")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=448)
ap.add_argument("--out", default=None, help="also write the lines to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
N, K, S = a.batch, 21, a.size
F32_MATRIX_PEAK = 157.3e12
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, reps):
    """ms per call between two device events around `reps` calls, after two warm-up calls."""
    for _ in range(2):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def walked_pairs(h, w, R):
    """Pairs the message pass evaluates for one image: per 16 x 8 output tile the 32 x 8 source tiles its window touches."""
    total = 0
    for Y0 in range(0, h, 8):
        ny = -(-(min(h - 1, Y0 + 7 + R) - max(0, Y0 - R) + 1) // 8)
        for X0 in range(0, w, 16):
            nx = -(-(min(w - 1, X0 + 15 + R) - max(0, X0 - R) + 1) // 32)
            total += ny * nx * 256 * 128
    return total


crit = muscle_amd.DenseEnergyLoss()
label = synth.synth_labels(N, 7)
img = torch.from_numpy(synth.normal(7, "img", (N, 3, S, S)).astype(np.float32)).to(dev)
say(f"dense-CRF energy loss, N={N} K={K} {S}x{S}, sxy {crit.sxy:g} srgb {crit.srgb:g} scale {crit.scale} trunc {crit.trunc:g}")

if a.part in ("all", "alone"):
    seg = torch.randn(N, K, S, S, device=dev, generator=torch.Generator(dev).manual_seed(8)) * 3
    window = torch.tensor([[0, 0, S, S - 16 * (i % 3)] for i in range(N)], dtype=torch.int32, device=dev)
    cfg = dict(sxy=crit.sxy, srgb=crit.srgb, scale=crit.scale, trunc=crit.trunc)
    loss, sums, M = crf_loss.energy_forward(seg, img, window, **cfg)
    g = torch.ones(1, device=dev)
    fwd = events(lambda: crf_loss.energy_forward(seg, img, window, **cfg), a.reps)
    bwd = events(lambda: crf_loss.energy_backward(seg, window, M, sums, g, crit.scale), a.reps)
    h = w = S // crit.scale
    R = int(np.ceil(crit.trunc * crit.sxy / crit.scale))
    pairs = N * walked_pairs(h, w, R)
    bound = pairs * 64 / F32_MATRIX_PEAK * 1e3
    say(f"alone: forward {fwd:.3f} ms, backward {bwd:.3f} ms per call (loss {float(loss):.6f}); message pass walks "
        f"{pairs / 1e9:.2f}e9 pairs, f32 MFMA bound {bound:.3f} ms; seg is {seg.numel() * 4 / 1e6:.0f} MB, read once by each")

if a.part in ("all", "step"):
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, a.model, layers=3, last_pooling=True, mode="dec").to(dev)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-5, weight_decay=5e-5)
    batch = {"img": img, "label": torch.from_numpy(label).to(dev), "mask": torch.from_numpy(synth.synth_soft_mask(label, S, 7)).to(dev)}
    arms = {"off": dict(), "on": dict(energy=crit, energy_weight=1.0)}
    out = {}
    for name, kw in arms.items():                              # warm-up of both arms
        for _ in range(2):
            out[name] = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128, **kw)
    ms = {"off": [], "on": []}
    for _ in range(a.rounds):                                  # off / on / off / on: drift of the box shows as a spread inside an arm
        for name, kw in arms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            torch.cuda.synchronize()
            e0.record()
            for _ in range(a.steps):
                out[name] = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128, **kw)
            e1.record()
            torch.cuda.synchronize()
            ms[name].append(e0.elapsed_time(e1) / a.steps)
    for name in arms:
        say(f"muscle_step {a.model} dec {S}x{S} bs{N} lamb 0.05, energy {name}: " + " / ".join(f"{t:.2f}" for t in ms[name]) +
            f" ms per step ({a.steps} steps each), loss_seg {float(out[name]['loss_seg'].detach()):.4f}" +
            (f" loss_energy {float(out[name]['loss_energy'].detach()):.4f}" if "loss_energy" in out[name] else ""))
    off, on = min(ms["off"]), min(ms["on"])
    say(f"best of each arm: off {off:.2f} ms, on {on:.2f} ms: the term costs {on - off:+.2f} ms per step ({(on / off - 1) * 100:+.2f} %)")

if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
