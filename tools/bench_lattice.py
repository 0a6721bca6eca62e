"""The lattice label CRF of IR-label generation (mx_ir_label_lattice, csrc/lattice.hip) against the windowed one (mx_ir_label) on a
synthetic 500 x 375 image with C smooth CAMs (L = C + 1 labels), sxy 3 / 50, srgb 5, weights 3 / 10.  One C per invocation
(--classes 2 or 6: one bounded step each; run it under a time limit).  Timed with device events, alternated in one process on one
GPU, --rounds rounds of --reps calls after a warm-up, medians:
  build      mx_lattice_build of the spatial (D = 2) and of the bilateral (D = 5) lattice, and their vertex counts
  lattice    mx_ir_label_lattice at t = 10 and at t = 1; per iteration = (t10 - t1) / 9, once per image = t1 - per iteration
  window     mx_ir_label, fused, trunc 4 (R = 12 / 200), t = 10
and the share of pixels on which the two backends' maps differ (they are different models).  Not the contract bench."""
import argparse
import json
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tests"))
import numpy as np
import torch

import ir_label_ref as IR
from muscle_amd import crf
from muscle_amd._lib import call, lib, ptr, stream
from muscle_amd.ir_label import ir_label_run

ap = argparse.ArgumentParser()
ap.add_argument("--classes", type=int, default=2)
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None, help="append the results as one JSON line to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
H, W, N_TRAIN_AUG = 375, 500, 10582
SG, WG, SB, SRGB, WB = crf.LABEL_MODEL
C = a.classes


def timed(fn, reps):
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


img, cams, keys = IR.synthetic(100 + C, H, W, C)
img_d, cams_d = torch.from_numpy(img).to(dev), torch.from_numpy(cams).to(dev)
ws2 = torch.empty(lib().mx_lattice_ws(2, H, W, 1) // 4, device=dev)
ws5 = torch.empty(lib().mx_lattice_ws(5, H, W, 1) // 4, device=dev)
out = {}


def build2():
    call("mx_lattice_build", ptr(img_d), H, W, SG, 0.0, ptr(ws2), stream())


def build5():
    call("mx_lattice_build", ptr(img_d), H, W, SB, SRGB, ptr(ws5), stream())


def lattice10():
    out["lattice"] = ir_label_run(img_d, cams_d, keys.tolist(), pairwise="lattice", want_pred=True)


def lattice1():
    ir_label_run(img_d, cams_d, keys.tolist(), pairwise="lattice", t=1)


def window10():
    out["window"] = ir_label_run(img_d, cams_d, keys.tolist(), want_pred=True)


steps = (("build_d2", build2), ("build_d5", build5), ("lattice_t10", lattice10), ("lattice_t1", lattice1), ("window_t10", window10))
ms = {k: [] for k, _ in steps}
for _ in range(a.rounds):
    for name, fn in steps:
        ms[name].append(timed(fn, a.reps))
med = {k: float(np.median(v)) for k, v in ms.items()}


def vertices(ws, D):
    n = torch.empty(1, dtype=torch.int32, device=dev)
    cap = H * W * (D + 1)
    t = [torch.empty(s, dtype=d, device=dev) for s, d in ((cap, torch.int32), (cap, torch.float32), (cap * D, torch.int32),
                                                            (2 * (D + 1) * cap, torch.int32))]
    call("mx_lattice_export", ptr(ws), *[ptr(x) for x in t], ptr(n), stream())
    return int(n.item())


per_iter = (med["lattice_t10"] - med["lattice_t1"]) / 9.0
res = {"image": [W, H], "C": C, "L": C + 1, "ms": med, "ms_rounds": ms, "lattice_ms_per_iteration": per_iter,
       "lattice_ms_once_per_image": med["lattice_t1"] - per_iter, "vertices_d2": vertices(ws2, 2), "vertices_d5": vertices(ws5, 5),
       "conf_pixels_that_differ": float((out["lattice"][0] != out["window"][0]).float().mean()),
       "train_aug_minutes_lattice": med["lattice_t10"] * N_TRAIN_AUG / 6e4,
       "train_aug_minutes_window": med["window_t10"] * N_TRAIN_AUG / 6e4}
print(f"C = {C} (L = {C + 1}), 500x375: build D=2 {med['build_d2']:.3f} ms ({res['vertices_d2']} vertices), D=5 {med['build_d5']:.3f} ms "
      f"({res['vertices_d5']} vertices); lattice t=10 {med['lattice_t10']:.2f} ms = {res['lattice_ms_once_per_image']:.2f} once + "
      f"{per_iter:.3f} per iteration; window t=10 {med['window_t10']:.1f} ms; train_aug {res['train_aug_minutes_lattice']:.1f} / "
      f"{res['train_aug_minutes_window']:.1f} min; conf differs on {res['conf_pixels_that_differ']:.4f} of the pixels", flush=True)
print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(res) + "\n")
