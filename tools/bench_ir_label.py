"""IR-label CRFs (muscle_amd.ir_label, mx_ir_label) per 500 x 375 image: synthetic image and C smooth CAMs, C = 2 and C = 6
(L = 3 / 7 labels), t = 10, trunc 4 (R = 12 / 200), sxy 3 / 50, srgb 5, weights 3 / 10.  Three ways to the same two label CRFs,
timed with device events in the order A / B / C, repeated --rounds times (alternating, same process, same GPU):
  baseline  two mx_crf_inference calls on one-hot maps with this model's parameters (what the library offered before):
            2 x (1 normaliser + t message) bilateral-sized passes,
  fused     mx_ir_label, fused = 1: both problems as columns of one stencil-GEMM: 1 + t bilateral-sized passes,
  unfused   mx_ir_label, fused = 0: the normalisers once, then one problem per pass: 1 + 2 t.
Reports ms per image (median of the rounds; each round is --reps calls between two events after a warm-up), the window pairs of
one bilateral pass, the pair rate of the fused call (pairs of all its bilateral and Gaussian passes over its time) and the
projected time for the 10 582 images of train_aug at that rate.  Checks that the fused and unfused maps agree bit for bit and that
the baseline's argmax maps agree with them.  Not the contract bench."""
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
ap.add_argument("--classes", default="2,6")
ap.add_argument("--reps", type=int, default=3)
ap.add_argument("--rounds", type=int, default=3)
ap.add_argument("--json", default=None, help="append the results as one JSON line to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
H, W, T_ITERS, TRUNC, N_TRAIN_AUG = 375, 500, IR.T, 4.0, 10582
SG, WG, SB, SRGB, WB = crf.LABEL_MODEL


def window_pairs(R):
    cx = sum(min(x + R, W - 1) - max(x - R, 0) + 1 for x in range(W))
    cy = sum(min(y + R, H - 1) - max(y - R, 0) + 1 for y in range(H))
    return cx * cy


def radius(trunc, sxy):
    r = int(np.ceil(trunc * sxy))
    return max(H, W) if trunc <= 0 or r >= max(H, W) - 1 else r


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


pairs_b, pairs_g = window_pairs(radius(TRUNC, SB)), window_pairs(radius(TRUNC, SG))
res = {"image": [W, H], "t": T_ITERS, "trunc": TRUNC, "R_gauss": radius(TRUNC, SG), "R_bilateral": radius(TRUNC, SB),
       "pairs_bilateral": pairs_b, "pairs_gauss": pairs_g}
print(f"R = {res['R_gauss']} / {res['R_bilateral']}: {pairs_b / 1e9:.2f}e9 bilateral and {pairs_g / 1e9:.3f}e9 Gaussian window pairs per pass",
      flush=True)

for C in [int(s) for s in a.classes.split(",")]:
    img, cams, keys = IR.synthetic(100 + C, H, W, C)
    L = C + 1
    labs = IR.label_maps(cams)
    img_d, cams_d = torch.from_numpy(img).to(dev), torch.from_numpy(cams).to(dev)
    onehot = [torch.from_numpy((np.arange(L)[:, None, None] == labs[g][None]).astype(np.float32)).to(dev) for g in range(2)]
    ws = torch.empty(lib().mx_crf_workspace_bytes(L, H, W) // 4, device=dev)
    pred = torch.empty(2, H, W, dtype=torch.uint8, device=dev)
    conf_c = (IR.GT_PROB - 1.0 / L) / (1.0 - 1.0 / L)

    def baseline():
        for g in range(2):
            call("mx_crf_inference", ptr(img_d), ptr(onehot[g]), L, H, W, T_ITERS, conf_c, SG, WG, SB, SRGB, WB, TRUNC, ptr(ws), None,
                 ptr(pred[g]), stream())

    out = {}

    def fused():
        out["fused"] = ir_label_run(img_d, cams_d, keys.tolist(), trunc=TRUNC, fused=True, want_pred=True)

    def unfused():
        out["unfused"] = ir_label_run(img_d, cams_d, keys.tolist(), trunc=TRUNC, fused=False, want_pred=True)

    ms = {"baseline": [], "fused": [], "unfused": []}
    for _ in range(a.rounds):
        for name, fn in (("baseline", baseline), ("fused", fused), ("unfused", unfused)):
            ms[name].append(timed(fn, a.reps))
    same = bool(torch.equal(out["fused"][0], out["unfused"][0]) and torch.equal(out["fused"][1], out["unfused"][1]))
    agree = float((out["fused"][1] == pred).float().mean())
    med = {k: float(np.median(v)) for k, v in ms.items()}
    passes_pairs = (1 + T_ITERS) * pairs_b + (1 + T_ITERS) * pairs_g
    rate = passes_pairs / (med["fused"] * 1e-3)
    r = res[f"C{C}"] = {"L": L, "ms": med, "ms_rounds": ms, "fused_pairs_per_s": rate, "fused_equals_unfused": same,
                        "baseline_argmax_agreement": agree, "train_aug_minutes_fused": med["fused"] * N_TRAIN_AUG / 6e4,
                        "train_aug_minutes_baseline": med["baseline"] * N_TRAIN_AUG / 6e4}
    print(f"C = {C} (L = {L}): baseline {med['baseline']:.1f} ms, fused {med['fused']:.1f} ms ({med['fused'] / med['baseline']:.2f} x), "
          f"unfused {med['unfused']:.1f} ms; fused {rate / 1e12:.2f}e12 pairs/s; train_aug {r['train_aug_minutes_fused']:.1f} min "
          f"(baseline {r['train_aug_minutes_baseline']:.1f}); fused == unfused bits: {same}; baseline argmax agreement {agree:.6f}",
          flush=True)

print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(res) + "\n")
