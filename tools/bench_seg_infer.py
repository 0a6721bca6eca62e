"""Segmentation inference (infer_seg.py) per image on the HIP path: EfficientNet-B7 decoder (mode='dec', 3 BiFPN layers,
last_pooling), one synthetic 500 x 375 image, scales 0.5-1.75 x flip (12 passes).  Reports ms per image for
  forward  the 6 batch-2 cam='seg_lr' forwards of infer.infer_seg,
  fused    mx_seg_infer over the 12 low-res maps (pred only, and pred + the [21,H,W] mean probability map),
  torch    the same post-processing written as torch ops on the GPU from the same low-res maps (align_corners upsample to
           the pass size, softmax, F.interpolate to the image, flip, mean, argmax) - the baseline the fused kernel replaces.
Not the contract bench.  --part runs one of the three (each GPU step of a job can then have its own time limit)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch
import torch.nn.functional as F

import muscle_amd
from muscle_amd._lib import call, ptr, stream
from muscle_amd.data import MSFStager
from muscle_amd.infer import infer_seg
from muscle_amd.infer_seg import DEFAULT_SCALES

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="efficientnet-b7")
ap.add_argument("--part", default="all", choices=["all", "forward", "post"])
ap.add_argument("--reps", type=int, default=20)
ap.add_argument("--json", default=None, help="append the results as one JSON line to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
torch.manual_seed(0)
H, W, K = 375, 500, 21
model = muscle_amd.MuSCLe(K, a.model, layers=3, last_pooling=True, mode="dec").to(dev).eval()
model.fold_eval_bn()
import PIL.Image
pil = PIL.Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB")
imgs = MSFStager(dev)(pil, DEFAULT_SCALES)
res = {"model": a.model, "image": [W, H], "passes": len(imgs)}


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def forwards():
    out = []
    with torch.no_grad():
        for i in range(0, len(imgs), 2):
            out.append(model(torch.cat(imgs[i:i + 2], 0), cam="seg_lr"))
    return out


if a.part in ("all", "forward"):
    res["forward_ms"] = timed(forwards, max(3, a.reps // 4))
    res["infer_seg_ms"] = timed(lambda: infer_seg(model, imgs, H, W), max(3, a.reps // 4))
    print(f"{a.model} 6 x batch-2 cam='seg_lr' forwards: {res['forward_ms']:8.2f} ms/image;  infer_seg end to end (forwards + "
          f"fused post): {res['infer_seg_ms']:8.2f} ms/image", flush=True)

if a.part in ("all", "post"):
    lrs = forwards()
    rows = []
    for j, lr in enumerate(lrs):
        for b in range(2):
            im = imgs[2 * j + b]
            rows.append([lr[b].data_ptr(), lr.shape[1], lr.shape[2], im.shape[2], im.shape[3], b, 0, 0])
    tab = torch.tensor(rows, dtype=torch.int64).to(dev)
    pred = torch.empty(H, W, dtype=torch.uint8, device=dev)
    prob = torch.empty(K, H, W, device=dev)

    def fused(with_prob):
        call("mx_seg_infer", ptr(tab), len(rows), 24, K, H, W, None, ptr(pred), ptr(prob) if with_prob else None, stream())

    def torch_post():                                   # from the same low-res maps: upsample (cam='seg'), softmax, resize, ...
        acc = torch.zeros(K, H, W, device=dev)
        for n in range(len(rows)):
            lr, im = lrs[n // 2][n % 2:n % 2 + 1, ..., :K].permute(0, 3, 1, 2), imgs[n]
            s = F.interpolate(lr, size=im.shape[2:], mode="bilinear", align_corners=True)
            p = F.interpolate(torch.softmax(s, dim=1), size=(H, W), mode="bilinear", align_corners=False)[0]
            acc += torch.flip(p, dims=[2]) if n % 2 else p
        m = acc / len(rows)
        return m, m.argmax(0).to(torch.uint8)

    res["fused_pred_ms"] = timed(lambda: fused(False), a.reps)
    res["fused_pred_prob_ms"] = timed(lambda: fused(True), a.reps)
    res["torch_post_ms"] = timed(torch_post, a.reps)
    m, pt = torch_post()
    fused(True)
    torch.cuda.synchronize()
    res["max_abs_prob_diff_vs_torch"] = float((m - prob).abs().max())
    res["pred_agreement_vs_torch"] = float((pt == pred).float().mean())
    print(f"post-processing of {len(rows)} passes -> [{K},{H},{W}]: fused pred only {res['fused_pred_ms'] * 1e3:8.1f} us, "
          f"fused pred + prob {res['fused_pred_prob_ms'] * 1e3:8.1f} us, torch ops {res['torch_post_ms'] * 1e3:8.1f} us per image"
          f"  (prob max |diff| {res['max_abs_prob_diff_vs_torch']:.2e}, pred agreement {res['pred_agreement_vs_torch']:.6f})",
          flush=True)

print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(res) + "\n")
