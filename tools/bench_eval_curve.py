"""The CAM-quality threshold curve (src/evaluation.py --type npy --curve True: 60 thresholds) on the HIP path: N synthetic
500 x 375 `{class: float32[H,W]}` dicts of 1-3 keys written to a temporary directory, then
  kernel   mx_camdict_confusion alone on maps already on the device (us per image, median and min-max over rounds),
  sweep    the whole per-file body of `python -m muscle_amd.evaluation`: np.load of the dict and PIL open of the ground
           truth, CamDictEval.add (stack, upload, launch), and the one table read at the end: files per second.
For scale it also times mx_eval_confusion (the training loop's kernel: 3 x nt LDS atomics per pixel) at the same 60
thresholds on a [21,H,W] map.  Not the contract bench."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from muscle_amd._lib import call, ptr, stream
from muscle_amd.evaluation import CamDictEval

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=200)
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--inner", type=int, default=50)
ap.add_argument("--json", default=None)
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_eval_curve needs the GPU"
import PIL.Image
dev = torch.device("cuda:0")
H, W, K = 375, 500, 21
THR = [i / 100.0 for i in range(60)]
rng = np.random.default_rng(0)


def synth(i):
    keys = sorted(rng.choice(20, 1 + i % 3, replace=False).tolist())
    lo = rng.random((len(keys), H // 25, W // 25)).astype(np.float32)
    maps = np.kron(lo, np.ones((25, 25), np.float32)) * rng.random((len(keys), H, W)).astype(np.float32)
    gt = np.kron(rng.choice([0] + [k + 1 for k in keys], size=(H // 25, W // 25)).astype(np.uint8), np.ones((25, 25), np.uint8))
    gt[rng.random((H, W)) < 0.03] = 255
    return {k: maps[j] for j, k in enumerate(keys)}, gt


def rounds(fn, inner, repeats):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    t = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        for _ in range(inner):
            fn()
        torch.cuda.synchronize()
        t.append((time.perf_counter() - t0) / inner * 1e6)
    return float(np.median(t)), float(min(t)), float(max(t))


res = {"image": [W, H], "thresholds": len(THR), "files": a.n}
ev = CamDictEval(dev, THR)
for nk in (1, 3):
    d, gt = synth(nk - 1)
    m = torch.from_numpy(np.stack([d[k] for k in sorted(d)])).to(dev)
    kk = torch.tensor(sorted(d), dtype=torch.int32, device=dev)
    g = torch.from_numpy(gt).to(dev)
    res[f"camdict_kernel_us_nkeep{nk}"] = rounds(lambda: call("mx_camdict_confusion", ptr(m), ptr(kk), nk, ptr(g), ptr(ev.thr), len(THR), K, H, W,
                                                              ptr(ev.counts), stream()), a.inner, a.repeats)
pred = torch.rand(K, H, W, device=dev)
lab = torch.ones(K, device=dev)
cnt = torch.zeros(len(THR), K, 3, dtype=torch.int64, device=dev)
res["eval_confusion_kernel_us_nt60"] = rounds(lambda: call("mx_eval_confusion", ptr(pred), ptr(lab), ptr(g), ptr(ev.thr), len(THR), K, H, W, ptr(cnt),
                                                           stream()), a.inner, a.repeats)
with tempfile.TemporaryDirectory() as td:
    for i in range(a.n):
        d, gt = synth(i)
        np.save(os.path.join(td, f"{i}.npy"), d)
        PIL.Image.fromarray(gt, "L").save(os.path.join(td, f"{i}.png"))
    rates = []
    for _ in range(3):
        ev = CamDictEval(dev, THR)
        t0 = time.perf_counter()
        for i in range(a.n):
            ev.add(np.load(os.path.join(td, f"{i}.npy"), allow_pickle=True).item(), np.array(PIL.Image.open(os.path.join(td, f"{i}.png"))))
        mious = ev.mious()
        rates.append(a.n / (time.perf_counter() - t0))
    res["sweep_files_per_s"] = [float(np.median(rates)), float(min(rates)), float(max(rates))]
    res["best_miou"] = float(max(mious))
for k, v in res.items():
    print(k, v, flush=True)
print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(res) + "\n")
