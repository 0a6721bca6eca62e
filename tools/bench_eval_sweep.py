"""The per-epoch evaluation sweeps per image on the HIP path: the rapid evaluation of train_mcl (train_mcl.py:286-318, CAM encoder)
and the validation of train_muscle (train_muscle.py:224-283, decoder), EfficientNet-B3 and B7, on a synthetic VOC tree of
500 x 375 and 375 x 500 images in a temporary directory, at `--batch` 1, 2, 4, 8 images per forward.  Per case:
  sweep  wall clock of the whole sweep per image: header reads, JPEG / PNG decoding, staging, forwards, counting, the final
         read of the table (median and min-max over `--repeats` sweeps after one warm-up sweep);
  gpu    the device part alone per image, from HIP events around each add / add_batch on images decoded beforehand.
batch 1 is the per-image loop (RapidEval.add, SegValidation.add).  On a checkout that has no batched drivers the tool runs
that loop itself, so `--batch 1` gives the baseline of an older commit with only this file copied in.
Not the contract bench."""
import argparse
import json
import os
import sys
import tempfile
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import PIL.Image
import torch

import muscle_amd
from muscle_amd import evaluation as E
from muscle_amd.data import MSFStager

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="efficientnet-b3,efficientnet-b7")
ap.add_argument("--batch", default="1,2,4,8")
ap.add_argument("--sweeps", default="rapid,seg")
ap.add_argument("--n", type=int, default=32, help="images of the synthetic list, half of each orientation")
ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--json", default=None, help="append the results as JSON lines to this file")
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_eval_sweep needs the GPU"
dev = torch.device("cuda:0")
BATCHED = hasattr(E, "rapid_eval_sweep")
K = 21


def make_tree(root, n):
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "SegmentationClass"))
    g = np.random.default_rng(0)
    names, labels = [], {}
    for i in range(n):
        h, w = ((375, 500), (500, 375))[i % 2]
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([127 + 100 * np.sin(xx / (9.0 + c) + i) * np.cos(yy / (13.0 - c)) for c in range(3)], -1) + g.normal(0, 10, (h, w, 3))
        nm = f"2009_{i:06d}"
        PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(os.path.join(root, "JPEGImages", nm + ".jpg"), quality=92)
        cls = [i % 20, (i + 7) % 20]
        lab = np.zeros(20, np.float32)
        lab[cls] = 1
        gt = g.choice([0, cls[0] + 1, cls[1] + 1, 255], size=(h // 16 + 1, w // 16 + 1), p=[0.6, 0.2, 0.15, 0.05]).astype(np.uint8)
        PIL.Image.fromarray(np.ascontiguousarray(np.kron(gt, np.ones((16, 16), np.uint8))[:h, :w]), "L").save(
            os.path.join(root, "SegmentationClass", nm + ".png"))
        names.append(nm)
        labels[nm] = lab
    return names, labels


def decode(root, nm):
    img = PIL.Image.open(os.path.join(root, "JPEGImages", nm + ".jpg")).convert("RGB")
    gt = np.array(PIL.Image.open(os.path.join(root, "SegmentationClass", nm + ".png")))
    return img, gt


def label_of(labels, nm):
    return torch.from_numpy(labels[nm]).view(1, -1)


def sweep_rapid(model, names, labels, root, batch):
    if BATCHED:
        return E.rapid_eval_sweep(model, names, root, labels, dev, batch=batch).best()[0]
    model.eval()
    ev, stager = E.RapidEval(dev), MSFStager(dev)
    for nm in names:
        img, gt = decode(root, nm)
        ev.add(model, stager(img, (1,))[0], label_of(labels, nm), torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(dev))
    return ev.best()[0]


def sweep_seg(model, names, labels, root, batch):
    if BATCHED:
        return E.validate_seg(model, names, root, dev, K, batch=batch)
    return E.validate_seg(model, names, root, dev, K)


def gpu_part(kind, model, names, labels, root, batch):
    """ms per image between HIP events around each add / add_batch, files decoded beforehand; the second of two passes."""
    sizes = [(nm, PIL.Image.open(os.path.join(root, "JPEGImages", nm + ".jpg")).size) for nm in names]
    buckets = E.size_buckets(sizes, batch) if BATCHED else [[nm] for nm in names]
    items = {nm: decode(root, nm) for nm in names}
    stager = MSFStager(dev)
    total = 0.0
    for rnd in range(2):
        ev = E.RapidEval(dev) if kind == "rapid" else E.SegValidation(dev, K)
        spans = []
        for b in buckets:
            t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            t0.record()
            if kind == "rapid" and len(b) == 1 and batch == 1:
                img, gt = items[b[0]]
                ev.add(model, stager(img, (1,))[0], label_of(labels, b[0]), torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(dev))
            elif kind == "rapid":
                imgs = torch.cat([stager(items[n][0], (1,))[0] for n in b], 0)
                gts = torch.from_numpy(np.stack([np.ascontiguousarray(items[n][1], dtype=np.uint8) for n in b])).to(dev)
                ev.add_batch(model, imgs, torch.cat([label_of(labels, n) for n in b], 0), gts)
            elif batch == 1:
                ev.add(model, items[b[0]][0], items[b[0]][1], b[0])
            else:
                ev.add_batch(model, [items[n][0] for n in b], [items[n][1] for n in b], b)
            t1.record()
            spans.append((t0, t1))
        torch.cuda.synchronize()
        total = sum(s.elapsed_time(e) for s, e in spans)
    return total / len(names)


with tempfile.TemporaryDirectory() as root:
    names, labels = make_tree(root, a.n)
    for name in a.models.split(","):
        for kind in a.sweeps.split(","):
            torch.manual_seed(0)
            model = (muscle_amd.MuSCLe(K, name, layers=3, last_pooling=False) if kind == "rapid"
                     else muscle_amd.MuSCLe(K, name, layers=3, last_pooling=True, mode="dec")).to(dev).eval()
            fn = sweep_rapid if kind == "rapid" else sweep_seg
            with torch.no_grad():
                for batch in [int(b) for b in a.batch.split(",")]:
                    if batch > 1 and not BATCHED:
                        continue
                    value = fn(model, names, labels, root, batch)                       # warm-up sweep
                    torch.cuda.synchronize()
                    t = []
                    for _ in range(a.repeats):
                        t0 = time.perf_counter()
                        fn(model, names, labels, root, batch)
                        torch.cuda.synchronize()
                        t.append((time.perf_counter() - t0) / len(names) * 1e3)
                    g = gpu_part(kind, model, names, labels, root, batch)
                    res = {"model": name, "sweep": kind, "batch": batch, "images": len(names), "batched_drivers": BATCHED,
                           "sweep_ms_per_image": [float(np.median(t)), float(min(t)), float(max(t))], "gpu_ms_per_image": g,
                           "value": float(value)}
                    print(f"{name} {kind:5s} batch={batch}: sweep {res['sweep_ms_per_image'][0]:7.2f} ms/img [{min(t):.2f}..{max(t):.2f}]  "
                          f"gpu {g:7.2f} ms/img  value {float(value):.6f}", flush=True)
                    if a.json:
                        with open(a.json, "a") as f:
                            f.write(json.dumps(res) + "\n")
            del model
