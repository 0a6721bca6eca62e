"""The kernels of the class-balanced self-training labels (csrc/selflabel.hip) at one VOC image, 375 x 500, K = 21:
  mx_conf_code   without and with a ground truth (label, code and the LDS-counted tables; reads prob once),
  mx_conf_select and mx_code_hist on the stored pair,
  mx_seg_infer   the launch that produced the map (12 passes of the decoder's low-res logits), in the same run, for scale.
Kernel times are device events around `--reps` back-to-back launches after a warm-up; the achieved bytes/s of mx_conf_code is
over the bytes the algorithm needs, K*H*W*4 + 2*H*W (+ H*W with a ground truth).  The probability map is the one mx_seg_infer
wrote from random weights, sharpened (p^8, renormalised); the second line of the output says how many classes and codes it
uses and how confident it is (a trained decoder's map is more confident: fewer distinct table entries per wave).
Writes the lines it prints to --out (default profiles/selflabel_bench.txt).  Not the contract bench; no pass/fail number."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np
import torch

import muscle_amd
from muscle_amd import selflabel as SL
from muscle_amd._lib import call, ptr, stream
from muscle_amd.data import MSFStager
from muscle_amd.infer_seg import DEFAULT_SCALES

ap = argparse.ArgumentParser()
ap.add_argument("--model", default="efficientnet-b0", help="the decoder whose low-res logits feed mx_seg_infer (the kernels timed here do not depend on it)")
ap.add_argument("--reps", type=int, default=200)
ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "selflabel_bench.txt"))
a = ap.parse_args()

if not torch.cuda.is_available():
    sys.exit("bench_selflabel.py measures on the GPU; there is none here")
dev = torch.device("cuda:0")
torch.manual_seed(0)
H, W, K = 375, 500, 21
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def timed_us(fn, reps):
    for _ in range(10):
        fn()
    torch.cuda.synchronize()
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    for _ in range(reps):
        fn()
    t1.record()
    torch.cuda.synchronize()
    return t0.elapsed_time(t1) / reps * 1e3


model = muscle_amd.MuSCLe(K, a.model, layers=3, last_pooling=True, mode="dec").to(dev).eval()
model.fold_eval_bn()
import PIL.Image
g = np.random.default_rng(0)
pil = PIL.Image.fromarray(g.integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB")
imgs = MSFStager(dev)(pil, DEFAULT_SCALES)
rows, lrs = [], []
with torch.no_grad():
    for i in range(0, len(imgs), 2):
        lr = model(torch.cat(imgs[i:i + 2], 0), cam="seg_lr")
        lrs.append(lr)
        for b in range(2):
            rows.append([lr[b].data_ptr(), lr.shape[1], lr.shape[2], imgs[i + b].shape[2], imgs[i + b].shape[3], b, 0, 0])
tab = torch.tensor(rows, dtype=torch.int64).to(dev)
pred = torch.empty(H, W, dtype=torch.uint8, device=dev)
mean = torch.empty(K, H, W, device=dev)
seg = lambda: call("mx_seg_infer", ptr(tab), len(rows), 24, K, H, W, None, ptr(pred), ptr(mean), stream())  # noqa: E731
seg()
prob = mean ** 8
prob = (prob / prob.sum(0, keepdim=True)).contiguous()
gt = torch.from_numpy(g.choice([0, 1, 4, 12, 15, 255], size=(H, W)).astype(np.uint8)).to(dev)

label = torch.empty(H, W, dtype=torch.uint8, device=dev)
code = torch.empty(H, W, dtype=torch.uint8, device=dev)
out = torch.empty(H, W, dtype=torch.uint8, device=dev)
t = torch.zeros(3, K, 256, dtype=torch.int64, device=dev)
kept = torch.zeros(K, 2, dtype=torch.int64, device=dev)
n = H * W


def conf(with_gt):
    call("mx_conf_code", ptr(prob), K, H, W, ptr(label), ptr(code), ptr(gt) if with_gt else None, ptr(t[0]),
         ptr(t[1]) if with_gt else None, ptr(t[2]) if with_gt else None, stream())


def hist(with_gt):
    call("mx_code_hist", ptr(label), ptr(code), ptr(gt) if with_gt else None, n, K, ptr(t[0]), ptr(t[1]) if with_gt else None,
         ptr(t[2]) if with_gt else None, stream())


conf(False)
torch.cuda.synchronize()
hst = t[0].cpu().numpy().copy()
tc = torch.from_numpy(SL.thresholds(hst, 0.5)).to(dev)
sel = lambda: call("mx_conf_select", ptr(label), ptr(code), ptr(tc), n, K, ptr(out), ptr(kept), stream())  # noqa: E731

res = {"image": [W, H], "K": K, "reps": a.reps, "passes": len(rows)}
used = np.flatnonzero(hst.sum(0))
say(f"# tools/bench_selflabel.py: {H}x{W}, K = {K}, {a.reps} back-to-back launches per figure (device events), {torch.cuda.get_device_name(0)}")
say(f"# the map: {int((hst.sum(1) > 0).sum())} predicted classes, {used.size} codes in use ({used.min()}..{used.max()}), "
    f"{100.0 * hst[:, :int(SL.code_of(0.99)) + 1].sum() / n:.1f} % of the pixels with conf > 0.99")
for name, fn, nbytes in (("mx_conf_code", lambda: conf(False), K * n * 4 + 2 * n),
                         ("mx_conf_code with gt", lambda: conf(True), K * n * 4 + 3 * n),
                         ("mx_code_hist", lambda: hist(False), 2 * n),
                         ("mx_code_hist with gt", lambda: hist(True), 3 * n),
                         ("mx_conf_select", sel, 3 * n),
                         ("mx_seg_infer (pred + prob, 12 passes)", seg, None)):
    # two rounds of every figure: the spread between them is the noise of this run
    us = [timed_us(fn, a.reps) for _ in range(2)]
    res[name] = us
    rate = "" if nbytes is None else f"  {nbytes / 1e6:6.2f} MB needed -> {nbytes / min(us) / 1e6:7.3f} TB/s achieved"
    say(f"{name:40s} {us[0]:8.2f} / {us[1]:8.2f} us per launch{rate}")
# the same launch on a confident map of smooth regions (softmax of 12 x a bilinearly upsampled 12 x 16 field): few entries per wave
prob = torch.softmax(12.0 * torch.nn.functional.interpolate(torch.randn(1, K, 12, 16, device=dev), size=(H, W), mode="bilinear",
                                                            align_corners=False)[0], dim=0).contiguous()
t.zero_()
conf(False)
torch.cuda.synchronize()
hst = t[0].cpu().numpy().copy()
used = np.flatnonzero(hst.sum(0))
say(f"# a confident map: {int((hst.sum(1) > 0).sum())} predicted classes, {used.size} codes in use ({used.min()}..{used.max()}), "
    f"{100.0 * hst[:, :int(SL.code_of(0.99)) + 1].sum() / n:.1f} % of the pixels with conf > 0.99")
for name, fn, nbytes in (("mx_conf_code, confident map", lambda: conf(False), K * n * 4 + 2 * n),
                         ("mx_conf_code with gt, confident map", lambda: conf(True), K * n * 4 + 3 * n)):
    us = [timed_us(fn, a.reps) for _ in range(2)]
    res[name] = us
    say(f"{name:40s} {us[0]:8.2f} / {us[1]:8.2f} us per launch  {nbytes / 1e6:6.2f} MB needed -> {nbytes / min(us) / 1e6:7.3f} TB/s achieved")
say(json.dumps(res))
os.makedirs(os.path.dirname(a.out), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
