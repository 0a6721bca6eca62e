"""Dense CRF (muscle_amd.crf, mx_crf_inference) per 500 x 375 image: synthetic image and probability map, 21 labels, t = 4,
scale_factor 1.5 (sxy 2 / 21.3, srgb 10), for trunc 3 / 4 / 5.  Reports ms per image for
  norm    the normaliser pass (mx_crf_normalizers: both window sums of the kernel weights),
  iter    one mean-field iteration (both messages + softmax): (t=4 call - t=1 call) / 3,
  full    the whole call, t = 4 (normalisers + unary + 4 iterations),
the pixel pairs of one bilateral pass and the implied pair rate, next to the bound of the f32 matrix pipe: every pair is one
row of a 32x32x2 MFMA (labels padded 21 -> 32: 64 FLOP per pair) at 157.3 TFLOP/s.
  e2e     infer.infer_seg on EfficientNet-B7 (12 passes) with and without crf_img, ms per image.
Not the contract bench.  --part runs one of them (each GPU step of a job can then have its own time limit)."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

from muscle_amd import crf
from muscle_amd._lib import call, lib, ptr, stream

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["all", "norm", "iter", "full", "e2e"])
ap.add_argument("--trunc", default="3,4,5")
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--model", default="efficientnet-b7")
ap.add_argument("--json", default=None, help="append the results as one JSON line to this file")
a = ap.parse_args()

dev = torch.device("cuda:0")
H, W, L, T_ITERS, SF = 375, 500, 21, 4, 1.5
F32_MATRIX_PEAK = 157.3e12
g = np.random.default_rng(0)
img = np.zeros((H, W, 3))
img[:, :W // 3] = [200, 30, 30]
img[H // 4:3 * H // 4, W // 3:4 * W // 5] = [20, 180, 60]
img[:, 4 * W // 5:] = [30, 40, 200]
img = np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
logit = torch.from_numpy(g.normal(0, 2.0, (L, H // 5, W // 5)).astype(np.float32))
probs = torch.softmax(torch.nn.functional.interpolate(logit[None], size=(H, W), mode="bilinear")[0] * 2, dim=0).to(dev)
img_d = torch.from_numpy(img).to(dev)
res = {"image": [W, H], "labels": L, "t": T_ITERS, "scale_factor": SF}


def timed(fn, reps):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(reps):
        fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) / reps * 1e3


def window_pairs(R):
    cx = sum(min(x + R, W - 1) - max(x - R, 0) + 1 for x in range(W))
    cy = sum(min(y + R, H - 1) - max(y - R, 0) + 1 for y in range(H))
    return cx * cy


def radius(trunc, sxy):
    r = int(np.ceil(trunc * sxy))
    return max(H, W) if trunc <= 0 or r >= max(H, W) - 1 else r


sg, sb = crf.GAUSS_SXY / SF, crf.BILATERAL_SXY / SF
for trunc in [float(s) for s in a.trunc.split(",")] if a.part != "e2e" else []:
    key = f"trunc{trunc:g}"
    r = res[key] = {"R_gauss": radius(trunc, sg), "R_bilateral": radius(trunc, sb)}
    pairs = r["pairs_bilateral"] = window_pairs(r["R_bilateral"])
    r["pairs_gauss"] = window_pairs(r["R_gauss"])
    r["mfma_bound_ms_per_pass"] = pairs * 64 / F32_MATRIX_PEAK * 1e3
    line = f"trunc {trunc:g}: R = {r['R_gauss']} / {r['R_bilateral']}, {pairs / 1e9:.2f}e9 bilateral pairs per pass (bound {r['mfma_bound_ms_per_pass']:.2f} ms)"
    if a.part in ("all", "norm"):
        ws = torch.empty(lib().mx_crf_workspace_bytes(L, H, W) // 4, device=dev)
        ng, nb = torch.empty(H, W, device=dev), torch.empty(H, W, device=dev)
        r["norm_ms"] = timed(lambda: call("mx_crf_normalizers", ptr(img_d), H, W, sg, sb, crf.BILATERAL_SRGB, trunc, ptr(ws), ptr(ng),
                                          ptr(nb), stream()), a.reps)
        line += f"; normalisers {r['norm_ms']:.2f} ms"
    if a.part in ("all", "iter", "full"):
        r["full_ms"] = timed(lambda: crf.crf_run(img_d, probs, T_ITERS, SF, L, 0.5, trunc, want_q=True, want_pred=True), a.reps)
        line += f"; whole call (t={T_ITERS}) {r['full_ms']:.2f} ms"
    if a.part in ("all", "iter"):
        t1 = timed(lambda: crf.crf_run(img_d, probs, 1, SF, L, 0.5, trunc, want_q=True, want_pred=True), a.reps)
        r["iter_ms"] = (r["full_ms"] - t1) / (T_ITERS - 1)
        r["iter_pairs_per_s"] = (pairs + r["pairs_gauss"]) / (r["iter_ms"] * 1e-3)
        r["iter_vs_mfma_bound"] = r["iter_ms"] / ((pairs + r["pairs_gauss"]) * 64 / F32_MATRIX_PEAK * 1e3)
        line += (f"; one iteration {r['iter_ms']:.2f} ms = {r['iter_pairs_per_s'] / 1e12:.2f}e12 pairs/s "
                 f"({r['iter_vs_mfma_bound']:.2f} x the f32 MFMA bound)")
    print(line, flush=True)

if a.part in ("all", "e2e"):
    import PIL.Image
    import muscle_amd
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    from muscle_amd.infer_seg import DEFAULT_SCALES
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(L, a.model, layers=3, last_pooling=True, mode="dec").to(dev).eval()
    model.fold_eval_bn()
    imgs = MSFStager(dev)(PIL.Image.fromarray(img, "RGB"), DEFAULT_SCALES)
    reps = max(3, a.reps // 2)
    res["infer_seg_ms"] = timed(lambda: infer_seg(model, imgs, H, W), reps)
    res["infer_seg_crf_ms"] = timed(lambda: infer_seg(model, imgs, H, W, crf_img=img_d, crf_t=T_ITERS, crf_trunc=4.0), reps)
    print(f"{a.model} infer_seg, {len(imgs)} passes: {res['infer_seg_ms']:.2f} ms/image without the CRF, "
          f"{res['infer_seg_crf_ms']:.2f} ms/image with it (t={T_ITERS}, trunc 4)", flush=True)

print(json.dumps(res), flush=True)
if a.json:
    with open(a.json, "a") as f:
        f.write(json.dumps(res) + "\n")
