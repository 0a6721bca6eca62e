"""CAM generation post-processing (infer_mcl.py:124-174) per image on the HIP path: one synthetic 500 x 375 image, scales
0.5/1/1.5/2 x flip (8 passes), EfficientNet-B3 and B7 CAM encoders.  For nkeep in {1, 2, 5, 20} labels and want_cam on / off:
  per-pass  what infer.infer_cam enqueues after the forwards: two zeroed [20,H,W] accumulators, 16 mx_infer_accum (one
            per pass and map, all 20 channels), two mx_infer_norm, two index_select of the kept channels;
  fused     what infer.infer_cam_fused enqueues: the pass table and keep list uploads, ONE mx_cam_infer over the kept
            channels, one mx_infer_norm per requested map (want_cam off: the SGC map only).
Both work on the same low-res maps of one set of forwards, are alternated in one process (warm-up, then `--repeats`
rounds of `--inner` calls each, every round closed by a device synchronise) and reported as the median round with the
min-max spread over rounds, in microseconds per image.  The outputs are compared bit for bit first.
Then the whole loop body per image, forwards and device->host copies included: infer_cam against infer_cam_fused.
Not the contract bench."""
import argparse
import json
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import muscle_amd
from muscle_amd._lib import call, ptr, stream
from muscle_amd.data import MSFStager
from muscle_amd.infer import infer_cam, infer_cam_fused

ap = argparse.ArgumentParser()
ap.add_argument("--models", default="efficientnet-b3,efficientnet-b7")
ap.add_argument("--repeats", type=int, default=9)
ap.add_argument("--inner", type=int, default=40)
ap.add_argument("--body_inner", type=int, default=4)
ap.add_argument("--json", default=None, help="append the results as JSON lines to this file")
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_cam_infer needs the GPU"
dev = torch.device("cuda:0")
H, W, K = 375, 500, 21
LABELS = {1: [14], 2: [8, 14], 5: [1, 6, 8, 14, 17], 20: list(range(20))}
import PIL.Image
pil = PIL.Image.fromarray(np.random.default_rng(0).integers(0, 256, (H, W, 3), dtype=np.uint8), "RGB")


def rounds(fns, inner, repeats):
    """Alternate the callables: per round each runs `inner` times between two synchronises.  -> per fn (median, min, max) in us."""
    for fn in fns:
        for _ in range(3):
            fn()
    torch.cuda.synchronize()
    t = [[] for _ in fns]
    for _ in range(repeats):
        for j, fn in enumerate(fns):
            t0 = time.perf_counter()
            for _ in range(inner):
                fn()
            torch.cuda.synchronize()
            t[j].append((time.perf_counter() - t0) / inner * 1e6)
    return [(float(np.median(x)), float(min(x)), float(max(x))) for x in t]


for name in a.models.split(","):
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(K, name, layers=3, last_pooling=False).to(dev).eval()
    model.fold_eval_bn()
    imgs = MSFStager(dev)(pil)
    lrs, rows = [], []
    with torch.no_grad():
        for i in range(0, len(imgs), 2):
            cam_lr, sgc_lr, _, _ = model(torch.cat(imgs[i:i + 2], 0), cam="cam_lr")
            lrs.append((cam_lr, sgc_lr))
            for b in range(2):
                rows.append([cam_lr[b].data_ptr(), sgc_lr[b].data_ptr(), cam_lr.shape[1], cam_lr.shape[2], imgs[i].shape[2], imgs[i].shape[3], b, 0])
    lds = lrs[0][0].shape[3]
    for nkeep, classes in LABELS.items():
        label = torch.zeros(1, 20)
        label[0, classes] = 1
        sel = torch.tensor(classes, device=dev)
        for want_cam in (True, False):
            def per_pass():
                acc_cam = torch.zeros(K - 1, H, W, device=dev)
                acc_sgc = torch.zeros(K - 1, H, W, device=dev)
                for n, r in enumerate(rows):
                    call("mx_infer_accum", r[0], ptr(acc_cam), r[2], r[3], lds, K, r[4], r[5], H, W, r[6], stream())
                    call("mx_infer_accum", r[1], ptr(acc_sgc), r[2], r[3], lds, K, r[4], r[5], H, W, r[6], stream())
                call("mx_infer_norm", ptr(acc_cam), K - 1, H * W, stream())
                call("mx_infer_norm", ptr(acc_sgc), K - 1, H * W, stream())
                return acc_cam.index_select(0, sel), acc_sgc.index_select(0, sel)

            def fused():
                tab = torch.tensor(rows, dtype=torch.int64).to(dev)
                idx = torch.tensor(classes, dtype=torch.int32).to(dev)
                oc = torch.empty(nkeep, H, W, device=dev) if want_cam else None
                os_ = torch.empty(nkeep, H, W, device=dev)
                call("mx_cam_infer", ptr(tab), len(rows), lds, K, H, W, ptr(idx), nkeep, ptr(oc), ptr(os_), stream())
                if want_cam:
                    call("mx_infer_norm", ptr(oc), nkeep, H * W, stream())
                call("mx_infer_norm", ptr(os_), nkeep, H * W, stream())
                return oc, os_

            rc, rs = per_pass()
            fc, fs = fused()
            torch.cuda.synchronize()
            equal = bool(torch.equal(rs, fs) and (fc is None or torch.equal(rc, fc)))
            (pm, plo, phi), (fm, flo, fhi) = rounds([per_pass, fused], a.inner, a.repeats)
            bodies = rounds([lambda: infer_cam(model, imgs, label, H, W),
                             lambda: infer_cam_fused(model, imgs, label, H, W, want_cam=want_cam)], a.body_inner, max(3, a.repeats // 2))
            res = {"model": name, "image": [W, H], "passes": len(rows), "nkeep": nkeep, "want_cam": want_cam, "bit_equal": equal,
                   "per_pass_us": [pm, plo, phi], "fused_us": [fm, flo, fhi],
                   "infer_cam_body_us": list(bodies[0]), "infer_cam_fused_body_us": list(bodies[1])}
            print(f"{name} nkeep={nkeep:2d} want_cam={int(want_cam)} bit_equal={equal}: post-processing per-pass {pm:8.1f} us "
                  f"[{plo:.1f}..{phi:.1f}]  fused {fm:8.1f} us [{flo:.1f}..{fhi:.1f}]   whole body infer_cam {bodies[0][0] / 1e3:7.2f} ms "
                  f"[{bodies[0][1] / 1e3:.2f}..{bodies[0][2] / 1e3:.2f}]  infer_cam_fused {bodies[1][0] / 1e3:7.2f} ms "
                  f"[{bodies[1][1] / 1e3:.2f}..{bodies[1][2] / 1e3:.2f}]", flush=True)
            if a.json:
                with open(a.json, "a") as f:
                    f.write(json.dumps(res) + "\n")
    del model, lrs
