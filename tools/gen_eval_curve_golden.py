"""Generate tests/golden/eval_curve.npz by running the REFERENCE's src/evaluation.py::do_python_eval as it is (its 8 worker
processes, files and all) on the CPU (build container only; never on the GPU box).

    python tools/gen_eval_curve_golden.py

The reference is imported as oracle/gen_golden.py::load_reference does.  Synthetic `{class: float32[H,W]}` dicts in the
layout infer_mcl.py:166-182 writes (1-4 keys per image, inserted unsorted, exact ties between channels and with the
thresholds 0.00 and 0.30, negative values), ground-truth PNGs with 255-pixels and 8-bit label PNGs in the layout of
infer_seg.py:129-131 are written to a temporary directory.  Stored: the inputs (maps, keys in insertion order, gt, label
maps) and what do_python_eval returned: the loglists (21 category IoUs in percent + mIoU) for input_type='npy' at the 60
thresholds of src/evaluation.py:128-131 and for input_type='png'.
"""
from __future__ import annotations

import os
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

from oracle import gen_golden as GG  # noqa: E402

OUT = os.path.join(ROOT, "tests", "golden", "eval_curve.npz")
SIZES = ((31, 45), (40, 37), (52, 60), (36, 36))


def main() -> None:
    from PIL import Image
    GG.load_reference()
    from src.evaluation import do_python_eval
    rng = np.random.default_rng(23)
    out = {}
    with tempfile.TemporaryDirectory() as td:
        pred_dir, gt_dir, png_dir = (os.path.join(td, d) for d in ("pred", "gt", "png"))
        for d in (pred_dir, gt_dir, png_dir):
            os.makedirs(d)
        names = []
        for i, (H, W) in enumerate(SIZES):
            keys = rng.permutation(20)[:1 + i].tolist()                    # insertion order of the dict: unsorted
            maps = (rng.random((len(keys), H, W)) * 0.7 - 0.05).astype(np.float32)      # some negative values
            maps[:, rng.random((H, W)) < 0.08] = np.float32(0.3)           # ties between channels and with t = 0.30
            maps[:, rng.random((H, W)) < 0.05] = 0.0                       # ... and with t = 0.00
            maps[0][rng.random((H, W)) < 0.05] = np.float32(0.17)          # on a threshold, one channel only
            gt = rng.integers(0, 21, size=(H // 6 + 1, W // 6 + 1)).astype(np.uint8)
            gt = np.kron(gt, np.ones((6, 6), np.uint8))[:H, :W].copy()
            if keys:
                gt[rng.random((H, W)) < 0.3] = keys[0] + 1                 # so that true positives exist
            gt[rng.random((H, W)) < 0.07] = 255
            png = rng.integers(0, 21, size=(H, W)).astype(np.uint8)
            agree = rng.random((H, W)) < 0.4
            png[agree] = np.where(gt[agree] < 21, gt[agree], 0)
            name = f"img{i}"
            names.append(name)
            np.save(os.path.join(pred_dir, name + ".npy"), {k: maps[j] for j, k in enumerate(keys)})
            Image.fromarray(gt).save(os.path.join(gt_dir, name + ".png"))
            Image.fromarray(png).save(os.path.join(png_dir, name + ".png"))
            out[f"keys{i}"] = np.array(keys, np.int32)
            out[f"maps{i}"] = maps
            out[f"gt{i}"] = gt
            out[f"png{i}"] = png
        thr = [i / 100.0 for i in range(60)]                               # src/evaluation.py:128-129
        rows = []
        for t in thr:
            ll = do_python_eval(pred_dir, gt_dir, names, 21, "npy", t)
            rows.append([ll[k] for k in list(ll.keys())])
        out["thresholds"] = np.array(thr, np.float64)
        out["loglists_npy"] = np.array(rows, np.float64)
        ll = do_python_eval(png_dir, gt_dir, names, 21, "png")
        out["loglist_png"] = np.array([ll[k] for k in list(ll.keys())], np.float64)
    assert np.ptp(out["loglists_npy"][:, -1]) > 1.0 and out["loglist_png"][-1] > 5.0      # not degenerate
    np.savez_compressed(OUT, **out)
    print("wrote", OUT, os.path.getsize(OUT), "bytes")


if __name__ == "__main__":
    main()
