"""`python -m muscle_amd.cam_to_ir_label`: the IR labels that `train_irn --ir_label_dir` reads, from the CAM dicts that
`infer_mcl` writes (IRN's cam_to_ir_label step around src/imutils.py:477-491, `crf_inference_label`), on the HIP path.

For every name of --infer_list: <voc12_root>/JPEGImages/<name>.jpg and <cam_dir>/<name>.npy ({class index: float [H,W]}) give
<ir_label_out_dir>/<name>.png, uint8: 0 background, k+1 class k, 255 ignore (`muscle_amd.ir_label` states the rule).

What a caller should know:
  * the CRF is the windowed model of `infer_seg --crf 2` with the label unary (--crf_trunc: R_m = ceil(trunc * sxy_m)); the window
    is part of the model, so the maps are not bit-identical with pydensecrf's.  --crf_pairwise lattice runs the CRFs on
    permutohedral lattices instead (pydensecrf's own approximation, cost independent of the bilateral width; a different model,
    pinned against a numpy restatement, not against pydensecrf itself); the default is window;
  * JPEG decode and np.load run on --num_workers host threads ahead of the device, the PNGs are written by one writer thread
    behind a bounded queue (drained, and a write error re-raised, before the script exits); one workspace is kept per image size
    and only the label map is read back per image;
  * every name is checked first: an image whose dict is missing or empty is named, and nothing is written.
"""
from __future__ import annotations

import argparse
import os
import sys
import types
from typing import List, Optional

import numpy as np


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.cam_to_ir_label", description=__doc__.split("\n")[0])
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--infer_list", default="data/train_aug.txt", type=str)
    ap.add_argument("--cam_dir", required=True, type=str, help="the <out_npy>_sgc directory of infer_mcl: <name>.npy dicts")
    ap.add_argument("--ir_label_out_dir", required=True, type=str)
    ap.add_argument("--conf_fg_thres", default=0.30, type=float)
    ap.add_argument("--conf_bg_thres", default=0.05, type=float)
    ap.add_argument("--crf_trunc", default=4.0, type=float, help="window half-width R_m = ceil(trunc * sxy_m); <= 0: all pairs")
    ap.add_argument("--crf_pairwise", default="window", choices=("window", "lattice"),
                    help="exact windowed sums, or the permutohedral lattice (--crf_trunc is ignored)")
    ap.add_argument("--num_workers", default=4, type=int, help="host threads that decode JPEGs and load dicts ahead of the device")
    return ap.parse_args(argv)


def save_png(path: str, conf: np.ndarray) -> None:
    import PIL.Image
    PIL.Image.fromarray(conf, "L").save(path)


def load_item(voc12_root: str, cam_dir: str, name: str):
    """(name, img uint8 [H,W,3], cam dict) on a host thread."""
    import PIL.Image
    img = np.array(PIL.Image.open(os.path.join(voc12_root, "JPEGImages", name + ".jpg")).convert("RGB"))
    cam_dict = np.load(os.path.join(cam_dir, name + ".npy"), allow_pickle=True).item()
    return name, img, cam_dict


def check_dicts(cam_dir: str, names: List[str]) -> List[str]:
    """The names whose dict is missing or empty."""
    bad = []
    for name in names:
        path = os.path.join(cam_dir, name + ".npy")
        if not os.path.exists(path) or len(np.load(path, allow_pickle=True).item()) == 0:
            bad.append(name)
    return bad


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    from concurrent.futures import ThreadPoolExecutor
    from muscle_amd.infer_mcl import NpyWriter
    from muscle_amd.infer_seg import read_names
    from muscle_amd.ir_label import cam_to_ir_label

    names = read_names(args.infer_list)
    bad = check_dicts(args.cam_dir, names)
    if bad:
        print(f"[muscle_amd] {len(bad)} image(s) of {args.infer_list} have a missing or empty CAM dict in {args.cam_dir}: "
              + " ".join(bad[:20]) + (" ..." if len(bad) > 20 else ""), file=sys.stderr)
        return 1
    os.makedirs(args.ir_label_out_dir, exist_ok=True)

    workers = max(1, args.num_workers)
    writer = NpyWriter(save=save_png)
    try:
        with ThreadPoolExecutor(max_workers=workers) as pool:
            ahead = 2 * workers
            pending = [pool.submit(load_item, args.voc12_root, args.cam_dir, n) for n in names[:ahead]]
            for it in range(len(names)):
                name, img, cam_dict = pending[it].result()
                pending[it] = None
                if it + ahead < len(names):
                    pending.append(pool.submit(load_item, args.voc12_root, args.cam_dir, names[it + ahead]))
                conf = cam_to_ir_label(img, cam_dict, conf_fg_thres=args.conf_fg_thres, conf_bg_thres=args.conf_bg_thres,
                                       trunc=args.crf_trunc, pairwise=args.crf_pairwise)
                writer.put(os.path.join(args.ir_label_out_dir, name + ".png"), conf.cpu().numpy())
                print(name, it, flush=True)
    finally:
        writer.close()
    return 0


class _CallableModule(types.ModuleType):
    """Importing this script binds `muscle_amd.cam_to_ir_label` to the module, over the function of that name that the package
    exports; calling the module is calling the function, so the public name means the same before and after."""

    def __call__(self, *args, **kwargs):
        from muscle_amd.ir_label import cam_to_ir_label
        return cam_to_ir_label(*args, **kwargs)


sys.modules[__name__].__class__ = _CallableModule

if __name__ == "__main__":
    sys.exit(main())
