"""`python -m muscle_amd.infer_mcl`: the reference's infer_mcl.py (multi-scale CAM generation, :62-205) on the HIP path.
Same arguments, same output files: one `{class: float32[H,W]}` dict per image of --infer_list under `<out_npy>_sgc/`.

Differences a caller can see:
  * the multi-scale / flip list is built on the device (`MSFStager`) and the post-processing of all eight passes is one
    kernel over the channels of the image's labels (`infer.infer_cam_fused`); the maps are bit-equal to `infer.infer_cam`'s;
  * --out_cam_npy DIR (new, optional): also writes the raw-CAM dicts the reference has commented out at :181.  Without it
    the CAM map is not computed at all;
  * --pretrained (new, default b3: the backbone hard-coded at :75);
  * --pamr_iters N [--pamr_dilations 1 2 4 8 12 24] (new, default 0 = off): every saved map is refined on the device by N
    iterations of pixel-adaptive mask refinement against the image (muscle_amd/pamr.py) and min-max normalised once more, so it
    still spans [0,1]; the affinity is computed once per image.  Parity with the published PAMR code unpinned, effect on mIoU
    unmeasured;
  * the files are written by one writer thread behind a bounded queue, so np.save does not hold up the next image's
    forwards; the queue is drained, and a write error re-raised, before the script exits;
  * --num_workers and --tblog are accepted and unused (no tensorboardX overlays, no tqdm bar; `name iter` is printed).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np

DEFAULT_SCALES = (0.5, 1, 1.5, 2)                          # infer_mcl.py:89


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.infer_mcl", description=__doc__.split("\n")[0])
    ap.add_argument("--weights", required=True, type=str, help="MCL weights: a .ckpt with 'state_dict' or a state dict")
    ap.add_argument("--infer_list", default="../data/VOC2012/train.txt", type=str)
    ap.add_argument("--num_workers", default=8, type=int, help="unused")
    ap.add_argument("--num_classes", default=21, type=int)
    ap.add_argument("--tblog", default=None, type=str, help="unused")
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--out_npy", default=None, type=str, help="the SGC dicts go to <out_npy>_sgc/<name>.npy")
    ap.add_argument("--out_cam_npy", default=None, type=str, help="directory for the raw-CAM dicts (not computed without it)")
    ap.add_argument("--pretrained", default="b3", type=str)
    add_pamr_arguments(ap, "every saved map")
    args = ap.parse_args(argv)
    check_pamr_arguments(ap, args)
    return args


def add_pamr_arguments(ap: argparse.ArgumentParser, what: str) -> None:
    """--pamr_iters / --pamr_dilations, shared with muscle_amd.infer_seg."""
    ap.add_argument("--pamr_iters", default=0, type=int,
                    help=f"pixel-adaptive mask refinement (muscle_amd/pamr.py) of {what} against the image: iterations (0: off)")
    ap.add_argument("--pamr_dilations", default=[1, 2, 4, 8, 12, 24], type=int, nargs="+",
                    help="--pamr_iters > 0: the dilations of the 8-neighbour stencil (1..8 values in 1..64)")


def check_pamr_arguments(ap: argparse.ArgumentParser, args) -> None:
    from muscle_amd.pamr import check_dilations
    if args.pamr_iters < 0:
        ap.error(f"--pamr_iters {args.pamr_iters}: the number of PAMR iterations cannot be negative (0 runs none)")
    try:
        args.pamr_dilations = list(check_dilations(args.pamr_dilations))
    except ValueError as e:
        ap.error(f"--pamr_dilations: {e}")


class NpyWriter:
    """np.save on one thread behind a bounded queue.  put() blocks only when `depth` files are pending; close() drains the
    queue, joins the thread and re-raises the first error a write met (put() does too, so a full disk ends the run early)."""

    def __init__(self, depth: int = 16, save=np.save):
        import queue
        import threading
        self._q = queue.Queue(maxsize=depth)
        self._err: Optional[BaseException] = None
        self._save = save                                      # (path, object) -> None; np.save here, a PNG writer elsewhere
        self._t = threading.Thread(target=self._run, name="npy-writer", daemon=True)
        self._t.start()

    def _run(self) -> None:
        while True:
            job = self._q.get()
            try:
                if job is None:
                    return
                if self._err is None:
                    self._save(job[0], job[1])
            except BaseException as e:  # noqa: BLE001  (handed to the main thread)
                self._err = e
            finally:
                self._q.task_done()

    def put(self, path: str, obj) -> None:
        if self._err is not None:
            self.close()
        self._q.put((path, obj))

    def close(self) -> None:
        if self._t.is_alive():
            self._q.put(None)
            self._t.join()
        if self._err is not None:
            err, self._err = self._err, None
            raise err


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import PIL.Image
    import torch
    import muscle_amd
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_cam_fused
    from muscle_amd.infer_seg import load_weights, read_names

    dev = torch.device("cuda:0")
    model = muscle_amd.MuSCLe(num_classes=args.num_classes, pretrained="efficientnet-" + args.pretrained, layers=3,
                              MemoryEfficient=True, last_pooling=False)
    load_weights(model, args.weights)                                                       # :76-79
    model = model.to(dev).eval()
    labels = np.load("data/cls_labels.npy", allow_pickle=True).item()                       # src/data.py:54-57
    stager = MSFStager(dev)
    if args.out_npy is not None:
        os.makedirs(args.out_npy + "_sgc", exist_ok=True)                                   # :104-105
    if args.out_cam_npy is not None:
        os.makedirs(args.out_cam_npy, exist_ok=True)
    want_cam, want_sgc = args.out_cam_npy is not None, args.out_npy is not None
    pamr = muscle_amd.PAMR(args.pamr_iters, args.pamr_dilations) if args.pamr_iters > 0 else None
    writer = NpyWriter()
    try:
        for it, name in enumerate(read_names(args.infer_list)):
            img = PIL.Image.open(os.path.join(args.voc12_root, "JPEGImages", name + ".jpg")).convert("RGB")
            W, H = img.size
            label = torch.from_numpy(np.asarray(labels[name], dtype=np.float32)).view(1, -1)
            cam_dict, sgc_dict, _score = infer_cam_fused(model, stager(img, DEFAULT_SCALES), label, H, W, want_cam=want_cam,
                                                         want_sgc=want_sgc, pamr=pamr,
                                                         pamr_img=np.asarray(img, dtype=np.uint8) if pamr is not None else None)
            if want_cam:
                writer.put(os.path.join(args.out_cam_npy, name + ".npy"), cam_dict)
            if want_sgc:
                writer.put(os.path.join(args.out_npy + "_sgc", name + ".npy"), sgc_dict)        # :182
            print(name, it, flush=True)
    finally:
        writer.close()
    return 0


if __name__ == "__main__":
    sys.exit(main())
