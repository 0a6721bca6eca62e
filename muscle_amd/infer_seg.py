"""`python -m muscle_amd.infer_seg`: the reference's infer_seg.py (semantic-segmentation inference of the trained decoder)
on the HIP path.  Same arguments, same output files: one 8-bit class-index PNG per image of --infer_list under --out_seg.

Differences a caller can see:
  * the dense CRF: --crf 2 [--crf_trunc 4.0] runs the reference's CRF model (imutils.crf_inference, t=4) on the GPU with
    its pairwise sums evaluated exactly over a square window (muscle_amd/crf.py).  --crf 1 in the reference means
    pydensecrf's lattice filter on the CPU, whose label maps are not reproduced bit for bit: it stays refused, with a
    message that points to --crf 2, and --crf defaults to 0 (the reference defaults to 1).  --crf 2 --crf_pairwise lattice
    runs the same model on permutohedral lattices instead (muscle_amd/lattice.py): pydensecrf's own approximation on the GPU,
    pinned against a numpy restatement of the algorithm, not against pydensecrf itself; the default is window;
  * --gt_dir (new, optional): the SegmentationClass directory; prints do_python_eval's IoU table for the written maps;
    with --boundary 1 (new, default 0) also the Boundary-IoU table and the trimap curve of evaluation.BoundaryEval;
  * --out_conf DIR (new, optional, with --out_seg): beside each label map the confidence code of its pixels, DIR/<name>.png
    (mode L), and DIR/stats.npz, the per-class code histograms - the inputs of `python -m muscle_amd.selflabel select`, which
    keeps the most confident portion of every class for a self-training round; with --gt_dir also the quality curve.  Refused
    with --cls_dir unless --crf 2 (a class-scaled mean map is no distribution).  Without it nothing changes;
  * --pamr_iters N [--pamr_dilations 1 2 4 8 12 24] (new, default 0 = off): the mean probability map is refined on the device by
    N iterations of pixel-adaptive mask refinement against the image (muscle_amd/pamr.py), the label map is the refined map's
    argmax and --out_conf sees the refined map.  An edge-aware option at a fraction of the CRF's cost; refused together with
    --crf 2.  Parity with the published PAMR code unpinned, effect on mIoU unmeasured;
  * --num_workers and --tblog are accepted and unused (the multi-scale list is built on the device, nothing is logged).
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np

DEFAULT_SCALES = (0.5, 0.75, 1, 1.25, 1.5, 1.75)          # infer_seg.py:75


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.infer_seg", description=__doc__.split("\n")[0])
    ap.add_argument("--weights", required=True, type=str, help="decoder weights: a .ckpt with 'state_dict' or a state dict")
    ap.add_argument("--infer_list", default="data/val.txt", type=str)
    ap.add_argument("--num_workers", default=8, type=int, help="unused")
    ap.add_argument("--num_classes", default=21, type=int)
    ap.add_argument("--tblog", default="logs/infer", type=str, help="unused")
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--cls_dir", default=None, type=str, help="per-image class scores <name>.npy scaling channels 1..K-1")
    ap.add_argument("--out_seg", default=None, type=str)
    ap.add_argument("--crf", default=0, type=int, help="0: none; 2: the dense CRF on the GPU, exact windowed kernels (1 = pydensecrf: refused)")
    ap.add_argument("--crf_trunc", default=4.0, type=float, help="--crf 2: window half-width in units of sxy (<= 0: all pairs)")
    ap.add_argument("--crf_pairwise", default="window", choices=("window", "lattice"),
                    help="--crf 2: exact windowed sums, or the permutohedral lattice (pydensecrf's approximation; --crf_trunc is ignored)")
    ap.add_argument("--bifpn", default=3, type=int)
    ap.add_argument("--pretrained", default="b7", type=str)
    ap.add_argument("--gt_dir", default=None, type=str, help="SegmentationClass directory: print the IoU table")
    ap.add_argument("--scales", default=",".join(str(s) for s in DEFAULT_SCALES), type=str)
    ap.add_argument("--boundary", default=0, type=int, choices=(0, 1),
                    help="--gt_dir, 1: after the IoU table, the Boundary-IoU table and the trimap curve (evaluation.BoundaryEval)")
    ap.add_argument("--out_conf", default=None, type=str,
                    help="with --out_seg: also write the confidence-code map <name>.png of every image and stats.npz, the "
                         "per-class histograms, here (muscle_amd.selflabel select turns them into self-training labels)")
    from muscle_amd.infer_mcl import add_pamr_arguments, check_pamr_arguments
    add_pamr_arguments(ap, "the mean probability map")
    args = ap.parse_args(argv)
    check_pamr_arguments(ap, args)
    if args.pamr_iters > 0 and args.crf != 0:
        ap.error("--pamr_iters with --crf: PAMR and the dense CRF are two refinements of the same map; choose one")
    if args.out_conf is not None and args.out_seg is None:
        ap.error("--out_conf writes the confidence of the --out_seg label maps: it needs --out_seg")
    if args.out_conf is not None and args.cls_dir and args.crf != 2:
        ap.error("--out_conf with --cls_dir needs --crf 2: a mean map whose channels are scaled by class scores is no "
                 "distribution, so its maximum is no confidence; the CRF's Q is one")
    if args.boundary and not args.gt_dir:
        ap.error("--boundary 1 compares against the ground truth: it needs --gt_dir")
    if args.crf not in (0, 2):
        ap.error(f"--crf {args.crf}: pydensecrf's lattice-filter CRF (--crf 1 of the reference, CPU) is not built on the HIP "
                 "path; --crf 2 runs the same CRF model with exact windowed kernels on the GPU (label maps close to, not "
                 "bit-identical with, pydensecrf's), --crf 0 runs none")
    return args


def load_weights(model, path: str):
    """infer_seg.py:67-70: a '.ckpt' file holds {'state_dict': ...}, anything else is the state dict; strict=False."""
    import torch
    sd = torch.load(path, map_location="cpu")
    if ".ckpt" in path:
        sd = sd["state_dict"]
    return model.load_state_dict(sd, strict=False)


def read_names(list_path: str) -> List[str]:
    """src/data.py:load_img_name_list."""
    return [ln.split(" ")[0].split("/")[-1].split(".")[0] for ln in open(list_path).read().splitlines()]


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import PIL.Image
    import torch
    import muscle_amd
    from muscle_amd.data import MSFStager
    from muscle_amd.evaluation import BoundaryEval, SegEval, categories
    from muscle_amd.infer import infer_seg, save_seg_png

    dev = torch.device("cuda:0")
    model = muscle_amd.MuSCLe(num_classes=args.num_classes, pretrained="efficientnet-" + args.pretrained, layers=args.bifpn,
                              MemoryEfficient=True, last_pooling=True, mode="dec")
    load_weights(model, args.weights)
    model = model.to(dev).eval()
    scales = tuple(float(s) for s in args.scales.split(","))
    stager = MSFStager(dev)
    pamr = muscle_amd.PAMR(args.pamr_iters, args.pamr_dilations) if args.pamr_iters > 0 else None
    ev = SegEval(dev, args.num_classes) if args.gt_dir else None
    bev = BoundaryEval(dev, args.num_classes) if args.boundary else None
    if args.out_seg is not None:
        os.makedirs(args.out_seg, exist_ok=True)
    stats = None
    if args.out_conf is not None:
        from muscle_amd.selflabel import ConfStats, curve_lines, quality_curve
        os.makedirs(args.out_conf, exist_ok=True)
        stats = ConfStats(dev, args.num_classes)
    for it, name in enumerate(read_names(args.infer_list)):
        img = PIL.Image.open(os.path.join(args.voc12_root, "JPEGImages", name + ".jpg")).convert("RGB")
        W, H = img.size
        cls = None
        if args.cls_dir:
            cls = np.load(os.path.join(args.cls_dir, name + ".npy"), allow_pickle=True).squeeze()
        crf_img = np.asarray(img, dtype=np.uint8) if args.crf == 2 else None                # infer_seg.py:128-129, t=4
        pamr_img = np.asarray(img, dtype=np.uint8) if pamr is not None else None
        pred, prob = infer_seg(model, stager(img, scales), H, W, cls_label=cls, crf_img=crf_img, crf_t=4, crf_trunc=args.crf_trunc,
                               crf_pairwise=args.crf_pairwise, return_prob=stats is not None, pamr=pamr, pamr_img=pamr_img)
        if args.out_seg is not None:
            save_seg_png(os.path.join(args.out_seg, name + ".png"), pred)
        if ev is not None:
            gt = np.array(PIL.Image.open(os.path.join(args.gt_dir, name + ".png")))
            gd = torch.from_numpy(gt).to(dev)
        if stats is not None:                             # the code of the map pred is the argmax of: the mean map, or the CRF's Q
            _, code = stats.add(prob, gd if ev is not None else None)
            save_seg_png(os.path.join(args.out_conf, name + ".png"), code)
        if ev is not None:
            ev.add(pred, gd)
            if bev is not None:
                bev.add(pred, gd)
        print(name, it, flush=True)
    if ev is not None:                                    # do_python_eval(printlog=True), src/evaluation.py:72-83
        log = ev.loglist()
        for i in range(args.num_classes):
            nm = categories[i] if i < len(categories) else str(i)
            print('%11s:%7.3f%%' % (nm, log[nm]), end='\t' if i % 2 != 1 else '\n')
        print('\n======================================================')
        print('%11s:%7.3f%%' % ('mIoU', log['mIoU']), flush=True)
    if bev is not None:
        print("\n".join(bev.lines()), flush=True)
    if stats is not None:
        stats.save(os.path.join(args.out_conf, "stats.npz"))
        if args.gt_dir:                                   # what each portion of muscle_amd.selflabel select would keep, and how right it is
            print("\n".join(curve_lines(quality_curve(*stats.tables(), [i / 10 for i in range(1, 11)]))), flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
