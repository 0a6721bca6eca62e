"""`python -m muscle_amd.infer_irn`: the reference's infer_irn.py (IRN boundary map + random walk -> pseudo labels) on the
HIP path.  Same arguments, same output files: `<sem_seg_out_dir>_png/<name>.png`, the label map as a palette PNG with the VOC
colour map, and with --soft_output 1 instead `<sem_seg_out_dir>/<name>.npy`, float16 [H,W,21].
--soft_output 2 (not in the reference) writes the compact form of that array, `<sem_seg_out_dir>/<name>.npz`
(muscle_amd/softlabel.py: the walk maps of the present classes, 47 KB per class at 375x500 instead of 7.9 MB), which
`train_muscle --mask_root` reads and `python -m muscle_amd.softlabel unpack` turns into the .npy bit for bit.

Differences a caller can see:
  * --irn_network is accepted and ignored: the one network the reference ships (src.backbones.resnet50_irn) is built in;
  * nothing is downloaded: --irn_weights_name must name a checkpoint (the reference fetches ImageNet weights first and then
    overwrites them with the checkpoint);
  * --walk stencil (not in the reference) runs the random walk matrix-free; the default, dense, is the reference's way;
  * --ins_seg_out_dir DIR (not in the reference: IRN's published make_ins_seg_labels step) also writes the instance
    pseudo-label `DIR/<name>.npy`, the dict {'score' [n], 'mask' bool [n,H,W], 'class' [n]} of muscle_amd/ins_seg.py, from
    the same network forward; --walk applies to both walks.  Without the flag nothing changes.
  * --ins_eval 1 (needs --ins_seg_out_dir; IRN's published eval_ins_seg step) also evaluates every instance label as it is made,
    from its seg_map on the device against SegmentationClass/ and SegmentationObject/ under --voc12_root, and prints the lines of
    `python -m muscle_amd.ins_eval` at the end (muscle_amd/ins_eval.py).  Off by default; the files written are the same.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional

import numpy as np


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.infer_irn", description=__doc__.split("\n")[0])
    ap.add_argument("--beta", default=8, type=int)
    ap.add_argument("--exp_times", default=6, type=int, help="the random walk is performed 2^exp_times times")
    ap.add_argument("--sem_seg_bg_thres", default=0.35, type=float)
    ap.add_argument("--irn_network", default="src.backbones.resnet50_irn", type=str, help="ignored (see the note)")
    ap.add_argument("--irn_weights_name", required=True, type=str, help="IRN checkpoint (a state dict)")
    ap.add_argument("--cam_dir", required=True, type=str)
    ap.add_argument("--sem_seg_out_dir", default="./irn_rw", type=str)
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--infer_list", default="data/train.txt", type=str)
    ap.add_argument("--soft_output", default=0, type=int,
                    help="1: write float16 soft pseudo labels <name>.npy instead of the PNG; 2: their compact form <name>.npz")
    ap.add_argument("--walk", default="dense", choices=("dense", "stencil"),
                    help="the random walk: dense = exp_times squarings of the n x n transition matrix (the reference's way), "
                         "stencil = 2^exp_times matrix-free steps on an fp64 state (O(n) memory)")
    ap.add_argument("--ins_seg_out_dir", default=None, type=str,
                    help="also write instance pseudo-labels <name>.npy here (muscle_amd/ins_seg.py); off by default")
    ap.add_argument("--ins_seg_bg_thres", default=0.25, type=float)
    ap.add_argument("--ins_refine_iters", default=300, type=int, help="centroid refinement iterations of the instance path")
    ap.add_argument("--ins_dp_thres", default=2.5, type=float, help="displacement magnitude below which a pixel seeds an instance")
    ap.add_argument("--ins_eval", default=0, type=int,
                    help="1: also evaluate the instance labels (VOC AP^r, muscle_amd/ins_eval.py) and print the result at the end")
    ap.add_argument("--ins_eval_iou", default=[0.25, 0.5, 0.7, 0.75], type=float, nargs="+", help="IoU thresholds of --ins_eval")
    args = ap.parse_args(argv)
    if args.ins_eval and not args.ins_seg_out_dir:
        ap.error("--ins_eval 1 evaluates the instance labels: it needs --ins_seg_out_dir")
    if args.irn_network != ap.get_default("irn_network"):
        print(f"[muscle_amd] note: --irn_network {args.irn_network} ignored; the ResNet-50 IRN is the one network built here",
              file=sys.stderr)
    return args


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import PIL.Image
    import torch
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import load_cam_dict
    from muscle_amd.infer_seg import read_names
    from muscle_amd.irn import EdgeDisplacement, infer_irn, save_palette_png
    from muscle_amd.softlabel import save_compact

    dev = torch.device("cuda:0")
    model = EdgeDisplacement()
    model.load_state_dict(torch.load(args.irn_weights_name, map_location="cpu"), strict=False)        # infer_irn.py:41
    model = model.to(dev).eval()
    stager = MSFStager(dev)
    if args.soft_output:
        os.makedirs(args.sem_seg_out_dir, exist_ok=True)
    os.makedirs(args.sem_seg_out_dir + "_png", exist_ok=True)
    ins_kw = None
    if args.ins_seg_out_dir:
        from muscle_amd.ins_seg import save_instances, warn_all_zero
        os.makedirs(args.ins_seg_out_dir, exist_ok=True)
        ins_kw = dict(bg_thres=args.ins_seg_bg_thres, iterations=args.ins_refine_iters, dp_thres=args.ins_dp_thres)
    ins_ev = None
    if args.ins_eval:
        from muscle_amd.ins_eval import InsSegEval, check_gt_files, read_gt_pngs
        check_gt_files(args.voc12_root, list(read_names(args.infer_list)))
        ins_ev = InsSegEval(dev, iou_thresholds=args.ins_eval_iou)
    for it, name in enumerate(read_names(args.infer_list)):
        img = PIL.Image.open(os.path.join(args.voc12_root, "JPEGImages", name + ".jpg")).convert("RGB")
        pair = torch.cat(stager(img, (1.0,)), dim=0)                                                 # image + flip, color_norm'ed
        cam = load_cam_dict(os.path.join(args.cam_dir, name + ".npy"))
        res = infer_irn(model, pair, cam, beta=args.beta, exp_times=args.exp_times, bg_thres=args.sem_seg_bg_thres,
                        soft_output="compact" if args.soft_output == 2 else bool(args.soft_output), method=args.walk, ins_seg=ins_kw)
        if ins_kw is not None:
            res, ins = res
            if ins.vmax == 0:
                warn_all_zero(name)
            save_instances(os.path.join(args.ins_seg_out_dir, name + ".npy"), ins)
            if ins_ev is not None:
                ins_ev.add(ins, *read_gt_pngs(args.voc12_root, name))
        if args.soft_output == 2:
            if res[1].vmax > 0:
                save_compact(os.path.join(args.sem_seg_out_dir, name + ".npz"), res[1])
            else:                                                # all-zero walk result: the dense array would be 0 / 0
                print(f"[muscle_amd] {name}: the walk result is all zero, no soft label written", file=sys.stderr)
        elif args.soft_output:
            np.save(os.path.join(args.sem_seg_out_dir, name + ".npy"), res[1].cpu().numpy())
        else:
            save_palette_png(os.path.join(args.sem_seg_out_dir + "_png", name + ".png"), res)
        print(name, it, flush=True)
    if ins_ev is not None:
        for line in ins_ev.lines():
            print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
