"""`python -m muscle_amd.train_muscle`: the reference's train_muscle.py (decoder training on soft pseudo-labels) on the HIP
path.  Same arguments, same files: `<session_name>/_<epoch>.pth` after every epoch.

Differences a caller can see:
  * the input path runs on the device (`muscle_amd.segdata`): DataLoader workers decode and plan, the GPU resizes, crops and
    flips image and label; --mask_root holds what `python -m muscle_amd.infer_irn --soft_output 1` writes (<name>.npy) or
    its compact form (--soft_output 2, <name>.npz), chosen by --mask_format (new; auto: the .npy where it exists, else the
    .npz); the compact form is expanded on the device to the same float16 rows, bit for bit;
  * --mask_type label (new; default soft): --mask_root holds label maps <name>.png instead - what `infer_irn --soft_output 0`
    and `infer_seg --out_seg` write, or SegmentationClass[Aug] itself; 255 is ignored by the loss, the resize is NEAREST and
    the crop padding is 255 (muscle_amd/segdata.py);
  * --val_list (new, default data/val.txt: the list the reference hard-codes) names the images of the per-epoch validation;
  * --crf 1 runs the dense CRF of the validation on the GPU with t=1 (the exact windowed CRF of muscle_amd/crf.py, not
    pydensecrf's lattice filter);
  * --val_batch N (new, default 1): images of one size share a forward of the validation; the same table;
  * --val_boundary 1 (new, default 0): one more line per epoch after the mIoU, the Boundary mIoU and the trimap mIoU at
    d = 1, 2, 4, 8 of the validation's predictions (evaluation.BoundaryEval); the mIoU and the schedule are untouched;
  * --energy_weight W (new, default 0: off) adds W times the dense-CRF energy loss of muscle_amd/crf_loss.py (ours, not the
    reference's) to the loss, with --energy_sxy / --energy_srgb / --energy_scale / --energy_trunc; the progress line gains
    loss_energy.  It reaches the pixels a label map ignores (255) inside the crop window;
  * --beacon_sampler device (new; default host: the reference's `random.sample` draws on the host) takes BEACON's boundary
    points on the GPU (edge.FieldLoss(sampler="device"), seeded by --seed): the step then has no host synchronisation, and
    --graph 1 (new, default 0; needs --beacon_sampler device, refuses --energy_weight > 0 and --lovasz_weight > 0) replays it
    as a hipGraph (muscle_amd.GraphedMuscleStep);
  * --lovasz_weight W (new, default 0: off; needs --mask_type label, refuses --graph 1) adds W times the Lovasz-softmax loss of
    muscle_amd/lovasz.py (ours, not the reference's: Berman et al. 2018, a surrogate of the mIoU the validation reports) to the
    loss, with --lovasz_classes present|all and --lovasz_per_image 0|1; the progress line gains loss_lovasz;
  * --tblog_dir is created and otherwise unused (the reference opens a tensorboardX writer and never writes to it).
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from typing import List, Optional

import numpy as np


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.train_muscle", description=__doc__.split("\n")[0])
    ap.add_argument("--batch_size", default=6, type=int)
    ap.add_argument("--max_epoches", default=8, type=int)
    ap.add_argument("--lr", default=1e-5, type=float)
    ap.add_argument("--num_workers", default=8, type=int)
    ap.add_argument("--wt_dec", default=1e-5, type=float)
    ap.add_argument("--train_list", default="data/VOC2012/train_aug.txt", type=str)
    ap.add_argument("--val_list", default="data/val.txt", type=str, help="images of the per-epoch validation")
    ap.add_argument("--num_classes", default=21, type=int)
    ap.add_argument("--session_name", default="runs/muscle", type=str)
    ap.add_argument("--crop_size", default=448, type=int)
    ap.add_argument("--weights", default=None, type=str)
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--mask_root", required=True, type=str, help="directory of soft pseudo-labels <name>.npy, [H,W,21]")
    ap.add_argument("--mask_format", default="auto", choices=("auto", "dense", "compact"),
                    help="dense: <name>.npy; compact: <name>.npz (infer_irn --soft_output 2); auto: the .npy where it exists, "
                         "else the .npz")
    ap.add_argument("--mask_type", default="soft", choices=("soft", "label"),
                    help="soft: the soft pseudo-labels above; label: --mask_root holds label maps <name>.png (one class index "
                         "per pixel, 255 = ignore)")
    ap.add_argument("--k", default=128, type=int)
    ap.add_argument("--step", default=7, type=int)
    ap.add_argument("--lamb", default=5e-2, type=float)
    ap.add_argument("--tblog_dir", default="logs/tblog_muscle", type=str, help="created; nothing is written to it")
    ap.add_argument("--cls_dir", default=None, type=str, help="per-image class scores <name>.npy for the validation")
    ap.add_argument("--crf", default=0, type=int,
                    help="1: dense CRF (t=1) in the validation, on the GPU with exact windowed kernels (not pydensecrf)")
    ap.add_argument("--seed", default=221, type=int)
    ap.add_argument("--pretrained", default="b7", type=str)
    ap.add_argument("--bifpn", default=3, type=int)
    ap.add_argument("--val_batch", default=1, type=int,
                    help="images per forward of the validation (1..8): 1 = one image per forward; above 1 images of one size "
                         "share a forward and the files of the next batch are decoded on host threads.  Same table")
    ap.add_argument("--val_boundary", default=0, type=int, choices=(0, 1),
                    help="1: after each epoch's mIoU, one line with the Boundary mIoU and the trimap mIoU at d = 1, 2, 4, 8 "
                         "of the same predictions (evaluation.BoundaryEval)")
    ap.add_argument("--energy_weight", default=0.0, type=float,
                    help="weight of the dense-CRF energy loss (muscle_amd/crf_loss.py; ours, not the reference's); 0: off")
    ap.add_argument("--energy_sxy", default=80.0, type=float, help="its spatial width in full-resolution pixels")
    ap.add_argument("--energy_srgb", default=15.0, type=float, help="its colour width")
    ap.add_argument("--energy_scale", default=4, type=int, choices=(1, 2, 4, 8), help="its pooling factor (crop_size % scale == 0)")
    ap.add_argument("--energy_trunc", default=2.0, type=float, help="its window: ceil(trunc * sxy / scale) cells; <= 0: all pairs")
    ap.add_argument("--lovasz_weight", default=0.0, type=float,
                    help="weight of the Lovasz-softmax loss (muscle_amd/lovasz.py; ours, not the reference's); 0: off; needs "
                         "--mask_type label")
    ap.add_argument("--lovasz_classes", default="present", choices=("present", "all"),
                    help="present: average over the classes that occur among the labelled pixels; all: over every class")
    ap.add_argument("--lovasz_per_image", default=0, type=int, choices=(0, 1), help="1: one Lovasz term per image, averaged")
    ap.add_argument("--beacon_sampler", default="host", choices=("host", "device"),
                    help="host: BEACON's boundary points by Python's random.sample, as the reference draws them; device: a keyed "
                         "k-subset taken on the GPU (seed: --seed), no host synchronisation in the step")
    ap.add_argument("--graph", default=0, type=int, choices=(0, 1),
                    help="1: replay the training step as a hipGraph (needs --beacon_sampler device; not with --energy_weight > 0 or "
                         "--lovasz_weight > 0)")
    args = ap.parse_args(argv)
    if args.graph and args.beacon_sampler != "device":
        ap.error("--graph 1 needs --beacon_sampler device (the host sampler reads the point counts back every step)")
    if args.graph and args.energy_weight > 0:
        ap.error("--graph 1 does not capture the energy loss (--energy_weight must be 0)")
    if args.lovasz_weight < 0:
        ap.error(f"--lovasz_weight {args.lovasz_weight} is negative")
    if args.lovasz_weight > 0 and args.mask_type != "label":
        ap.error("--lovasz_weight > 0 needs --mask_type label (the Lovasz-softmax loss is defined on label maps)")
    if args.graph and args.lovasz_weight > 0:
        ap.error("--graph 1 does not capture the Lovasz-softmax loss (--lovasz_weight must be 0)")
    if not 1 <= args.val_batch <= 8:
        ap.error(f"--val_batch {args.val_batch} outside 1..8")
    if args.energy_weight < 0:
        ap.error(f"--energy_weight {args.energy_weight} is negative")
    if args.energy_weight > 0 and args.crop_size % args.energy_scale:
        ap.error(f"--crop_size {args.crop_size} is not a multiple of --energy_scale {args.energy_scale}")
    return args


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import torch
    import muscle_amd
    from muscle_amd import edge
    from muscle_amd.evaluation import BoundaryEval, validate_seg
    from muscle_amd.infer_seg import read_names
    from muscle_amd.segdata import SegLoader, VOC12SegDataset

    print(vars(args))
    if args.seed:                                                                           # train_muscle.py:103-106
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    dev = torch.device("cuda:0")
    model = muscle_amd.MuSCLe(num_classes=args.num_classes, pretrained="efficientnet-" + args.pretrained, layers=args.bifpn,
                              MemoryEfficient=True, mode="dec", last_pooling=True)
    os.makedirs(args.tblog_dir, exist_ok=True)
    os.makedirs(args.session_name, exist_ok=True)
    train_dataset = VOC12SegDataset(args.train_list, args.voc12_root, args.mask_root, min_scale=0.5, max_scale=1.75,
                                    crop_size=args.crop_size, mask_type=args.mask_type,
                                    mask_format=args.mask_format, num_classes=args.num_classes)   # :119-125
    if train_dataset.labels is None:
        raise FileNotFoundError("data/cls_labels.npy (the image-level labels, src/data.py:53-56) not found")
    loader = SegLoader(train_dataset, args.batch_size, dev, num_workers=args.num_workers, shuffle=True, drop_last=True,
                       prefetch_factor=4, windows=args.energy_weight > 0)                   # :128-130
    energy = None
    if args.energy_weight > 0:
        from muscle_amd.crf_loss import DenseEnergyLoss
        energy = DenseEnergyLoss(args.energy_sxy, args.energy_srgb, args.energy_scale, args.energy_trunc)
    lovasz = None
    if args.lovasz_weight > 0:
        lovasz = muscle_amd.LovaszSoftmaxLoss(args.lovasz_classes, bool(args.lovasz_per_image))
    val_names = read_names(args.val_list)
    max_step = len(train_dataset) // args.batch_size * args.max_epoches
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location="cpu"), strict=False)   # :153-155
    model = model.to(dev)
    optimizer = muscle_amd.FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wt_dec)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, "max", patience=0, cooldown=0, factor=0.5, min_lr=5e-6)
    criterion2 = edge.FieldLoss(sobel_size=5, beta=1e2, k=args.k, sampler=args.beacon_sampler, seed=args.seed)
    graphed = None
    if args.graph:
        graphed = muscle_amd.GraphedMuscleStep(model, optimizer, criterion2, lamb=args.lamb, step=args.step, k=args.k)
    start = stage_start = time.time()
    print("Session started: ", time.ctime(start))
    for ep in range(args.max_epoches):
        model.train()
        print("lr: %.6f" % (optimizer.param_groups[0]["lr"]))
        for it, (_names, batch) in enumerate(loader):
            if graphed is not None:
                out = graphed(batch)
            else:
                out = muscle_amd.muscle_step(model, optimizer, batch, lamb=args.lamb, step=args.step, k=args.k, criterion2=criterion2,
                                             energy=energy, energy_weight=args.energy_weight, lovasz=lovasz,
                                             lovasz_weight=args.lovasz_weight)
            if it % 25 == 0:                                                                # :210-218
                elapsed = time.time() - start
                est_finish = int(start + elapsed / (it / max_step + 1))
                print("Iter:%5d/%5d" % (it + max_step // args.max_epoches * ep, max_step),
                      "loss_seg:%.4f" % (float(out["loss_seg"])),
                      "loss_beacon:%.4f" % (float(out["loss_beacon"])),
                      *(("loss_energy:%.4f" % (float(out["loss_energy"])),) if "loss_energy" in out else ()),
                      *(("loss_lovasz:%.4f" % (float(out["loss_lovasz"])),) if "loss_lovasz" in out else ()),
                      "imps:%.1f" % ((it + 1) * args.batch_size / (time.time() - stage_start)),
                      "Fin:%s" % (time.ctime(est_finish)), flush=True)
        torch.save(model.state_dict(), os.path.join(args.session_name, "_{}".format(str(ep)) + ".pth"))
        stamp = time.time()                                                                 # :224-283
        bev = BoundaryEval(dev, args.num_classes) if args.val_boundary else None
        miou = validate_seg(model, val_names, args.voc12_root, dev, args.num_classes, cls_dir=args.cls_dir, crf=bool(args.crf),
                            batch=args.val_batch, boundary=bev)
        print(f"\n Epoch:{ep} val miou:{miou}", f"Time elapse:{time.time() - stamp}s", flush=True)
        if bev is not None:
            print(f" Epoch:{ep} val boundary miou:{bev.boundary_miou():.3f}%",
                  " ".join(f"trimap{d}:{bev.trimap_miou(d):.3f}%" for d in (1, 2, 4, 8)), flush=True)
        scheduler.step(miou)
        stage_start = time.time()
    return 0


if __name__ == "__main__":
    sys.exit(main())
