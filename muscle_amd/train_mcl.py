"""`python -m muscle_amd.train_mcl`: the reference's train_mcl.py (multi-scale contrastive CAM training, :71-320) on the HIP
path.  Same arguments, same files: `<session_name>/_<epoch>.pth` after every epoch, then the rapid evaluation whose best
mIoU steps ReduceLROnPlateau.

Differences a caller can see:
  * the input path runs on the device (`muscle_amd.data`): DataLoader workers decode and plan, the GPU resizes, jitters,
    crops and erases; the loop body is `muscle_amd.mcl_step`, the optimiser `FusedAdam`;
  * --pretrained (new, default b3: the backbone the reference hard-codes at :94) and --eval_list (new, default
    data/train.txt: the list hard-coded at :117 and :306);
  * --start_epoch (new, default 0): the loop runs range(start_epoch, max_epoches), so a run continued from
    `--weights <session>/_7.pth --start_epoch 8` enters the PixPro / EMD epoch gates where it left off.  The reference
    saves no optimiser state: the learning rate and Adam's moments start afresh;
  * the rapid evaluation counts on the device (`RapidEval`): no training_eval/*.npy files are written;
  * --eval_batch N (new, default 1): images of one size share a forward of the rapid evaluation; the same table;
  * --tblog_dir is created and otherwise unused: the JET overlays of :256-277 are not built (no tensorboardX, no cv2).
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
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.train_mcl", description=__doc__.split("\n")[0])
    ap.add_argument("--batch_size", default=16, type=int)
    ap.add_argument("--max_epoches", default=16, type=int)
    ap.add_argument("--lr", default=1e-4, type=float)
    ap.add_argument("--num_workers", default=8, type=int)
    ap.add_argument("--wt_dec", default=5e-5, type=float)
    ap.add_argument("--train_list", default="data/train_aug.txt", type=str)
    ap.add_argument("--eval_list", default="data/train.txt", type=str, help="images of the per-epoch rapid evaluation")
    ap.add_argument("--num_classes", default=21, type=int)
    ap.add_argument("--session_name", default="runs/EffSeg_mcl", type=str)
    ap.add_argument("--crop_size", default=448, type=int)
    ap.add_argument("--weights", default=None, type=str)
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--tblog_dir", default="logs/tblog_mcl", type=str, help="created; nothing is written to it")
    ap.add_argument("--seed", default=0, type=int)
    ap.add_argument("--pretrained", default="b3", type=str)
    ap.add_argument("--start_epoch", default=0, type=int,
                    help="first epoch of range(start_epoch, max_epoches): continue a run from --weights <session>/_<N-1>.pth "
                         "--start_epoch N with the epoch gates (IMC 4, PixPro 8, EMD 12) where it left off; no optimiser "
                         "state is saved, so the learning rate and Adam's moments restart")
    ap.add_argument("--eval_batch", default=1, type=int,
                    help="images per forward of the rapid evaluation (1..8): 1 = one image per forward; above 1 images of one "
                         "size share a forward and the files of the next batch are decoded on host threads.  Same table")
    args = ap.parse_args(argv)
    if not 1 <= args.eval_batch <= 8:
        ap.error(f"--eval_batch {args.eval_batch} outside 1..8")
    if not 0 <= args.start_epoch <= args.max_epoches:
        ap.error(f"--start_epoch {args.start_epoch} outside 0..--max_epoches {args.max_epoches}")
    return args


def rapid_eval(model, names, labels, voc12_root: str, dev, num_cls: int = 21, batch: int = 1):
    """train_mcl.py:286-315 over the images `names`: (max_miou, max_t).  Leaves the model in eval mode."""
    from muscle_amd.evaluation import rapid_eval_sweep
    max_miou, max_t, _ = rapid_eval_sweep(model, names, voc12_root, labels, dev, batch=batch, num_cls=num_cls).best()
    return max_miou, max_t


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import torch
    import muscle_amd
    from muscle_amd.data import StagedLoader, VOC12ClsPix
    from muscle_amd.infer_seg import read_names

    print(vars(args))
    if args.seed:                                                                           # train_mcl.py:89-92
        random.seed(args.seed)
        np.random.seed(args.seed)
        torch.manual_seed(args.seed)
    dev = torch.device("cuda:0")
    model = muscle_amd.MuSCLe(num_classes=args.num_classes, pretrained="efficientnet-" + args.pretrained, layers=3,
                              MemoryEfficient=True, last_pooling=False)
    os.makedirs(args.tblog_dir, exist_ok=True)
    os.makedirs(args.session_name, exist_ok=True)
    train_dataset = VOC12ClsPix(args.train_list, args.voc12_root, crop_size=args.crop_size)  # :105-115
    if train_dataset.labels is None:
        raise FileNotFoundError("data/cls_labels.npy (the image-level labels, src/data.py:53-56) not found")
    eval_names = read_names(args.eval_list)
    loader = StagedLoader(train_dataset, args.batch_size, dev, num_workers=args.num_workers, shuffle=True, drop_last=True)
    max_step = len(train_dataset) // args.batch_size * args.max_epoches
    if args.weights:
        model.load_state_dict(torch.load(args.weights, map_location="cpu"), strict=False)   # :138-140
    model = model.to(dev)
    optimizer = muscle_amd.FusedAdam(model.parameters(), lr=args.lr, weight_decay=args.wt_dec)
    scheduler = torch.optim.lr_scheduler.ReduceLROnPlateau(optimizer, "max", patience=0, cooldown=0, factor=0.5, min_lr=1e-5)
    start = stage_start = time.time()
    print("Session started: ", time.ctime(start))
    for ep in range(args.start_epoch, args.max_epoches):
        for it, (_names, batch) in enumerate(loader):
            # :178 reads label.sum() back from the device every iteration; the loader still has the labels on the host
            out = muscle_amd.mcl_step(model, optimizer, batch, ep, valid_channel=int(loader.host_label_sum))
            if it % 25 == 0:                                                                # :234-254
                elapsed = time.time() - start
                est_finish = int(start + elapsed / (it / max_step + 1))
                print("Iter:%5d/%5d" % (it + max_step // args.max_epoches * ep, max_step),
                      "loss_focal:%.4f" % (float(out["loss_focal"])),
                      "loss_softmargin:%.4f" % (float(out["loss_softmargin"])),
                      "loss_pair:%.4f" % (float(out["loss_pair"])),
                      "loss_er:%.4f" % (float(out["loss_er"])),
                      "loss_imc:%.4f" % (float(out["loss_imc"])),
                      "loss_pixc:%.4f" % (float(out["loss_pixpro"])),
                      "loss_emd:%.4f" % (float(out["loss_emd"])),
                      "imps:%.1f" % ((it + 1) * args.batch_size / (time.time() - stage_start)),
                      "Fin:%s" % (time.ctime(est_finish)),
                      "lr: %.7f" % (optimizer.param_groups[0]["lr"]), flush=True)
        else:
            print("")
        torch.save(model.state_dict(), os.path.join(args.session_name, "_{}".format(str(ep)) + ".pth"))   # :283
        stamp = time.time()                                                                 # :286-318
        max_miou, max_t = rapid_eval(model, eval_names, train_dataset.labels, args.voc12_root, dev, args.num_classes,
                                     batch=args.eval_batch)
        print(f"\n Epoch:{ep} max miou:{max_miou} max t:{max_t}", f"Time elapse:{time.time() - stamp}s", flush=True)
        scheduler.step(max_miou)
        stage_start = time.time()
    return 0


if __name__ == "__main__":
    sys.exit(main())
