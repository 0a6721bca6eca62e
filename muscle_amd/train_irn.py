"""`python -m muscle_amd.train_irn`: training the IRN edge / displacement heads on the HIP path, the stage between
`infer_mcl` + IR labels and `infer_irn`.  The reference ships the model (src/backbones/resnet50_irn.py:143-212) and the dataset
(src/data.py:639-705) but no script; this is the public IRN training loop around them:

    AffinityDisplacementLoss(PathIndex(radius=10, (crop/4, crop/4))), PolyOptimizer over (edge heads x1 lr, displacement heads
    x10 lr), --irn_num_epoches epochs of irn_step, then one eval pass over the list that averages dp_out per image into
    mean_shift.running_mean, then torch.save(state_dict()) - a file `python -m muscle_amd.infer_irn --irn_weights_name` loads.

What a caller should know:
  * --backbone_weights names a ResNet-50 state dict (torchvision names, `conv1.weight` ...) or an IRN state dict
    (`resnet50.conv1.weight` ...); nothing is downloaded.  The backbone is frozen, as in the reference;
  * --ir_label_dir holds the IR label PNGs (0..20, 255 = ignore), one per name of --train_list; `python -m muscle_amd.cam_to_ir_label`
    writes them from the CAM dicts of `infer_mcl`;
  * the loader is the host-side restatement of VOC12AffinityDataset with PIL and numpy, draws in the reference's order; it ships
    the reduced uint8 label map [crop/4, crop/4], never the three [n_dst, n_src] float label tensors - the loss kernel derives
    the pair labels on the fly;
  * --loader device leaves only decoding and the draws to the workers and does the pixel work of both the training loop and
    the displacement-mean pass on the GPU (muscle_amd.irndata: mx_resample + mx_irn_input_stage); the tensors are the host
    loader's bit for bit, the host loader stays the default.
"""
from __future__ import annotations

import argparse
import os
import random
import sys
import time
from typing import List, Optional

import numpy as np

_MEAN, _STD = (0.485, 0.456, 0.406), (0.229, 0.224, 0.225)


# ---- src/imutils.py / src/data.py, restated for in-memory arrays -----------------------------------------------------------
def pil_rescale(img: np.ndarray, scale: float, order: int) -> np.ndarray:
    """src/imutils.py:55-69: PIL resize to round(h*scale) x round(w*scale), bicubic (order 3) or nearest (order 0)."""
    import PIL.Image
    h, w = img.shape[:2]
    th, tw = int(np.round(h * scale)), int(np.round(w * scale))
    if (th, tw) == (h, w):
        return img
    return np.asarray(PIL.Image.fromarray(img).resize((tw, th), PIL.Image.BICUBIC if order == 3 else PIL.Image.NEAREST))


def normalize(img: np.ndarray) -> np.ndarray:
    """TorchvisionNormalize, src/data.py:596-609: uint8 [H,W,3] -> float32."""
    out = np.empty(img.shape, np.float32)
    for c in range(3):
        out[..., c] = (img[..., c] / 255. - _MEAN[c]) / _STD[c]
    return out


def random_crop_box(h: int, w: int, crop: int, rng):
    """src/imutils.py:183-206 (the width is drawn before the height): `data.random_crop_box` in the reference's 8-value form."""
    from .data import random_crop_box as box
    cont_top, cont_left, img_top, img_left, ch, cw = box(h, w, crop, rng)
    return cont_top, cont_top + ch, cont_left, cont_left + cw, img_top, img_top + ch, img_left, img_left + cw


def affinity_sample(img: np.ndarray, label: np.ndarray, crop_size: int, rng=random, rescale=(0.5, 1.5)):
    """VOC12AffinityDataset.__getitem__ (src/data.py:659-705) for a decoded image uint8 [H,W,3] and its label uint8 [H,W]:
    random scale (one draw; bicubic / nearest), normalisation, flip (one bit), random crop with fills (0, 255) (two draws),
    the label reduced by 0.25 with nearest.  Returns (img float32 [3,crop,crop], label uint8 [crop/4,crop/4])."""
    s = rescale[0] + rng.random() * (rescale[1] - rescale[0])
    img, label = pil_rescale(img, s, 3), pil_rescale(label, s, 0)
    img = normalize(img)
    if bool(rng.getrandbits(1)):
        img, label = np.fliplr(img), np.fliplr(label)
    box = random_crop_box(img.shape[0], img.shape[1], crop_size, rng)
    ci = np.zeros((crop_size, crop_size, 3), np.float32)
    cl = np.full((crop_size, crop_size), 255, np.uint8)
    ci[box[0]:box[1], box[2]:box[3]] = img[box[4]:box[5], box[6]:box[7]]
    cl[box[0]:box[1], box[2]:box[3]] = label[box[4]:box[5], box[6]:box[7]]
    return np.ascontiguousarray(ci.transpose(2, 0, 1)), np.ascontiguousarray(pil_rescale(cl, 0.25, 0))


def top_left_sample(img: np.ndarray, crop_size: int) -> np.ndarray:
    """The eval pass's view (crop_method="top_left", src/data.py:680 and src/imutils.py:319-333): normalised, zero fill."""
    img = normalize(img)
    out = np.zeros((crop_size, crop_size, 3), np.float32)
    h, w = min(crop_size, img.shape[0]), min(crop_size, img.shape[1])
    out[:h, :w] = img[:h, :w]
    return np.ascontiguousarray(out.transpose(2, 0, 1))


class VOC12AffinityDataset:
    def __init__(self, names, voc12_root, label_dir, crop_size, train=True):
        self.names, self.root, self.label_dir, self.crop, self.is_train = list(names), voc12_root, label_dir, crop_size, train

    def __len__(self):
        return len(self.names)

    def __getitem__(self, i):
        import PIL.Image
        name = self.names[i]
        img = np.asarray(PIL.Image.open(os.path.join(self.root, "JPEGImages", name + ".jpg")).convert("RGB"))
        if not self.is_train:
            return {"img": top_left_sample(img, self.crop)}
        label = np.asarray(PIL.Image.open(os.path.join(self.label_dir, name + ".png")))
        if label.ndim != 2 or label.shape != img.shape[:2]:
            raise ValueError(f"{name}: the IR label must be a single-channel map of the image's size (got {label.shape})")
        x, y = affinity_sample(img, label.astype(np.uint8), self.crop)
        return {"img": x, "label": y}


def load_backbone(model, path: str) -> None:
    """A ResNet-50 state dict (`conv1.weight`, `layer1.0...`) goes under `resnet50.`; an IRN state dict loads as it is.  The heads
    keep their initialisation unless the file has them."""
    import torch
    sd = torch.load(path, map_location="cpu")
    sd = sd.get("state_dict", sd)
    if not any(k.startswith("resnet50.") for k in sd):
        sd = {"resnet50." + k: v for k, v in sd.items() if not k.startswith("fc.")}
    missing, unexpected = model.load_state_dict(sd, strict=False)
    bad = [k for k in missing if k.startswith("resnet50.") and not k.endswith("num_batches_tracked")]
    if bad:
        raise KeyError(f"{path}: the backbone tensors {bad[:4]}... are missing")
    if unexpected:
        print(f"[muscle_amd] note: {len(unexpected)} tensors of {path} have no place in the IRN ({unexpected[:3]}...)", file=sys.stderr)


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.train_irn", description=__doc__.split("\n")[0])
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--train_list", default="data/train_aug.txt", type=str)
    ap.add_argument("--ir_label_dir", required=True, type=str, help="IR label PNGs <name>.png (0..20, 255 = ignore)")
    ap.add_argument("--irn_weights_name", required=True, type=str, help="the checkpoint to write")
    ap.add_argument("--backbone_weights", required=True, type=str, help="ResNet-50 or IRN state dict (nothing is downloaded)")
    ap.add_argument("--irn_crop_size", default=512, type=int)
    ap.add_argument("--irn_batch_size", default=32, type=int)
    ap.add_argument("--irn_num_epoches", default=3, type=int)
    ap.add_argument("--irn_learning_rate", default=0.1, type=float)
    ap.add_argument("--irn_weight_decay", default=1e-4, type=float,
                    help="handed to PolyOptimizer as the reference does: it becomes SGD's momentum (see muscle_amd.optim)")
    ap.add_argument("--num_workers", default=8, type=int)
    ap.add_argument("--loader", default="host", choices=("host", "device"),
                    help="host: the workers build the float32 samples; device: they decode and plan only and the GPU rescales, "
                         "normalises, flips, crops and reduces the label (muscle_amd.irndata), the same tensors bit for bit")
    ap.add_argument("--seed", default=0, type=int)
    args = ap.parse_args(argv)
    if args.irn_crop_size % 16:
        ap.error("--irn_crop_size must be a multiple of 16")
    return args


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import torch
    import muscle_amd
    from muscle_amd import indexing
    from muscle_amd.infer_seg import read_names
    from torch.utils.data import DataLoader

    print(vars(args))
    random.seed(args.seed)
    np.random.seed(args.seed)
    torch.manual_seed(args.seed)
    dev = torch.device("cuda:0")
    feat = args.irn_crop_size // 4
    model = muscle_amd.AffinityDisplacementLoss(indexing.PathIndex(radius=10, default_size=(feat, feat)), crop_size=args.irn_crop_size)
    load_backbone(model, args.backbone_weights)
    model = model.to(dev)
    names = read_names(args.train_list)
    if args.loader == "device":
        # the same sampler, worker seeding and draws as below; the batches arrive as device tensors (muscle_amd.irndata)
        from muscle_amd.irndata import IrnLoader, VOC12AffinityPlans
        train = VOC12AffinityPlans(names, args.voc12_root, args.ir_label_dir, args.irn_crop_size)
        loader = IrnLoader(train, args.irn_batch_size, dev, num_workers=args.num_workers, shuffle=True, drop_last=True,
                           persistent_workers=False)
    else:
        train = VOC12AffinityDataset(names, args.voc12_root, args.ir_label_dir, args.irn_crop_size)
        loader = DataLoader(train, batch_size=args.irn_batch_size, shuffle=True, num_workers=args.num_workers, pin_memory=True,
                            drop_last=True)
    max_step = (len(train) // args.irn_batch_size) * args.irn_num_epoches
    edge_params, dp_params = model.trainable_parameters()
    optimizer = muscle_amd.PolyOptimizer([{"params": edge_params, "lr": 1 * args.irn_learning_rate},
                                          {"params": dp_params, "lr": 10 * args.irn_learning_rate}],
                                         lr=args.irn_learning_rate, weight_decay=args.irn_weight_decay, max_step=max_step)
    start = time.time()
    for ep in range(args.irn_num_epoches):
        model.train()
        print("Epoch %d/%d" % (ep + 1, args.irn_num_epoches))
        for it, pack in enumerate(loader):
            out = muscle_amd.irn_step(model, optimizer, {"img": pack["img"].to(dev, non_blocking=True),
                                                         "label": pack["label"].to(dev, non_blocking=True)})
            if (optimizer.global_step - 1) % 50 == 0:
                print("step:%5d/%5d" % (optimizer.global_step - 1, max_step),
                      "loss:%.4f %.4f %.4f %.4f" % tuple(float(out[k]) for k in ("pos_aff_loss", "neg_aff_loss", "dp_fg_loss", "dp_bg_loss")),
                      "imps:%.1f" % ((it + 1) * args.irn_batch_size / max(time.time() - start, 1e-9)),
                      "lr: %.4f" % (optimizer.param_groups[0]["lr"]), flush=True)
        start = time.time()
    # the mean displacement over the list becomes mean_shift.running_mean
    model.eval()
    model.mean_shift.running_mean.zero_()
    if args.loader == "device":
        infer = IrnLoader(VOC12AffinityPlans(names, args.voc12_root, args.ir_label_dir, args.irn_crop_size, train=False),
                          args.irn_batch_size, dev, num_workers=args.num_workers, shuffle=False, drop_last=False,
                          persistent_workers=False)
    else:
        infer = DataLoader(VOC12AffinityDataset(names, args.voc12_root, args.ir_label_dir, args.irn_crop_size, train=False),
                           batch_size=args.irn_batch_size, shuffle=False, num_workers=args.num_workers, drop_last=False)
    print("Analyzing displacements mean ... ", end="", flush=True)
    total, count = torch.zeros(2, dtype=torch.float64, device=dev), 0
    for pack in infer:
        _edge, dp = model(pack["img"].to(dev))
        total += dp.double().mean(dim=(2, 3)).sum(0)
        count += dp.shape[0]
    model.mean_shift.running_mean = (total / max(count, 1)).float()
    print("done.")
    os.makedirs(os.path.dirname(os.path.abspath(args.irn_weights_name)), exist_ok=True)
    torch.save(model.state_dict(), args.irn_weights_name)
    return 0


if __name__ == "__main__":
    sys.exit(main())
