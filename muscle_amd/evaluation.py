"""Per-epoch rapid evaluation that drives ReduceLROnPlateau — train_mcl.py:286-318 + src/evaluation.py:10-68 — on the GPU.

The reference writes one `{class: float16[H,W]}` .npy per training image (1464 files), then for each of 16 thresholds
forks 8 processes that reload every file, argmax against the threshold, and count P / T / TP per class under locks.
Here each image's SGC goes `cam_maxnorm -> * label -> fp16 -> argmax vs all thresholds -> counts` in one kernel that
accumulates an int64 [thresholds, 21, 3] table on the device; the table is read once per epoch.  Same integers, same
`loglist` dict (per-category IoU in percent + 'mIoU').

`SegEval` is the same table for segmentation maps (do_python_eval with input_type='png', the evaluation of infer_seg.py's
PNGs): one integer confusion kernel per image over the uint8 prediction and ground truth.

`SegValidation` / `validate_seg` are the per-epoch validation of train_muscle.py:224-283 on top of `infer.infer_seg` and `SegEval`.
"""
from __future__ import annotations

from typing import Dict, List, Sequence

import numpy as np
import torch

from ._lib import MuscleHipError, call, ptr, stream
from .phase2 import cam_maxnorm

categories = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
              'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']

RAPID_THRESHOLDS = tuple(t / 100.0 for t in range(20, 52, 2))          # train_mcl.py:308-309


def miou_loglist(counts) -> Dict[str, float]:
    """src/evaluation.py:56-68 on an integer (TP, P, T) table [num_cls, 3]: per-category IoU in percent + 'mIoU'."""
    c = np.asarray(counts).astype(np.int64)
    num_cls = c.shape[0]
    TP, P, T = c[:, 0], c[:, 1], c[:, 2]
    iou = [TP[i] / (T[i] + P[i] - TP[i] + 1e-10) for i in range(num_cls)]
    out = {categories[i] if i < len(categories) else str(i): iou[i] * 100 for i in range(num_cls)}
    out['mIoU'] = np.mean(np.array(iou)) * 100
    return out


class RapidEval:
    """Accumulates the (TP, P, T) table over the evaluation images of one epoch."""

    def __init__(self, device, thresholds: Sequence[float] = RAPID_THRESHOLDS, num_cls: int = 21):
        self.thresholds = tuple(float(t) for t in thresholds)
        self.num_cls = num_cls
        self.thr = torch.tensor(self.thresholds, dtype=torch.float32, device=device)
        self.counts = torch.zeros(len(self.thresholds), num_cls, 3, dtype=torch.int64, device=device)

    def add_prediction(self, pred: torch.Tensor, label_with_bg: torch.Tensor, gt: torch.Tensor) -> None:
        """pred: [K,H,W] fp32 CUDA, already cam_maxnorm'ed (train_mcl.py:297); label_with_bg: [K]; gt: uint8 [H,W]
        (255 = ignore), the SegmentationClass png."""
        if not pred.is_cuda:
            raise MuscleHipError("RapidEval runs on the HIP kernels only")
        K, H, W = pred.shape
        if gt.shape != (H, W) or gt.dtype != torch.uint8:
            raise ValueError(f"gt must be uint8 [{H},{W}] (got {gt.dtype} {tuple(gt.shape)})")
        pred = pred.contiguous().float()
        lab = label_with_bg.to(pred.device, torch.float32).contiguous().view(-1)
        g = gt.to(pred.device).contiguous()
        call("mx_eval_confusion", ptr(pred), ptr(lab), ptr(g), ptr(self.thr), len(self.thresholds), K, H, W, ptr(self.counts),
             stream())

    def add(self, model, img: torch.Tensor, label: torch.Tensor, gt: torch.Tensor) -> None:
        """One image of the eval loader (train_mcl.py:290-303): img [1,3,H,W], label [1,20], gt uint8 [H,W]."""
        if not model.training and getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
            model.fold_eval_bn()          # once per evaluation sweep: model.train() drops it again (weights change)
        with torch.no_grad():
            _, pred, _, _ = model(img.float(), cam="cam")
            pred = cam_maxnorm(pred)
        lwb = torch.cat([torch.ones(1, device=pred.device), label.view(-1).to(pred.device).float()])
        self.add_prediction(pred[0], lwb, gt)

    def loglist(self, ti: int) -> Dict[str, float]:
        """do_python_eval's return value for threshold index ti (src/evaluation.py:56-68)."""
        return miou_loglist(self.counts[ti].cpu().numpy())

    def best(self):
        """(max_miou, max_t) exactly as train_mcl.py:311-312 (first maximum; max_t = index*0.02 + 0.2 there)."""
        mious: List[float] = [self.loglist(i)['mIoU'] for i in range(len(self.thresholds))]
        max_miou = max(mious)
        return max_miou, self.thresholds[mious.index(max_miou)], mious


class SegEval:
    """do_python_eval(input_type='png') (src/evaluation.py:10-68) over segmentation maps: accumulates the int64 (TP, P, T)
    table [num_cls, 3] on the device, one mx_seg_confusion launch per image; loglist() reads it once."""

    def __init__(self, device, num_cls: int = 21):
        self.num_cls = num_cls
        self.counts = torch.zeros(num_cls, 3, dtype=torch.int64, device=device)

    def add(self, pred: torch.Tensor, gt: torch.Tensor) -> None:
        """pred: uint8 [H,W] class indices (infer.infer_seg); gt: uint8 [H,W] SegmentationClass png (255 = ignore)."""
        if not self.counts.is_cuda:
            raise MuscleHipError("SegEval.add runs on the HIP kernels only: create it with a ROCm device")
        if pred.dim() != 2 or pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or tuple(gt.shape) != tuple(pred.shape):
            raise ValueError(f"pred and gt must be uint8 [H,W] of one shape (got {pred.dtype} {tuple(pred.shape)}, "
                             f"{gt.dtype} {tuple(gt.shape)})")
        H, W = pred.shape
        dev = self.counts.device
        call("mx_seg_confusion", ptr(pred.to(dev).contiguous()), ptr(gt.to(dev).contiguous()), self.num_cls, H, W,
             ptr(self.counts), stream())

    def loglist(self) -> Dict[str, float]:
        """do_python_eval's return value (src/evaluation.py:56-68)."""
        return miou_loglist(self.counts.cpu().numpy())


class SegValidation:
    """The per-epoch validation of train_muscle.py:224-283 on the device: per image the single scale-1, un-flipped pass of
    the eval list (`img_list[:1]`), softmax, resize to the ground truth's size, optional class-score scaling (--cls_dir,
    :262-264), optional dense CRF with t=1 (:266-267; the exact windowed CRF of muscle_amd.crf), argmax, and the (TP, P, T)
    counts of :270-276 in a `SegEval` table.  `miou()` is :278-280: mean over classes of TP / (T + P - TP + 1e-10), a
    fraction (the value ReduceLROnPlateau is stepped with), not a percentage."""

    def __init__(self, device, num_cls: int = 21, cls_dir=None, crf: bool = False, crf_trunc: float = 4.0):
        from .data import MSFStager
        self.dev, self.cls_dir, self.crf, self.crf_trunc = device, cls_dir, bool(crf), crf_trunc
        self.stager = MSFStager(device)
        self.table = SegEval(device, num_cls)

    def reset(self) -> None:
        self.table.counts.zero_()

    def add(self, model, pil_img, gt, name=None) -> torch.Tensor:
        """pil_img: the RGB image; gt: uint8 [H,W] SegmentationClass map (255 = ignore); name: the image's name, needed
        with cls_dir (`<cls_dir>/<name>.npy`).  Returns the uint8 prediction [H,W] on the device."""
        import os
        from .infer import infer_seg
        gt = np.asarray(gt)
        H, W = gt.shape
        cls = None
        if self.cls_dir:
            cls = np.load(os.path.join(self.cls_dir, name + '.npy'), allow_pickle=True).squeeze()
        crf_img = np.asarray(pil_img, dtype=np.uint8) if self.crf else None
        pred, _ = infer_seg(model, self.stager(pil_img, (1,))[:1], H, W, cls_label=cls, crf_img=crf_img, crf_t=1,
                            crf_trunc=self.crf_trunc)
        self.table.add(pred, torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(self.dev))
        return pred

    def miou(self) -> float:
        return float(miou_loglist(self.table.counts.cpu().numpy())['mIoU']) / 100.0


def validate_seg(model, names: Sequence[str], voc12_root: str, device, num_cls: int = 21, cls_dir=None, crf: bool = False) -> float:
    """train_muscle.py:224-283 over the images `names` of a VOC tree; leaves the model in eval mode (as the script does
    until the next epoch's model.train())."""
    import os
    import PIL.Image
    model.eval()
    val = SegValidation(device, num_cls, cls_dir=cls_dir, crf=crf)
    for name in names:
        img = PIL.Image.open(os.path.join(voc12_root, 'JPEGImages', name + '.jpg')).convert('RGB')
        gt = np.array(PIL.Image.open(os.path.join(voc12_root, 'SegmentationClass', name + '.png')))
        val.add(model, img, gt, name)
    return val.miou()
