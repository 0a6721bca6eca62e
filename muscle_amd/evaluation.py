"""Per-epoch rapid evaluation that drives ReduceLROnPlateau — train_mcl.py:286-318 + src/evaluation.py:10-68 — on the GPU.

The reference writes one `{class: float16[H,W]}` .npy per training image (1464 files), then for each of 16 thresholds
forks 8 processes that reload every file, argmax against the threshold, and count P / T / TP per class under locks.
Here each image's SGC goes `cam_maxnorm -> * label -> fp16 -> argmax vs all thresholds -> counts` in one kernel that
accumulates an int64 [thresholds, 21, 3] table on the device; the table is read once per epoch.  Same integers, same
`loglist` dict (per-category IoU in percent + 'mIoU').

`SegEval` is the same table for segmentation maps (do_python_eval with input_type='png', the evaluation of infer_seg.py's
PNGs): one integer confusion kernel per image over the uint8 prediction and ground truth.

`SegValidation` / `validate_seg` are the per-epoch validation of train_muscle.py:224-283 on top of `infer.infer_seg` and `SegEval`.

Batched sweeps (`size_buckets`, `RapidEval.add_batch`, `SegValidation.add_batch`, `rapid_eval_sweep`, `validate_seg(batch=)`):
the eval-mode forward is per-sample, so images of one size share a forward and one post-processing launch
(mx_rapid_eval_lr / mx_seg_infer_batch); the tables are integer for integer the per-image ones.  batch=1 is the per-image path.

`BoundaryEval` (new; DESIGN.md "Boundary evaluation") counts what trimap mIoU and Boundary IoU need for the same uint8 maps:
three mx_label_edge_dist launches and one mx_boundary_counts launch per image; `SegValidation` / `validate_seg` feed it the
predictions they already hold on the device (`boundary=`), `--type png --boundary 1` prints its two blocks.  Off by default.

`CamDictEval` is do_python_eval(input_type='npy') over the `{class: float32[H,W]}` dicts that infer_mcl writes, for a whole
list of thresholds at once (one mx_camdict_confusion launch per image); `python -m muscle_amd.evaluation` is the
reference's src/evaluation.py command line (:105-133) on top of it and of `SegEval`.

Differences of the command line a caller can see:
  * --curve takes a value as in the README (`--curve True`): True / true / 1 switch the threshold curve on and, unlike the
    reference's `type=bool` (any non-empty string is True), False / false / 0 switch it off;
  * --type npy needs --t or --curve (the reference would compare against `None`); a negative threshold is refused;
  * the curve reads every file once for all 60 thresholds (the reference: 60 sweeps of 8 processes each);
  * the list is read as src/data.py:load_img_name_list does (`infer_seg.read_names`), not with pandas.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Sequence

import numpy as np
import torch

from ._lib import MuscleHipError, call, lib, ptr, stream
from .phase2 import cam_maxnorm

categories = ['background', 'aeroplane', 'bicycle', 'bird', 'boat', 'bottle', 'bus', 'car', 'cat', 'chair', 'cow',
              'diningtable', 'dog', 'horse', 'motorbike', 'person', 'pottedplant', 'sheep', 'sofa', 'train', 'tvmonitor']

RAPID_THRESHOLDS = tuple(t / 100.0 for t in range(20, 52, 2))          # train_mcl.py:308-309

# the largest batch of the batched sweeps: sample b of an eval-mode batch-B forward equals the batch-1 forward of that sample
# bit for bit, which tests/test_gpu_eval_batch.py pins for B up to this value; nothing larger is accepted
MAX_EVAL_BATCH = 8
_DECODE_THREADS = 4        # host threads that decode the next batch's files; fixed, never sized by the machine


def _check_batch(batch: int) -> int:
    if not 1 <= int(batch) <= MAX_EVAL_BATCH:
        raise ValueError(f"batch must be 1..{MAX_EVAL_BATCH} (the per-sample equality of the eval forward is pinned up to "
                         f"{MAX_EVAL_BATCH}); got {batch}")
    return int(batch)


def check_thresholds(thresholds, num_cls: int, who: str):
    """The threshold list of the kernels that count every threshold at once (mx_camdict_confusion, mx_irn_sweep_confusion) as a
    tuple of floats, or ValueError with `who` as the message's prefix: 1..64 values, finite, >= 0, ascending; num_cls in 2..24
    (EVAL_MAXT / EVAL_MAXK of csrc/eval_counts.h).  A NaN would sort nowhere and a negative threshold would let the zero of an
    absent channel win, so neither is a threshold."""
    import math
    ts = tuple(float(t) for t in thresholds)
    if not 1 <= len(ts) <= 64:
        raise ValueError(f"{who} takes 1..64 thresholds (got {len(ts)})")
    if any(not math.isfinite(t) or t < 0 for t in ts):
        raise ValueError(f"{who}: a negative threshold would let the zero of an absent channel win; thresholds must be finite and >= 0")
    if any(b < a for a, b in zip(ts, ts[1:])):
        raise ValueError(f"{who}: thresholds must be ascending")
    if not 2 <= int(num_cls) <= 24:
        raise ValueError(f"{who}: num_cls {num_cls} outside 2..24")
    return ts


def size_buckets(names_and_sizes, batch: int) -> List[List[str]]:
    """names_and_sizes: (name, (W, H)) pairs, the size as `PIL.Image.open(path).size` gives it.  Groups the names by size and
    cuts every group into batches of at most `batch`; within a group the list order is kept, the groups come in the order
    of their first image.  batch=1 is the list itself, one name per batch."""
    if int(batch) < 1:
        raise ValueError(f"batch must be >= 1 (got {batch})")
    pairs = [(n, tuple(sz)) for n, sz in names_and_sizes]
    if int(batch) == 1:
        return [[n] for n, _ in pairs]
    groups: Dict[tuple, List[str]] = {}
    for n, sz in pairs:
        groups.setdefault(sz, []).append(n)
    return [g[i:i + batch] for g in groups.values() for i in range(0, len(g), batch)]


def _image_sizes(names: Sequence[str], voc12_root: str):
    """(name, (W, H)) from the JPEG headers (PIL.Image.open decodes nothing)."""
    import os
    import PIL.Image
    out = []
    for n in names:
        with PIL.Image.open(os.path.join(voc12_root, 'JPEGImages', n + '.jpg')) as im:
            out.append((n, im.size))
    return out


def _decode(voc12_root: str, name: str):
    """Host only: the RGB image and the SegmentationClass map of one name."""
    import os
    import PIL.Image
    img = PIL.Image.open(os.path.join(voc12_root, 'JPEGImages', name + '.jpg')).convert('RGB')
    gt = np.ascontiguousarray(np.array(PIL.Image.open(os.path.join(voc12_root, 'SegmentationClass', name + '.png'))), dtype=np.uint8)
    return img, gt


def _prefetched(buckets: List[List[str]], voc12_root: str):
    """Yields (names, [(img, gt), ...]) per bucket; the NEXT bucket's files are decoded on a small thread pool while the
    caller works on the current one.  The pool only reads and decodes files."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=_DECODE_THREADS) as pool:
        submit = lambda b: [pool.submit(_decode, voc12_root, n) for n in b]  # noqa: E731
        nxt = submit(buckets[0]) if buckets else None
        for i, b in enumerate(buckets):
            cur, nxt = nxt, (submit(buckets[i + 1]) if i + 1 < len(buckets) else None)
            yield b, [f.result() for f in cur]


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

    def add_batch(self, model, imgs: torch.Tensor, labels: torch.Tensor, gts: torch.Tensor) -> None:
        """B images of one size in one forward: imgs [B,3,H,W], labels [B,20], gts uint8 [B,H,W].  The forward is asked for
        its low-resolution maps (cam='cam_lr') and mx_rapid_eval_lr does the upsample, cam_maxnorm, label multiply, fp16
        rounding, argmax and counting of `add` without a full-resolution tensor: the same integers as B calls of `add`."""
        if not imgs.is_cuda:
            raise MuscleHipError("RapidEval runs on the HIP kernels only")
        if imgs.dim() != 4:
            raise ValueError(f"imgs must be [B,3,H,W] (got {tuple(imgs.shape)})")
        B, _, H, W = imgs.shape
        _check_batch(B)
        K, nt = self.num_cls, len(self.thresholds)
        if tuple(gts.shape) != (B, H, W) or gts.dtype != torch.uint8:
            raise ValueError(f"gts must be uint8 [{B},{H},{W}] (got {gts.dtype} {tuple(gts.shape)})")
        if tuple(labels.shape) != (B, K - 1):
            raise ValueError(f"labels must be [{B},{K - 1}] (got {tuple(labels.shape)})")
        if not model.training and getattr(model.backbone, "_eval_fold", None) is None and hasattr(model, "fold_eval_bn"):
            model.fold_eval_bn()
        dev = imgs.device
        with torch.no_grad():
            _, sgc_lr, _, _ = model(imgs.float(), cam="cam_lr")                 # NHWC [B,h,w,24]
        _, h, w, lds = sgc_lr.shape
        lwb = torch.cat([torch.ones(B, 1, device=dev), labels.to(dev).float()], dim=1).contiguous()
        nbytes = int(lib().mx_rapid_eval_lr_ws(B, K))
        ws = torch.empty(nbytes, dtype=torch.uint8, device=dev)
        call("mx_rapid_eval_lr", ptr(sgc_lr.contiguous()), ptr(lwb), ptr(gts.to(dev).contiguous()), ptr(self.thr), nt, B, h, w, lds,
             K, H, W, ptr(self.counts), ptr(ws), nbytes, stream())

    def loglist(self, ti: int) -> Dict[str, float]:
        """do_python_eval's return value for threshold index ti (src/evaluation.py:56-68)."""
        return miou_loglist(self.counts[ti].cpu().numpy())

    def best(self):
        """(max_miou, max_t) exactly as train_mcl.py:311-312 (first maximum; max_t = index*0.02 + 0.2 there)."""
        mious: List[float] = [self.loglist(i)['mIoU'] for i in range(len(self.thresholds))]
        max_miou = max(mious)
        return max_miou, self.thresholds[mious.index(max_miou)], mious


def rapid_eval_sweep(model, names: Sequence[str], voc12_root: str, labels, device, batch: int = 1, num_cls: int = 21) -> RapidEval:
    """train_mcl.py:286-306 over the images `names` of a VOC tree; labels: {name: [20]}.  Returns the filled RapidEval
    (`.best()` is :308-312); leaves the model in eval mode.  batch=1: one image per forward (`RapidEval.add`), in list order.
    batch>1: images of one size share a forward (`size_buckets`, `RapidEval.add_batch`) and the next batch's files are
    decoded on host threads meanwhile; the table is the same, integer for integer."""
    from .data import MSFStager
    batch = _check_batch(batch)
    model.eval()
    ev, stager = RapidEval(device, num_cls=num_cls), MSFStager(device)
    lab = lambda n: torch.from_numpy(np.asarray(labels[n], dtype=np.float32)).view(1, -1)  # noqa: E731
    if batch == 1:
        for name in names:
            img, gt = _decode(voc12_root, name)
            ev.add(model, stager(img, (1,))[0], lab(name), torch.from_numpy(gt).to(device))
        return ev
    for bnames, items in _prefetched(size_buckets(_image_sizes(names, voc12_root), batch), voc12_root):
        imgs = torch.cat([stager(img, (1,))[0] for img, _ in items], dim=0)
        gts = torch.from_numpy(np.stack([gt for _, gt in items])).to(device)
        ev.add_batch(model, imgs, torch.cat([lab(n) for n in bnames], dim=0), gts)
    return ev


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


def boundary_radius(H: int, W: int, ratio: float, dmax: int) -> int:
    """The per-image radius of Boundary IoU: round(ratio * diagonal), at least 1 (as the published code chooses it), at most dmax."""
    import math
    return min(int(dmax), max(1, int(round(float(ratio) * math.hypot(int(H), int(W))))))


class BoundaryEval:
    """Boundary evaluation of segmentation maps (DESIGN.md "Boundary evaluation"): trimap mIoU - mIoU inside the band of
    Chebyshev radius d around the ground truth's label changes - and Boundary IoU (Cheng et al. 2021) for every d in 1..dmax
    from one pass per image.  Per image three mx_label_edge_dist launches (gt without and with the image edge, pred with it)
    and one mx_boundary_counts launch accumulate two integer tables on the device:
      hist  int64 [6, num_cls, dmax+2]: rows (T_tri, P_tri, TP_tri, T_b, P_b, TP_b) binned by distance (bin 0 unused,
            bin dmax+1 = farther than dmax); a count within d is the sum of bins 1..d;
      ratio int64 [3, num_cls]: (T_b, P_b, TP_b) within each image's own radius `boundary_radius(H, W, ratio, dmax)`.
    The metrics are float64 on the host, formed as `miou_loglist` forms mIoU: per class TP / (T + P - TP + 1e-10), the mean
    over all num_cls classes, in per cent."""

    ROWS = ("T_tri", "P_tri", "TP_tri", "T_b", "P_b", "TP_b")

    def __init__(self, device, num_cls: int = 21, dmax: int = 16, ratio: float = 0.02):
        if not 2 <= int(num_cls) <= 32:
            raise ValueError(f"BoundaryEval: num_cls {num_cls} outside 2..32")
        if not 1 <= int(dmax) <= 64:
            raise ValueError(f"BoundaryEval: dmax {dmax} outside 1..64")
        if not float(ratio) > 0:
            raise ValueError(f"BoundaryEval: ratio must be positive (got {ratio})")
        self.num_cls, self.dmax, self.ratio = int(num_cls), int(dmax), float(ratio)
        self.hist = torch.zeros(6, self.num_cls, self.dmax + 2, dtype=torch.int64, device=device)
        self.ratio_counts = torch.zeros(3, self.num_cls, dtype=torch.int64, device=device)
        self._dist = None                                    # uint8 [3,H,W] of the last size: dt, db, dp

    def reset(self) -> None:
        self.hist.zero_()
        self.ratio_counts.zero_()

    def add(self, pred: torch.Tensor, gt: torch.Tensor) -> None:
        """pred: uint8 [H,W] class indices; gt: uint8 [H,W] SegmentationClass png (255 = ignore)."""
        if not self.hist.is_cuda:
            raise MuscleHipError("BoundaryEval.add runs on the HIP kernels only: create it with a ROCm device")
        if pred.dim() != 2 or pred.dtype != torch.uint8 or gt.dtype != torch.uint8 or tuple(gt.shape) != tuple(pred.shape):
            raise ValueError(f"pred and gt must be uint8 [H,W] of one shape (got {pred.dtype} {tuple(pred.shape)}, "
                             f"{gt.dtype} {tuple(gt.shape)})")
        H, W = pred.shape
        dev = self.hist.device
        p, g = pred.to(dev).contiguous(), gt.to(dev).contiguous()
        if self._dist is None or tuple(self._dist.shape[1:]) != (H, W):
            self._dist = torch.empty(3, H, W, dtype=torch.uint8, device=dev)
        d, st = self._dist, stream()
        call("mx_label_edge_dist", ptr(g), H, W, self.dmax, 0, ptr(d[0]), st)
        call("mx_label_edge_dist", ptr(g), H, W, self.dmax, 1, ptr(d[1]), st)
        call("mx_label_edge_dist", ptr(p), H, W, self.dmax, 1, ptr(d[2]), st)
        call("mx_boundary_counts", ptr(p), ptr(g), ptr(d[0]), ptr(d[1]), ptr(d[2]), self.num_cls, H, W, self.dmax,
             boundary_radius(H, W, self.ratio, self.dmax), ptr(self.hist), ptr(self.ratio_counts), st)

    def tables(self):
        """(hist [6,num_cls,dmax+2], ratio [3,num_cls]) as numpy int64."""
        return self.hist.cpu().numpy(), self.ratio_counts.cpu().numpy()

    def _check_d(self, d) -> int:
        if not 1 <= int(d) <= self.dmax:
            raise ValueError(f"d must be in 1..{self.dmax} (got {d})")
        return int(d)

    @staticmethod
    def _iou(T, P, TP):
        return TP / (T + P - TP + 1e-10)

    def _within(self, hist, d):
        c = hist[:, :, 1:d + 1].sum(axis=2)
        return c[0], c[1], c[2], c[3], c[4], c[5]

    def trimap_miou(self, d: int) -> float:
        """mIoU (per cent) over the pixels within Chebyshev distance d of a change of the ground-truth label."""
        T, P, TP, _, _, _ = self._within(self.tables()[0], self._check_d(d))
        return float(np.mean(self._iou(T, P, TP)) * 100)

    def trimap_curve(self) -> List[float]:
        """trimap_miou(d) for d = 1..dmax from one read of the table."""
        hist = self.tables()[0]
        out = []
        for d in range(1, self.dmax + 1):
            T, P, TP, _, _, _ = self._within(hist, d)
            out.append(float(np.mean(self._iou(T, P, TP)) * 100))
        return out

    def boundary_miou(self, d: Optional[int] = None) -> float:
        """Mean Boundary IoU (per cent) at radius d; None: at every image's own radius (the ratio table)."""
        hist, ratio = self.tables()
        if d is None:
            T, P, TP = ratio[0], ratio[1], ratio[2]
        else:
            _, _, _, T, P, TP = self._within(hist, self._check_d(d))
        return float(np.mean(self._iou(T, P, TP)) * 100)

    def loglist(self) -> Dict[str, float]:
        """Per-category Boundary IoU in per cent at the per-image radius + 'mIoU', the dict shape of `miou_loglist`."""
        r = self.tables()[1]
        return miou_loglist(np.stack([r[2], r[1], r[0]], axis=1))

    def lines(self) -> List[str]:
        """What the scripts print after the IoU table: the Boundary-IoU table, then the trimap curve, one line per d."""
        log = self.loglist()
        out, row = ['Boundary IoU (ratio %g of the diagonal, at most %d px):' % (self.ratio, self.dmax)], ''
        for i in range(self.num_cls):
            nm = categories[i] if i < len(categories) else str(i)
            row += '%11s:%7.3f%%' % (nm, log[nm])
            if i % 2 == 1 or i == self.num_cls - 1:
                out.append(row)
                row = ''
            else:
                row += '\t'
        out.append('%11s:%7.3f%%' % ('mBIoU', log['mIoU']))
        hist = self.tables()[0]
        for d in range(1, self.dmax + 1):
            T, P, TP, Tb, Pb, TPb = self._within(hist, d)
            out.append('trimap d=%2d\tmIoU: %.3f%%\tBoundary mIoU: %.3f%%' % (d, np.mean(self._iou(T, P, TP)) * 100,
                                                                             np.mean(self._iou(Tb, Pb, TPb)) * 100))
        return out

    def logdict(self) -> Dict[str, object]:
        """What the scripts append to --logfile."""
        hist = self.tables()[0]
        bc = []
        for d in range(1, self.dmax + 1):
            _, _, _, Tb, Pb, TPb = self._within(hist, d)
            bc.append(float(np.mean(self._iou(Tb, Pb, TPb)) * 100))
        return {'boundary': self.loglist(), 'trimap_mIoU': self.trimap_curve(), 'boundary_mIoU': bc}


class SegValidation:
    """The per-epoch validation of train_muscle.py:224-283 on the device: per image the single scale-1, un-flipped pass of
    the eval list (`img_list[:1]`), softmax, resize to the ground truth's size, optional class-score scaling (--cls_dir,
    :262-264), optional dense CRF with t=1 (:266-267; the exact windowed CRF of muscle_amd.crf), argmax, and the (TP, P, T)
    counts of :270-276 in a `SegEval` table.  `miou()` is :278-280: mean over classes of TP / (T + P - TP + 1e-10), a
    fraction (the value ReduceLROnPlateau is stepped with), not a percentage."""

    def __init__(self, device, num_cls: int = 21, cls_dir=None, crf: bool = False, crf_trunc: float = 4.0,
                 boundary: Optional[BoundaryEval] = None):
        from .data import MSFStager
        self.dev, self.cls_dir, self.crf, self.crf_trunc = device, cls_dir, bool(crf), crf_trunc
        self.stager = MSFStager(device)
        self.table = SegEval(device, num_cls)
        self.boundary = boundary                 # optional: fed every prediction the table is fed, where it lies on the device

    def reset(self) -> None:
        self.table.counts.zero_()
        if self.boundary is not None:
            self.boundary.reset()

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
        gd = torch.from_numpy(np.ascontiguousarray(gt, dtype=np.uint8)).to(self.dev)
        self.table.add(pred, gd)
        if self.boundary is not None:
            self.boundary.add(pred, gd)
        return pred

    def add_batch(self, model, pil_imgs, gts, names=None) -> torch.Tensor:
        """`add` for B images of one size in one forward and one mx_seg_infer_batch launch, which also counts (without the
        CRF; with it mx_crf_inference and the counting run per image, as in `add`).  pil_imgs: B RGB images; gts: B uint8
        [H,W] maps; names: the B names, needed with cls_dir.  Returns the uint8 predictions [B,H,W] on the device."""
        import os
        from .infer import infer_seg_batch
        B = _check_batch(len(pil_imgs))
        g = np.stack([np.ascontiguousarray(np.asarray(x), dtype=np.uint8) for x in gts])
        if g.ndim != 3 or g.shape[0] != B:
            raise ValueError(f"gts must be {B} maps of one size [H,W] (got {g.shape})")
        _, H, W = g.shape
        cls = None
        if self.cls_dir:
            cls = np.stack([np.asarray(np.load(os.path.join(self.cls_dir, n + '.npy'), allow_pickle=True).squeeze(),
                                       dtype=np.float32).reshape(-1) for n in names])
        crf_imgs = [np.asarray(im, dtype=np.uint8) for im in pil_imgs] if self.crf else None
        imgs = torch.cat([self.stager(im, (1,))[0] for im in pil_imgs], dim=0)
        gd = torch.from_numpy(g).to(self.dev)
        pred, _ = infer_seg_batch(model, imgs, H, W, cls_labels=cls, crf_imgs=crf_imgs, crf_t=1, crf_trunc=self.crf_trunc,
                                  gts=None if self.crf else gd, counts=None if self.crf else self.table.counts)
        if self.crf:
            for b in range(B):
                self.table.add(pred[b], gd[b])
        if self.boundary is not None:
            for b in range(B):
                self.boundary.add(pred[b], gd[b])
        return pred

    def miou(self) -> float:
        return float(miou_loglist(self.table.counts.cpu().numpy())['mIoU']) / 100.0


def validate_seg(model, names: Sequence[str], voc12_root: str, device, num_cls: int = 21, cls_dir=None, crf: bool = False,
                 batch: int = 1, boundary: Optional[BoundaryEval] = None) -> float:
    """train_muscle.py:224-283 over the images `names` of a VOC tree; leaves the model in eval mode (as the script does
    until the next epoch's model.train()).  batch=1: one image per forward (`SegValidation.add`), in list order.  batch>1:
    images of one size share a forward (`size_buckets`, `SegValidation.add_batch`) and the next batch's files are decoded on
    host threads meanwhile; the same table.  boundary: an optional `BoundaryEval` that is fed the same predictions (it is not
    reset here: the caller owns it and reads it afterwards)."""
    batch = _check_batch(batch)
    model.eval()
    val = SegValidation(device, num_cls, cls_dir=cls_dir, crf=crf, boundary=boundary)
    if batch == 1:
        for name in names:
            img, gt = _decode(voc12_root, name)
            val.add(model, img, gt, name)
        return val.miou()
    for bnames, items in _prefetched(size_buckets(_image_sizes(names, voc12_root), batch), voc12_root):
        val.add_batch(model, [img for img, _ in items], [gt for _, gt in items], bnames)
    return val.miou()


class CamDictEval:
    """do_python_eval(input_type='npy') (src/evaluation.py:25-68) for every threshold of `thresholds` at once: accumulates the
    int64 (TP, P, T) table [len(thresholds), num_cls, 3] on the device, one mx_camdict_confusion launch per image."""

    def __init__(self, device, thresholds: Sequence[float], num_cls: int = 21):
        self.thresholds = check_thresholds(thresholds, num_cls, "CamDictEval")
        self.num_cls = num_cls
        self.dev = torch.device(device)
        self.thr = torch.tensor(self.thresholds, dtype=torch.float32, device=device)
        self.counts = torch.zeros(len(self.thresholds), num_cls, 3, dtype=torch.int64, device=device)

    def add(self, pred_dict: Dict[int, np.ndarray], gt) -> None:
        """pred_dict: {class key 0..num_cls-2: [H,W] map of any float dtype} (stored as float32, as `tensor[key+1] = ...` of
        :29-31 does); gt: uint8 [H,W] SegmentationClass map (255 = ignore), numpy or tensor."""
        if not self.counts.is_cuda:
            raise MuscleHipError("CamDictEval.add runs on the HIP kernels only: create it with a ROCm device")
        keys = sorted(int(k) for k in pred_dict.keys())
        if not keys:
            raise ValueError("CamDictEval.add: empty dict (src/evaluation.py:28 needs one map for the image size)")
        if keys[0] < 0 or keys[-1] > self.num_cls - 2 or len(set(keys)) != len(keys):
            raise ValueError(f"CamDictEval.add: class keys {keys} outside 0..{self.num_cls - 2}")
        maps = np.stack([np.asarray(pred_dict[k]) for k in keys]).astype(np.float32, copy=False)
        if maps.ndim != 3:
            raise ValueError(f"CamDictEval.add: maps must be [H,W] (got {maps.shape[1:]})")
        _, H, W = maps.shape
        g = gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt))
        if g.dtype != torch.uint8 or tuple(g.shape) != (H, W):
            raise ValueError(f"gt must be uint8 [{H},{W}] (got {g.dtype} {tuple(g.shape)})")
        m = torch.from_numpy(np.ascontiguousarray(maps)).to(self.dev)
        kk = torch.tensor(keys, dtype=torch.int32).to(self.dev)
        call("mx_camdict_confusion", ptr(m), ptr(kk), len(keys), ptr(g.to(self.dev).contiguous()), ptr(self.thr),
             len(self.thresholds), self.num_cls, H, W, ptr(self.counts), stream())

    def loglist(self, ti: int) -> Dict[str, float]:
        """do_python_eval's return value for threshold index ti (src/evaluation.py:56-75)."""
        return miou_loglist(self.counts[ti].cpu().numpy())

    def mious(self) -> List[float]:
        """loglist(ti)['mIoU'] for every threshold, from one read of the table."""
        c = self.counts.cpu().numpy()
        return [miou_loglist(c[ti])['mIoU'] for ti in range(len(self.thresholds))]


# ---- python -m muscle_amd.evaluation: src/evaluation.py:72-133 --------------------------------------------------------------
def print_loglist(loglist: Dict[str, float], num_cls: int = 21) -> None:
    """do_python_eval(printlog=True), src/evaluation.py:76-83."""
    for i in range(num_cls):
        nm = categories[i] if i < len(categories) else str(i)
        if i % 2 != 1:
            print('%11s:%7.3f%%' % (nm, loglist[nm]), end='\t')
        else:
            print('%11s:%7.3f%%' % (nm, loglist[nm]))
    print('\n======================================================')
    print('%11s:%7.3f%%' % ('mIoU', loglist['mIoU']))


def writedict(file, dictionary) -> None:
    """src/evaluation.py:86-92."""
    s = ''
    for key in dictionary.keys():
        s += '%s:%s  ' % (key, dictionary[key])
    file.write(s + '\n')


def writelog(filepath: str, metric, comment: str) -> None:
    """src/evaluation.py:94-102: appends the time stamp, the comment, the metric dict and a rule."""
    import time
    with open(filepath, 'a') as logfile:
        logfile.write(time.strftime("%Y-%m-%d %H:%M:%S", time.localtime()))
        logfile.write('\t%s\n' % comment)
        writedict(logfile, metric)
        logfile.write('=====================================\n')


def _flag(v: str) -> bool:
    if v in ("True", "true", "1"):
        return True
    if v in ("False", "false", "0"):
        return False
    import argparse
    raise argparse.ArgumentTypeError(f"--curve takes True/true/1 or False/false/0 (got {v!r})")


def parse_args(argv: Optional[List[str]] = None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.evaluation",
                                 description="The reference's src/evaluation.py (IoU table of CAM dicts or segmentation PNGs) on the HIP path.")
    ap.add_argument("--list", default="data/train.txt", type=str)
    ap.add_argument("--predict_dir", default="out_sgc", type=str)
    ap.add_argument("--gt_dir", default="data/VOC2012/SegmentationClass", type=str)
    ap.add_argument("--logfile", default="./evallog.txt", type=str)
    ap.add_argument("--comment", required=True, type=str)
    ap.add_argument("--type", default="npy", choices=["npy", "png"], type=str)
    ap.add_argument("--t", default=None, type=float, help="background threshold of --type npy (>= 0)")
    ap.add_argument("--curve", default=False, type=_flag,
                    help="True/true/1: mIoU at the 60 thresholds 0.00..0.59 from one pass over the files; False/false/0: off "
                         "(the reference's type=bool reads any non-empty string as True)")
    ap.add_argument("--boundary", default=0, type=int, choices=(0, 1),
                    help="--type png, 1: after the IoU table, the Boundary-IoU table and the trimap curve (BoundaryEval)")
    ap.add_argument("--boundary_dmax", default=16, type=int, help="--boundary 1: the largest band radius in pixels (1..64)")
    ap.add_argument("--boundary_ratio", default=0.02, type=float,
                    help="--boundary 1: the per-image Boundary-IoU radius as a fraction of the image diagonal")
    args = ap.parse_args(argv)
    if args.boundary and args.type != "png":
        ap.error("--boundary 1 evaluates label maps: it needs --type png")
    if args.boundary and not (1 <= args.boundary_dmax <= 64 and args.boundary_ratio > 0):
        ap.error("--boundary_dmax must be in 1..64 and --boundary_ratio positive")
    if args.curve and args.type != "npy":
        ap.error("--curve sweeps the background threshold of --type npy")
    if args.type == "npy" and not args.curve and args.t is None:
        ap.error("--type npy needs a background threshold: --t T, or --curve True for the 60-threshold sweep")
    if args.type == "npy" and not args.curve and args.t < 0:
        ap.error("--t must be >= 0")
    return args


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import os
    import PIL.Image
    from .infer_seg import read_names
    dev = torch.device("cuda:0")
    names = read_names(args.list)
    gt_of = lambda n: np.array(PIL.Image.open(os.path.join(args.gt_dir, n + ".png")))  # noqa: E731
    if args.type == "png":
        ev = SegEval(dev, 21)
        bev = BoundaryEval(dev, 21, args.boundary_dmax, args.boundary_ratio) if args.boundary else None
        for n in names:
            pred = np.array(PIL.Image.open(os.path.join(args.predict_dir, n + ".png")))
            p, g = torch.from_numpy(pred).to(dev), torch.from_numpy(gt_of(n)).to(dev)
            ev.add(p, g)
            if bev is not None:
                bev.add(p, g)
        loglist = ev.loglist()
        print_loglist(loglist)
        writelog(args.logfile, loglist, args.comment)
        if bev is not None:
            print("\n".join(bev.lines()))
            writelog(args.logfile, bev.logdict(), args.comment + " (boundary)")
        return 0
    thresholds = [i / 100.0 for i in range(60)] if args.curve else [args.t]
    cev = CamDictEval(dev, thresholds, 21)
    for n in names:
        cev.add(np.load(os.path.join(args.predict_dir, n + ".npy"), allow_pickle=True).item(), gt_of(n))
    if not args.curve:
        loglist = cev.loglist(0)
        print_loglist(loglist)
        writelog(args.logfile, loglist, args.comment)
        return 0
    l = cev.mious()
    for i, t in enumerate(thresholds):
        print('%d/60 background score: %.3f\tmIoU: %.3f%%' % (i, t, l[i]))
    writelog(args.logfile, {'mIoU': l}, args.comment)
    return 0


if __name__ == "__main__":
    import sys
    sys.exit(main())
