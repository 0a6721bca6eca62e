"""Instance-segmentation evaluation: IRN's published `eval_ins_seg` step (VOC AP^r at several IoU thresholds) on the HIP path.

`infer_irn --ins_seg_out_dir` writes instance pseudo-labels (muscle_amd/ins_seg.py); this module says how good they are
("Instance evaluation", is the specification):

  1. ground truth   voc_instances: SegmentationClass + SegmentationObject PNGs -> the instance map G (uint8, 0 = none, j = the
                    j-th object) and the objects' classes; host, one bincount
  2. pair table     one pass over the pixels gives the integer joint-count table of the prediction against G
                        InstanceLabels (non-overlapping seg_map, on the device already)         mx_label_pair_counts
                        IRN dict / bool [n,H,W] masks (may overlap)                              mx_mask_pair_counts
                    read back with one synchronising copy per image; the bool [n,H,W] stack of an InstanceLabels is never formed
  3. IoU            mask_iou: I / (A_p + A_g - I) for every (prediction, object) pair from the table, float64, host
  4. AP             InsSegEval: greedy matching per image, class and threshold; pooled precision/recall per class; the area
                    under the monotone precision envelope (all points, not the 11-point VOC07 rule); float64, host.  One table
                    per image serves all thresholds.

What is pinned is this algorithm against a numpy restatement (tests/ins_eval_ref.py); parity with chainercv's
`eval_instance_segmentation_voc` and with IRN's own numbers is unpinned (neither is available to the tests): that covers the
argsort tie order, the void handling and the object-class rule.

`python -m muscle_amd.ins_eval --voc12_root VOC --list LIST --ins_seg_dir INS` evaluates a directory of `<name>.npy` files.
"""
from __future__ import annotations

import argparse
import os
import sys
from typing import List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import MuscleHipError, call, ptr, stream
from .ins_seg import InstanceLabels

IOU_THRESHOLDS = (0.25, 0.5, 0.7, 0.75)
MAX_CELLS = 1 << 26
_DECODE_THREADS = 4


# ---- 1. ground truth ----------------------------------------------------------------------------------------------------------
def voc_instances(cls_png: np.ndarray, obj_png: np.ndarray, num_cls: int = 20) -> Tuple[np.ndarray, np.ndarray]:
    """cls_png, obj_png: uint8 [H,W], the palette indices of SegmentationClass/ and SegmentationObject/.  Objects are the values
    1..254 of obj_png in ascending order; an object's class is the most frequent value in 1..num_cls of cls_png under it (ties to
    the smaller value) minus 1; an object with no such pixel is dropped.  Returns (G uint8 [H,W]: j on the j-th kept object, 0
    elsewhere, void (255) included; gt_cls int64 [m], m <= 254)."""
    cls_png, obj_png = np.asarray(cls_png), np.asarray(obj_png)
    if cls_png.dtype != np.uint8 or obj_png.dtype != np.uint8 or cls_png.ndim != 2 or cls_png.shape != obj_png.shape:
        raise ValueError(f"voc_instances: two uint8 [H,W] arrays of one size are needed (got {cls_png.dtype} {cls_png.shape}, "
                         f"{obj_png.dtype} {obj_png.shape})")
    if not 1 <= int(num_cls) <= 254:
        raise ValueError(f"voc_instances: num_cls must be in 1..254 (got {num_cls!r})")
    joint = np.bincount(obj_png.reshape(-1).astype(np.int64) * 256 + cls_png.reshape(-1), minlength=65536).reshape(256, 256)
    votes = joint[1:255, 1:int(num_cls) + 1]                                   # [object 1..254, class 1..num_cls]
    best = votes.argmax(1)                                                     # the first maximum: ties to the smaller class
    kept = np.flatnonzero(votes.max(1) > 0)
    lut = np.zeros(256, np.uint8)
    lut[kept + 1] = np.arange(1, kept.size + 1)
    return lut[obj_png], best[kept].astype(np.int64)


# ---- 2. pair table ------------------------------------------------------------------------------------------------------------
def _dev_tensor(what: str, name: str, t, dtypes):
    if not torch.is_tensor(t) or t.dtype not in dtypes:
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{what}: {name} must be a {' or '.join(str(d) for d in dtypes)} tensor (got {got})")
    if not t.is_cuda:
        raise MuscleHipError(f"{what} runs on the HIP kernels only ({name} is on the host)")
    return t.contiguous()


def _outputs(what: str, cells: int, table, bad, dev):
    if cells > MAX_CELLS:
        raise ValueError(f"{what}: the table would have {cells} cells, at most 2^26 are supported")
    if table is None:
        buf = torch.empty(cells + 1, dtype=torch.int32, device=dev)
        table, bad = buf[:cells], buf[cells:]
    for name, t, n in (("table", table, cells), ("bad", bad, 1)):
        if not torch.is_tensor(t) or t.dtype != torch.int32 or t.numel() != n:
            raise ValueError(f"{what}: {name} must be an int32 tensor of {n} elements")
    return table, bad


def label_pair_counts(a: torch.Tensor, b: torch.Tensor, A: int, B: int, table: torch.Tensor = None, bad: torch.Tensor = None):
    """Enqueues mx_label_pair_counts.  a int32 (values 0..A), b uint8 (values 0..B): device tensors of one size.  Returns the device
    tensors (table int32 [(A+1)*(B+1)], bad int32 [1]); handed in, they are overwritten.  Nothing is read back."""
    what = "label_pair_counts"
    a, b = _dev_tensor(what, "a", a, (torch.int32,)), _dev_tensor(what, "b", b, (torch.uint8,))
    if a.shape != b.shape or a.numel() == 0:
        raise ValueError(f"{what}: a is {tuple(a.shape)}, b is {tuple(b.shape)}: one non-empty size is needed")
    if A < 0 or not 0 <= B <= 255:
        raise ValueError(f"{what}: A >= 0 and 0 <= B <= 255 are needed (got A={A}, B={B})")
    table, bad = _outputs(what, (A + 1) * (B + 1), table, bad, a.device)
    call("mx_label_pair_counts", ptr(a), ptr(b), a.numel(), int(A), int(B), ptr(table), ptr(bad), stream())
    return table, bad


def mask_pair_counts(masks: torch.Tensor, b: torch.Tensor, B: int, table: torch.Tensor = None, bad: torch.Tensor = None):
    """Enqueues mx_mask_pair_counts.  masks bool / uint8 [n, ...] (non-zero = set), b uint8 [...] (values 0..B) on the device.
    Returns the device tensors (table int32 [(n+1)*(B+1)], bad int32 [1])."""
    what = "mask_pair_counts"
    masks, b = _dev_tensor(what, "masks", masks, (torch.bool, torch.uint8)), _dev_tensor(what, "b", b, (torch.uint8,))
    if masks.dim() < 1 or masks.shape[1:] != b.shape or b.numel() == 0:
        raise ValueError(f"{what}: masks are {tuple(masks.shape)}, b is {tuple(b.shape)}: [n, ...] over one non-empty size is needed")
    if not 0 <= B <= 255:
        raise ValueError(f"{what}: 0 <= B <= 255 is needed (got {B})")
    n = masks.shape[0]
    if masks.dtype == torch.bool:
        masks = masks.view(torch.uint8)                                        # same bytes: True is 1
    table, bad = _outputs(what, (n + 1) * (B + 1), table, bad, b.device)
    call("mx_mask_pair_counts", ptr(masks) if n else None, ptr(b), b.numel(), n, int(B), ptr(table), ptr(bad), stream())
    return table, bad


def pair_table(pred, G_dev: torch.Tensor, m: Optional[int] = None) -> np.ndarray:
    """The joint-count table int32 [n+1, m+1] of one image as a host array; one synchronising read.
    pred: an `InstanceLabels` (label-map kernel on its seg_map: table[s+1][j] = pixels of segment s on object j, row 0 = pixels
    of no segment), or an IRN dict / a bool or uint8 [n,H,W] tensor or array (mask kernel: row p+1 = mask p by object, row 0 =
    every pixel).  G_dev: uint8 [H,W] on the device (voc_instances), m: its number of objects; without m the table is counted
    over all 256 values and cut after the last object that occurs.  A numpy mask stack is uploaded; tensors must be on the device.
    Raises ValueError on a size mismatch and on a value outside 0..n (seg_map) or 0..m (G)."""
    what = "pair_table"
    G_dev = _dev_tensor(what, "G_dev", G_dev, (torch.uint8,))
    if G_dev.dim() != 2 or G_dev.numel() == 0:
        raise ValueError(f"{what}: G_dev must be a non-empty uint8 [H,W] tensor (got {tuple(G_dev.shape)})")
    B = 255 if m is None else int(m)
    if not 0 <= B <= 255:
        raise ValueError(f"{what}: m must be in 0..255 (got {m!r})")
    if isinstance(pred, InstanceLabels):
        n = len(pred)
        seg_map = _dev_tensor(what, "seg_map", pred.seg_map, (torch.int32,))
        if seg_map.shape != G_dev.shape:
            raise ValueError(f"{what}: the prediction is {tuple(seg_map.shape)}, the ground truth {tuple(G_dev.shape)}")
        launch = lambda table, bad: label_pair_counts(seg_map, G_dev, n, B, table, bad)  # noqa: E731
    else:
        masks = pred["mask"] if isinstance(pred, dict) else pred
        if isinstance(masks, np.ndarray):
            if masks.dtype not in (np.bool_, np.uint8):
                raise ValueError(f"{what}: masks must be bool or uint8 (got {masks.dtype})")
            masks = torch.from_numpy(np.ascontiguousarray(masks).view(np.uint8)).to(G_dev.device)
        masks = _dev_tensor(what, "masks", masks, (torch.bool, torch.uint8))
        if masks.dim() != 3 or masks.shape[1:] != G_dev.shape:
            raise ValueError(f"{what}: the prediction is {tuple(masks.shape)}, the ground truth {tuple(G_dev.shape)}: [n,H,W] is needed")
        n = masks.shape[0]
        launch = lambda table, bad: mask_pair_counts(masks, G_dev, B, table, bad)  # noqa: E731
    cells = (n + 1) * (B + 1)
    if cells > MAX_CELLS:
        raise ValueError(f"{what}: the table would have {cells} cells, at most 2^26 are supported")
    buf = torch.empty(cells + 1, dtype=torch.int32, device=G_dev.device)       # table and bad in one buffer ...
    launch(buf[:-1], buf[-1:])
    host = buf.cpu().numpy()                                                   # ... and the one synchronising read
    if host[cells]:
        raise ValueError(f"{what}: {int(host[cells])} pixels hold a value outside 0..{n} (prediction) or 0..{B} (ground truth)")
    out = host[:cells].reshape(n + 1, B + 1)
    if m is None:
        present = np.flatnonzero(out.sum(0, dtype=np.int64))
        out = out[:, :max(int(present[-1]) if present.size else 0, 0) + 1]
    return np.ascontiguousarray(out)


# ---- 3. IoU -------------------------------------------------------------------------------------------------------------------
def mask_iou(table: np.ndarray, overlapping: bool) -> np.ndarray:
    """float64 [n,m]: I / (A_p + A_g - I) from a pair table [n+1, m+1].  I = table[1:,1:], A_p = the row sums.  A_g: the column
    sums for a label-map table (overlapping=False: every pixel is in exactly one row), row 0 for a mask table (overlapping=True:
    row 0 counts every pixel).  An empty union gives 0."""
    t = np.asarray(table).astype(np.int64)
    if t.ndim != 2 or t.shape[0] < 1 or t.shape[1] < 1:
        raise ValueError(f"mask_iou: a [n+1, m+1] table is needed (got {t.shape})")
    inter = t[1:, 1:]
    a_p = t[1:].sum(1)[:, None]
    a_g = (t[0, 1:] if overlapping else t[:, 1:].sum(0))[None, :]
    union = a_p + a_g - inter
    return np.where(union > 0, inter / np.maximum(union, 1), 0.0)


# ---- 4. AP --------------------------------------------------------------------------------------------------------------------
def average_precision(score: np.ndarray, tp: np.ndarray, n_pos: int) -> float:
    """The area under the precision envelope of one class.  score, tp [k] in pooled order (order of add, then the per-image
    order); sorted here by descending score with a stable sort.  n_pos == 0 gives nan; no prediction gives 0."""
    if n_pos == 0:
        return float("nan")
    order = np.argsort(-np.asarray(score, np.float64), kind="stable")
    hit = np.asarray(tp, bool)[order]
    ctp = np.cumsum(hit).astype(np.float64)
    cfp = np.cumsum(~hit).astype(np.float64)
    mrec = np.concatenate([[0.0], ctp / n_pos, [1.0]])
    mpre = np.concatenate([[0.0], ctp / np.maximum(ctp + cfp, 1.0), [0.0]])
    mpre = np.maximum.accumulate(mpre[::-1])[::-1]
    i = np.flatnonzero(mrec[1:] != mrec[:-1])
    return float(np.sum((mrec[i + 1] - mrec[i]) * mpre[i + 1]))


class InsSegEval:
    """Accumulates the matches of the evaluation images; .result() gives {'ap': float64 [T,num_cls], 'map': float64 [T]}."""

    def __init__(self, device, num_cls: int = 20, iou_thresholds: Sequence[float] = IOU_THRESHOLDS):
        self.device = device
        self.num_cls = int(num_cls)
        self.iou_thresholds = tuple(float(t) for t in iou_thresholds)
        if self.num_cls < 1 or not self.iou_thresholds:
            raise ValueError("InsSegEval: num_cls >= 1 and at least one IoU threshold are needed")
        self.n_pos = np.zeros(self.num_cls, np.int64)
        self._score: List[List[np.ndarray]] = [[] for _ in range(self.num_cls)]
        self._tp: List[List[List[np.ndarray]]] = [[[] for _ in range(self.num_cls)] for _ in self.iou_thresholds]

    def add(self, pred, cls_png: np.ndarray, obj_png: np.ndarray) -> None:
        """pred: an `InstanceLabels` or an IRN dict {'score','mask','class'} (scores and classes are taken from it)."""
        if isinstance(pred, InstanceLabels):
            score, cls = pred.score, pred.cls
        elif isinstance(pred, dict):
            score, cls = pred["score"], pred["class"]
        else:
            raise ValueError(f"InsSegEval.add: an InstanceLabels or an IRN dict is needed (got {type(pred).__name__})")
        G, gt_cls = voc_instances(cls_png, obj_png, self.num_cls)
        table = pair_table(pred, torch.from_numpy(G).to(self.device), gt_cls.size)
        self.add_iou(mask_iou(table, not isinstance(pred, InstanceLabels)), score, cls, gt_cls)

    def add_iou(self, iou: np.ndarray, score, cls, gt_cls) -> None:
        """One image from its IoU matrix [n,m], the predictions' scores and 0-based classes [n] and the objects' classes [m]."""
        iou = np.asarray(iou, np.float64)
        score, cls, gt_cls = np.asarray(score, np.float64), np.asarray(cls, np.int64), np.asarray(gt_cls, np.int64)
        if iou.shape != (score.size, gt_cls.size) or cls.shape != score.shape:
            raise ValueError(f"InsSegEval: an IoU matrix {iou.shape} does not fit {score.size} predictions and {gt_cls.size} objects")
        for v in (cls, gt_cls):
            if v.size and (v.min() < 0 or v.max() >= self.num_cls):
                raise ValueError(f"InsSegEval: a class index outside 0..{self.num_cls - 1}")
        self.n_pos += np.bincount(gt_cls, minlength=self.num_cls)
        for c in np.unique(cls):
            p = np.flatnonzero(cls == c)
            p = p[np.argsort(-score[p], kind="stable")]                        # descending score, ties by ascending index
            g = np.flatnonzero(gt_cls == c)
            self._score[c].append(score[p])
            if g.size:
                best = iou[np.ix_(p, g)].argmax(1)                             # the first arg-max
                best_iou = iou[p, g[best]]
            for ti, t in enumerate(self.iou_thresholds):
                tp = np.zeros(p.size, bool)
                if g.size:
                    taken = np.zeros(g.size, bool)
                    for k in range(p.size):
                        if best_iou[k] >= t and not taken[best[k]]:
                            taken[best[k]] = tp[k] = True
                self._tp[ti][c].append(tp)

    def result(self):
        T = len(self.iou_thresholds)
        ap = np.full((T, self.num_cls), np.nan)
        for c in range(self.num_cls):
            score = np.concatenate(self._score[c]) if self._score[c] else np.zeros(0)
            for ti in range(T):
                tp = np.concatenate(self._tp[ti][c]) if self._tp[ti][c] else np.zeros(0, bool)
                ap[ti, c] = average_precision(score, tp, int(self.n_pos[c]))
        valid = ~np.isnan(ap)
        mean = np.where(valid.any(1), np.where(valid, ap, 0.0).sum(1) / np.maximum(valid.sum(1), 1), np.nan)
        return {"ap": ap, "map": mean}

    def lines(self) -> List[str]:
        """One "<t>iou: {'ap': ..., 'map': ...}" line per threshold (IRN's eval_ins_seg prints these)."""
        r = self.result()
        return [f"{t}iou: " + str({"ap": r["ap"][i], "map": float(r["map"][i])}) for i, t in enumerate(self.iou_thresholds)]


# ---- script -------------------------------------------------------------------------------------------------------------------
def read_gt_pngs(voc12_root: str, name: str) -> Tuple[np.ndarray, np.ndarray]:
    """(SegmentationClass/<name>.png, SegmentationObject/<name>.png) as uint8 palette indices."""
    import PIL.Image
    return tuple(np.asarray(PIL.Image.open(os.path.join(voc12_root, d, name + ".png")), dtype=np.uint8)
                 for d in ("SegmentationClass", "SegmentationObject"))


def _decode(voc12_root: str, ins_seg_dir: str, name: str):
    cls_png, obj_png = read_gt_pngs(voc12_root, name)
    path = os.path.join(ins_seg_dir, name + ".npy")
    if not os.path.exists(path):
        print(f"[muscle_amd] {path}: no prediction file, the image counts as having no predictions", file=sys.stderr)
        pred = {"score": np.zeros(0, np.float32), "mask": np.zeros((0,) + cls_png.shape, bool), "class": np.zeros(0, np.int64)}
    else:
        pred = np.load(path, allow_pickle=True).item()
    return pred, cls_png, obj_png


def _prefetched(names: List[str], voc12_root: str, ins_seg_dir: str, ahead: int = 2 * _DECODE_THREADS):
    """Yields (pred, cls_png, obj_png) per name; the next files are read and decoded on a small thread pool while the caller
    counts the current image on the GPU.  The pool only reads and decodes files."""
    from concurrent.futures import ThreadPoolExecutor
    with ThreadPoolExecutor(max_workers=_DECODE_THREADS) as pool:
        pending = [pool.submit(_decode, voc12_root, ins_seg_dir, n) for n in names[:ahead]]
        for i in range(len(names)):
            if i + ahead < len(names):
                pending.append(pool.submit(_decode, voc12_root, ins_seg_dir, names[i + ahead]))
            yield pending.pop(0).result()


def check_gt_files(voc12_root: str, names: List[str]) -> None:
    for n in names:
        for d in ("SegmentationObject", "SegmentationClass"):
            p = os.path.join(voc12_root, d, n + ".png")
            if not os.path.exists(p):
                raise FileNotFoundError(f"{p} is missing: instance evaluation needs the {d} PNG of every listed image")


def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.ins_eval", description=__doc__.split("\n")[0])
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--list", required=True, type=str, help="image names, one per line")
    ap.add_argument("--ins_seg_dir", required=True, type=str, help="<name>.npy dicts of infer_irn --ins_seg_out_dir")
    ap.add_argument("--iou", default=list(IOU_THRESHOLDS), type=float, nargs="+")
    ap.add_argument("--num_classes", default=20, type=int)
    return ap.parse_args(argv)


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    from .infer_seg import read_names
    names = list(read_names(args.list))
    check_gt_files(args.voc12_root, names)
    ev = InsSegEval(torch.device("cuda:0"), args.num_classes, args.iou)
    for pred, cls_png, obj_png in _prefetched(names, args.voc12_root, args.ins_seg_dir):
        ev.add(pred, cls_png, obj_png)
    for line in ev.lines():
        print(line, flush=True)
    return 0


if __name__ == "__main__":
    sys.exit(main())
