"""Class-balanced self-training labels: the step between `infer_seg --out_seg` and a second `train_muscle --mask_type label`
round that drops the pixels the model is not sure of (CBST, Zou et al., ECCV 2018: keep the most confident portion of the
pixels of EACH predicted class, one threshold per class taken over the whole list).

The confidence code (csrc/selflabel.hip, include/muscle_hip.h, DESIGN.md "Self-training labels").  Per pixel of a map
prob fp32 [K,H,W] - the mean map of infer_seg, or the CRF's Q:
  label  best = prob[0], label = 0; for c = 1..K-1: if (prob[c] > best) { best = prob[c]; label = c; }   (the first maximum)
  conf   = best
  code   uint8, a logarithmic code of the uncertainty u = 1.0f - conf (one fp32 subtraction):
           conf is NaN -> 255 (never selected);  u <= 0 (conf >= 1) -> 0;  otherwise clamp((bits(u) >> 20) - 823, 1, 193)
         u = 2^-24 is code 1, u in [0.5, 1) is 185..192, u >= 1 is 193; lower = more confident; 194..254 are unused.
`infer_seg --out_conf DIR` writes the code map beside every label map and the per-class histograms hist[label][code]
(with --gt_dir also val / hit: the pixels with a ground truth, and those whose label it confirms) as DIR/stats.npz.

  python -m muscle_amd.selflabel select --seg_dir SEG --conf_dir DIR --out_dir SELF --portion 0.5
      [--stats F.npz ...] [--min_conf 0.0] [--list LIST] [--gt_dir G] [--num_classes 21]
reads the two PNGs per name and writes SELF/<name>.png, mode L: the class index where the pixel's code is within its
class's threshold, 255 elsewhere - the file `train_muscle --mask_type label --mask_root SELF` reads.

The thresholds, the curve and the files are host integer arithmetic; the code, the tables and the selection exist as HIP
kernels only.
"""
from __future__ import annotations

import argparse
import math
import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from ._lib import MuscleHipError, call, ptr, stream

MAXK = 24               # CONF_MAXK of csrc/selflabel.hip
TOP_CODE = 193          # the least confident code a threshold can take; 255 (NaN) is never selected
NAN_CODE = 255
VERSION = 1


# ---- the code as numpy (printing thresholds as confidences; the device evaluates the same bits) -------------------------------
def code_of(conf) -> np.ndarray:
    """The code of fp32 confidences, any shape (a scalar gives a 0-d array)."""
    conf = np.asarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore"):
        u = np.float32(1.0) - conf
        c = (np.ascontiguousarray(u).reshape(-1).view(np.uint32).reshape(u.shape) >> np.uint32(20)).astype(np.int64) - 823
        code = np.clip(c, 1, TOP_CODE)
        code = np.where(u > 0, code, 0)
    return np.where(np.isnan(conf), NAN_CODE, code).astype(np.uint8)


def code_interval(code: int) -> Tuple[float, float]:
    """(lo, hi): the confidences of `code` lie in (lo, hi], up to the rounding of the fp32 subtraction.  Code 0 is
    [1, inf), code 193 is (-inf, 0], 255 and the unused codes are (nan, nan)."""
    code = int(code)
    if code == 0:
        return 1.0, math.inf
    if code == TOP_CODE:
        return -math.inf, 0.0
    if not 1 <= code < TOP_CODE:
        return math.nan, math.nan
    edge = lambda c: float(np.array([(c + 823) << 20], dtype=np.uint32).view(np.float32)[0])     # noqa: E731
    return 1.0 - edge(code + 1), 1.0 - (edge(code) if code > 1 else 0.0)


# ---- host arithmetic on the tables -------------------------------------------------------------------------------------------
def _table(a, name: str, K: Optional[int] = None) -> np.ndarray:
    a = np.asarray(a)
    if a.ndim != 2 or a.shape[1] != 256 or not 1 <= a.shape[0] <= MAXK or (K is not None and a.shape[0] != K):
        raise ValueError(f"{name} must be an integer table [K,256] with 1 <= K <= {MAXK} (got {a.shape})")
    if a.dtype.kind not in "iu":
        raise ValueError(f"{name} must hold integers (got {a.dtype})")
    a = a.astype(np.int64)
    if (a < 0).any():
        raise ValueError(f"{name} has negative counts")
    return a


def _portions(portion, K: int) -> np.ndarray:
    p = np.asarray(portion, dtype=np.float64)
    if p.ndim == 0:
        p = np.full(K, float(p))
    if p.shape != (K,):
        raise ValueError(f"portion must be a float or a [{K}] array (got shape {p.shape})")
    if not np.all((p > 0) & (p <= 1)):
        raise ValueError(f"portion must lie in (0, 1] (got {p.tolist() if K > 1 else float(p[0])})")
    return p


def thresholds(hist, portion, min_conf: Optional[float] = None) -> np.ndarray:
    """uint8 [K]: per class the smallest code t whose cumulative count reaches
    need = min(n_c, max(1, ceil(portion_c * n_c))), n_c = hist[c].sum().  Ties inside one code are all kept, so at least the
    portion is kept; an empty class gets 0; t is capped at 193 (code 255 is never reachable).  min_conf lowers every
    threshold to at most the code of 1 - min_conf."""
    hist = _table(hist, "hist")
    K = hist.shape[0]
    p = _portions(portion, K)
    cap = TOP_CODE
    if min_conf is not None:
        if not float(min_conf) <= 1.0:                     # also a NaN
            raise ValueError(f"min_conf must be at most 1 (got {min_conf})")
        cap = min(cap, int(code_of(np.float32(min_conf))))
    t = np.zeros(K, dtype=np.uint8)
    for c in range(K):
        n_c = int(hist[c].sum())
        if n_c == 0:
            continue
        need = min(n_c, max(1, math.ceil(float(p[c]) * n_c)))
        cum = np.cumsum(hist[c, :TOP_CODE + 1])
        t[c] = min(int(np.searchsorted(cum, need, side="left")), cap)
    return t


def kept_counts(table, tcode) -> np.ndarray:
    """int64 [K]: the entries of an integer table [K,256] within the thresholds."""
    table = _table(table, "table")
    tcode = np.asarray(tcode).astype(np.int64)
    if tcode.shape != (table.shape[0],):
        raise ValueError(f"tcode must be [{table.shape[0]}] (got {tcode.shape})")
    return np.array([table[c, :min(int(tcode[c]), TOP_CODE) + 1].sum() for c in range(table.shape[0])], dtype=np.int64)


def quality_curve(hist, val, hit, portions: Sequence[float]) -> Dict[str, np.ndarray]:
    """The thresholds of every portion and what they keep.  With P portions: portion [P], tcode uint8 [P,K], total int64
    [K] and kept / val / hit int64 [P,K] (pixels, pixels with a ground truth, pixels whose label it confirms, all within the
    threshold), coverage [P,K] = kept / total and precision [P,K] = hit / val (nan where the divisor is 0), coverage_all [P]
    = kept / total over all classes, mean_precision [P] = the mean over the classes that keep valid pixels (nan if none).
    Integers up to the final float64 division."""
    hist = _table(hist, "hist")
    K = hist.shape[0]
    val, hit = _table(val, "val", K), _table(hit, "hit", K)
    ps = [float(p) for p in portions]
    tc = np.stack([thresholds(hist, p) for p in ps]) if ps else np.zeros((0, K), np.uint8)
    total = hist.sum(1)
    kept, kv, kh = (np.stack([kept_counts(t, row) for row in tc]) if ps else np.zeros((0, K), np.int64) for t in (hist, val, hit))
    with np.errstate(invalid="ignore", divide="ignore"):
        cov = np.where(total > 0, kept / np.maximum(total, 1).astype(np.float64), np.nan)
        prec = np.where(kv > 0, kh / np.maximum(kv, 1).astype(np.float64), np.nan)
        cov_all = kept.sum(1) / np.float64(total.sum()) if total.sum() else np.full(len(ps), np.nan)
    mean_prec = np.array([np.nan if not (kv[i] > 0).any() else prec[i][kv[i] > 0].mean() for i in range(len(ps))], dtype=np.float64)
    return {"portion": np.array(ps, dtype=np.float64), "tcode": tc, "total": total, "kept": kept, "val": kv, "hit": kh,
            "coverage": cov, "coverage_all": np.asarray(cov_all, dtype=np.float64), "precision": prec, "mean_precision": mean_prec}


def curve_lines(curve: Dict[str, np.ndarray]) -> List[str]:
    """The quality curve as printed by `infer_seg --out_conf --gt_dir`."""
    out = ["portion  coverage  mean precision of the kept labels"]
    for p, c, m in zip(curve["portion"], curve["coverage_all"], curve["mean_precision"]):
        out.append("%7.2f  %7.3f%%  %7.3f%%" % (p, 100 * c, 100 * m))
    return out


# ---- the device side ---------------------------------------------------------------------------------------------------------
def _check_map(t, name: str, shape=None) -> None:
    if not torch.is_tensor(t) or t.dtype != torch.uint8 or t.dim() < 1 or t.numel() < 1 or (shape is not None and tuple(t.shape) != tuple(shape)):
        want = f"uint8 {list(shape)}" if shape is not None else "a non-empty uint8 tensor"
        got = f"{t.dtype} {tuple(t.shape)}" if torch.is_tensor(t) else type(t).__name__
        raise ValueError(f"{name} must be {want} (got {got})")
    if t.numel() >= 2 ** 31:
        raise ValueError(f"{name} has {t.numel()} pixels; the kernels take fewer than 2^31")


def _check_k(K: int) -> int:
    if not 1 <= int(K) <= MAXK:
        raise ValueError(f"the kernels take 1..{MAXK} classes (got {K})")
    return int(K)


def _on_device(*ts) -> torch.device:
    dev = None
    for t in ts:
        if t is None:
            continue
        if not t.is_cuda:
            raise MuscleHipError("muscle_amd.selflabel runs on the HIP kernels only; there is no CPU path")
        if dev is not None and t.device != dev:
            raise ValueError(f"tensors on different devices ({dev}, {t.device})")
        dev = t.device
    return dev


class ConfStats:
    """The tables hist / val / hit int64 [K][256] of a run, resident on `device`.  add / add_coded only enqueue: nothing is
    read back until tables() or save()."""

    def __init__(self, device, num_cls: int = 21):
        self.num_cls = _check_k(num_cls)
        self.device = torch.device(device)
        self._t = torch.zeros(3, self.num_cls, 256, dtype=torch.int64, device=self.device)

    hist = property(lambda self: self._t[0])
    val = property(lambda self: self._t[1])
    hit = property(lambda self: self._t[2])

    def add(self, prob: torch.Tensor, gt: Optional[torch.Tensor] = None) -> Tuple[torch.Tensor, torch.Tensor]:
        """From a probability map [K,H,W]; returns (label, code)."""
        return conf_code(prob, gt, self)

    def add_coded(self, label: torch.Tensor, code: torch.Tensor, gt: Optional[torch.Tensor] = None) -> None:
        """From a stored (label, code) pair; a label >= num_cls is counted nowhere."""
        _check_map(label, "label")
        _check_map(code, "code", label.shape)
        if gt is not None:
            _check_map(gt, "gt", label.shape)
        dev = _on_device(label, code, gt, self._t)
        with torch.cuda.device(dev):
            call("mx_code_hist", ptr(label.contiguous()), ptr(code.contiguous()), ptr(gt.contiguous()) if gt is not None else None,
                 label.numel(), self.num_cls, ptr(self.hist), ptr(self.val) if gt is not None else None,
                 ptr(self.hit) if gt is not None else None, stream())

    def tables(self) -> Tuple[np.ndarray, np.ndarray, np.ndarray]:
        t = self._t.cpu().numpy()
        return t[0], t[1], t[2]

    def save(self, path: str) -> None:
        hist, val, hit = self.tables()
        np.savez(path, version=np.int32(VERSION), hist=hist, val=val, hit=hit)

    @classmethod
    def load(cls, *paths: str, device="cpu") -> "ConfStats":
        """The sum of several stats files (a sharded infer_seg run).  The result lives on `device`; on the host it serves
        tables() / save() only."""
        if not paths:
            raise ValueError("ConfStats.load needs at least one file")
        total = None
        for path in paths:
            with np.load(path, allow_pickle=False) as z:
                if any(k not in z.files for k in ("version", "hist", "val", "hit")) or int(z["version"]) != VERSION:
                    raise ValueError(f"{path}: not a confidence-statistics file of version {VERSION}")
                t = np.stack([_table(z[k], f"{path}: {k}") for k in ("hist", "val", "hit")])
            if total is not None and t.shape != total.shape:
                raise ValueError(f"{path}: {t.shape[1]} classes, the files before it {total.shape[1]}")
            total = t if total is None else total + t
        st = cls(device, total.shape[1])
        st._t.copy_(torch.from_numpy(total))
        return st


def conf_code(prob: torch.Tensor, gt: Optional[torch.Tensor] = None, stats: Optional[ConfStats] = None
              ) -> Tuple[torch.Tensor, torch.Tensor]:
    """prob fp32 [K,H,W] on the device -> (label, code) uint8 [H,W] (mx_conf_code).  stats: its hist is added to, and with
    gt (uint8 [H,W], 255 = ignore) its val and hit."""
    if not torch.is_tensor(prob) or prob.dtype != torch.float32 or prob.dim() != 3 or prob.numel() < 1:
        got = f"{prob.dtype} {tuple(prob.shape)}" if torch.is_tensor(prob) else type(prob).__name__
        raise ValueError(f"prob must be float32 [K,H,W] (got {got})")
    K, H, W = prob.shape
    _check_k(K)
    if H * W >= 2 ** 31:
        raise ValueError(f"H*W = {H * W}; the kernel takes fewer than 2^31 pixels")
    if gt is not None:
        _check_map(gt, "gt", (H, W))
    if stats is not None and stats.num_cls != K:
        raise ValueError(f"prob has {K} channels, stats {stats.num_cls} classes")
    dev = _on_device(prob, gt, stats._t if stats is not None else None)
    label = torch.empty(H, W, dtype=torch.uint8, device=dev)
    code = torch.empty(H, W, dtype=torch.uint8, device=dev)
    t = stats._t if stats is not None else torch.zeros(3 if gt is not None else 1, K, 256, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        call("mx_conf_code", ptr(prob.contiguous()), K, H, W, ptr(label), ptr(code), ptr(gt.contiguous()) if gt is not None else None,
             ptr(t[0]), ptr(t[1]) if gt is not None else None, ptr(t[2]) if gt is not None else None, stream())
    return label, code


def select(label: torch.Tensor, code: torch.Tensor, tcode) -> Tuple[torch.Tensor, torch.Tensor]:
    """out = the label where label < K and code <= tcode[label], 255 elsewhere (uint8, the shape of label); kept int64 [K,2]
    = (kept, total) per class, on the device (mx_conf_select).  tcode: uint8 [K], a numpy array or a tensor."""
    _check_map(label, "label")
    _check_map(code, "code", label.shape)
    if torch.is_tensor(tcode):
        if tcode.dtype != torch.uint8 or tcode.dim() != 1:
            raise ValueError(f"tcode must be uint8 [K] (got {tcode.dtype} {tuple(tcode.shape)})")
    else:
        tcode = np.asarray(tcode)
        if tcode.dtype != np.uint8 or tcode.ndim != 1:
            raise ValueError(f"tcode must be uint8 [K] (got {tcode.dtype} {tcode.shape})")
    K = _check_k(tcode.shape[0])
    dev = _on_device(label, code)
    tc = tcode.to(dev) if torch.is_tensor(tcode) else torch.from_numpy(np.ascontiguousarray(tcode)).to(dev)
    out = torch.empty_like(label, memory_format=torch.contiguous_format)
    kept = torch.zeros(K, 2, dtype=torch.int64, device=dev)
    with torch.cuda.device(dev):
        call("mx_conf_select", ptr(label.contiguous()), ptr(code.contiguous()), ptr(tc.contiguous()), label.numel(), K, ptr(out),
             ptr(kept), stream())
    return out, kept


# ---- the script ----------------------------------------------------------------------------------------------------------------
def parse_args(argv: Optional[List[str]] = None):
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.selflabel", description=__doc__.split("\n")[0])
    sub = ap.add_subparsers(dest="cmd", required=True)
    sp = sub.add_parser("select", help="write the class-balanced self-training label maps of an infer_seg --out_seg / --out_conf run")
    sp.add_argument("--seg_dir", required=True, help="the --out_seg directory: <name>.png label maps")
    sp.add_argument("--conf_dir", required=True, help="the --out_conf directory: <name>.png code maps (and stats.npz)")
    sp.add_argument("--out_dir", required=True, help="where <name>.png (class index or 255) is written")
    sp.add_argument("--portion", required=True, type=float, help="the portion of every predicted class to keep, in (0, 1]")
    sp.add_argument("--stats", nargs="+", default=None, help="statistics files to sum (default: CONF_DIR/stats.npz; if there is "
                    "none, the histograms are counted from the files first)")
    sp.add_argument("--min_conf", default=0.0, type=float, help="keep no pixel whose confidence code lies below this confidence's")
    sp.add_argument("--list", default=None, help="image list (one name or VOC path per line); default: every .png of SEG_DIR")
    sp.add_argument("--gt_dir", default=None, help="SegmentationClass directory: also print the precision of the kept pixels")
    sp.add_argument("--num_classes", default=21, type=int, help="used when the histograms are counted from the files")
    args = ap.parse_args(argv)
    if not 0.0 < args.portion <= 1.0:
        ap.error(f"--portion {args.portion}: must lie in (0, 1]")
    if not args.min_conf <= 1.0:
        ap.error(f"--min_conf {args.min_conf}: must be at most 1")
    if not 1 <= args.num_classes <= MAXK:
        ap.error(f"--num_classes {args.num_classes}: the kernels take 1..{MAXK}")
    return args


def _read_png(path: str) -> np.ndarray:
    import PIL.Image
    a = np.array(PIL.Image.open(path))
    if a.ndim != 2 or a.dtype != np.uint8:
        raise ValueError(f"{path}: not an 8-bit single-channel image ({a.dtype} {a.shape})")
    return a


def run_select(args, device="cuda:0") -> int:
    from .infer import save_seg_png
    from .infer_seg import read_names
    if args.list:
        names = read_names(args.list)
    else:
        names = sorted(f[:-4] for f in os.listdir(args.seg_dir) if f.endswith(".png"))
    dirs = [args.seg_dir, args.conf_dir] + ([args.gt_dir] if args.gt_dir else [])
    for name in names:                                     # before the loop: a missing file is an error that names it
        for d in dirs:
            if not os.path.isfile(os.path.join(d, name + ".png")):
                raise FileNotFoundError(os.path.join(d, name + ".png"))
    stats_paths = args.stats
    if stats_paths is None and os.path.isfile(os.path.join(args.conf_dir, "stats.npz")):
        stats_paths = [os.path.join(args.conf_dir, "stats.npz")]
    for p in stats_paths or []:
        if not os.path.isfile(p):
            raise FileNotFoundError(p)
    dev = torch.device(device)

    def load(name):
        lab, code = _read_png(os.path.join(args.seg_dir, name + ".png")), _read_png(os.path.join(args.conf_dir, name + ".png"))
        if lab.shape != code.shape:
            raise ValueError(f"{name}: the label map is {lab.shape}, the code map {code.shape}")
        gt = None
        if args.gt_dir:
            gt = _read_png(os.path.join(args.gt_dir, name + ".png"))
            if gt.shape != lab.shape:
                raise ValueError(f"{name}: the label map is {lab.shape}, the ground truth {gt.shape}")
        return [None if a is None else torch.from_numpy(a).to(dev) for a in (lab, code, gt)]

    if stats_paths:
        stats = ConfStats.load(*stats_paths)
    else:
        stats = ConfStats(dev, args.num_classes)
        for name in names:
            lab, code, _ = load(name)
            stats.add_coded(lab, code)
    K = stats.num_cls
    hist = stats.tables()[0]
    tcode = thresholds(hist, args.portion, args.min_conf)
    tc_dev = torch.from_numpy(tcode).to(dev)
    os.makedirs(args.out_dir, exist_ok=True)
    kept = torch.zeros(K, 2, dtype=torch.int64, device=dev)
    kstats = ConfStats(dev, K) if args.gt_dir else None    # the kept pixels alone against the ground truth
    for it, name in enumerate(names):
        lab, code, gt = load(name)
        out, k = select(lab, code, tc_dev)
        kept += k
        if kstats is not None:
            kstats.add_coded(out, code, gt)
        save_seg_png(os.path.join(args.out_dir, name + ".png"), out)
        print(name, it, flush=True)
    kept = kept.cpu().numpy()
    from .evaluation import categories
    if kstats is not None:
        _, kv, kh = kstats.tables()
        kv, kh = kv.sum(1), kh.sum(1)
    for c in range(K):
        nm = categories[c] if c < len(categories) else str(c)
        lo, hi = code_interval(int(tcode[c]))
        # the least confident code kept holds the confidences (lo, hi]: everything above lo is kept
        line = "%11s: code <= %3d, conf in (%.8f, %.8f] and above  kept %d / %d" % (nm, tcode[c], lo, hi, kept[c, 0], kept[c, 1])
        if kstats is not None:
            line += "  precision " + ("%7.3f%% (%d / %d)" % (100.0 * kh[c] / kv[c], kh[c], kv[c]) if kv[c] else "-")
        print(line)
    print("%11s: kept %d / %d" % ("all", kept[:, 0].sum(), kept[:, 1].sum()), flush=True)
    return len(names)


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    run_select(args)
    return 0


if __name__ == "__main__":
    sys.exit(main())
