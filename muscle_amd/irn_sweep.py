"""`python -m muscle_amd.irn_sweep`: mIoU of infer_irn's pseudo-labels over the whole (--beta, --exp_times, --sem_seg_bg_thres)
grid, from one pass over the list.  IRN's workflow picks the three knobs by mIoU against SegmentationClass on train.txt; done
with the scripts that is one `infer_irn` run plus one `evaluation --type png` run per grid point.  Here each image costs one
network forward, one walk per beta and one counting launch per beta; no label map, soft label or file is produced.

The rule.  For an image with ground truth gt and every (beta b, exp_times e, threshold t) of the grid the table holds exactly
the counts of this chain, integer for integer:

    down  = ops.resize_planar_halfpixel(cam_stack(cam_dict, H, W), h, w)
    rw    = indexing.propagate_to_edge(down, edge, beta=b, exp_times=e, radius=5, method="stencil")
    label = indexing.finish_semseg(rw, H, W, t)
    mx_seg_confusion(label, gt)   ->  counts[b][e][t][k] = (TP, P, T), int64, accumulated over images

How it is cheaper.  (1) The stencil walk reaches 2^e steps through every smaller power of two on its fp64 state, so one walk to
the largest exp_times passes through the state of every smaller one; `mx_irn_walk_snap` writes those states, each bit for bit
the result of a separate walk.  (2) Only the channels present in the dict are walked: an absent channel stays exactly 0, never
beats a threshold >= 0 and does not change the maximum.  (3) The winner among the channels does not depend on the threshold, so
a pixel is described by its bin #{t_i < best value}: `mx_irn_sweep_confusion` counts all thresholds of all snapshots in one
launch with at most three integer atomics per pixel (the bin argument of `evaluation --curve`).  A tie value == threshold is
background, as in the label kernel; an all-zero walk result (values 0 / 0) is background at every threshold.  The maximum each
snapshot is divided by comes from the label step's own kernel (`mx_irn_up_max`) run on the full 20-channel stack, as
`finish_semseg` runs it: one kernel forms the word every consumer divides by, so the sweep takes the word from it.

The sweep scores the STENCIL walk (`infer_irn --walk stencil`).  The dense walk (`--walk dense`, exp_times fp32 squarings of
the matrix) is a different fp32 computation of the same quantity and can differ from it in a few pixels per image.

Grid limits (ValueError before anything is launched): betas - finite, 0 < beta <= 64, no duplicates (an integral beta is an
exact repeated multiplication, any other goes through powf, as in the walk); exp_times - integers 0..12, strictly ascending;
thresholds - 1..64 values, >= 0, ascending; num_cls 2..24.

`--from_soft DIR` is the thresholds-only sweep of the compact soft labels `infer_irn --soft_output 2` wrote (the beta and
exp_times are the ones that run used): no network, no CAMs.  infer_irn writes no file for an image whose walk result is all
zero; such an image is named on stderr and counted as all background, which is what its PNG holds.
"""
from __future__ import annotations

import os
import sys
from typing import Dict, List, Optional, Sequence, Tuple

import numpy as np

DEFAULT_BETAS = (6, 8, 10, 12)
DEFAULT_EXP_TIMES = (4, 5, 6, 7, 8)
DEFAULT_THRESHOLDS = tuple(round(0.15 + 0.02 * i, 2) for i in range(20))         # 0.15 .. 0.53
RADIUS = 5                                                                        # infer_irn.py:77


def check_grid(betas, exp_times, thresholds, num_cls: int = 21):
    """The grid as tuples, or ValueError (see the module docstring for the ranges).  Touches no device."""
    import math
    from .evaluation import check_thresholds
    from .indexing import check_exp_times_list
    bs = tuple(float(b) for b in betas)
    if not bs:
        raise ValueError("irn_sweep: betas is empty")
    if any(not math.isfinite(b) or not 0 < b <= 64 for b in bs):
        raise ValueError(f"irn_sweep: every beta must be finite and in (0, 64] (got {list(bs)})")
    if len(set(bs)) != len(bs):
        raise ValueError(f"irn_sweep: duplicate beta in {list(bs)}")
    ets = check_exp_times_list(exp_times)
    return bs, ets, check_thresholds(thresholds, num_cls, "irn_sweep")


def best_of(mious: np.ndarray) -> Tuple[int, int, int]:
    """(b, e, t) of the largest entry of mious [B,E,T]; ties break toward the lowest index in grid order (b, then e, then t)."""
    m = np.asarray(mious, dtype=np.float64)
    return tuple(int(i) for i in np.unravel_index(int(np.argmax(m)), m.shape))


class IrnSweep:
    """Accumulates the int64 (TP, P, T) table [B,E,T,num_cls,3] of the grid betas x exp_times x thresholds on the device.
    Per image and beta: one mx_irn_walk_weights, one mx_irn_walk_snap, the maxima, one mx_irn_sweep_confusion.  Nothing
    synchronises per image; `counts()` reads the table once."""

    def __init__(self, device, betas: Sequence[float] = DEFAULT_BETAS, exp_times: Sequence[int] = DEFAULT_EXP_TIMES,
                 thresholds: Sequence[float] = DEFAULT_THRESHOLDS, num_cls: int = 21, _thresholds_only: bool = False):
        import torch
        if _thresholds_only:
            _, _, self.thresholds = check_grid((1,), (0,), thresholds, num_cls)
            self.betas, self.exp_times = (None,), (None,)
        else:
            self.betas, self.exp_times, self.thresholds = check_grid(betas, exp_times, thresholds, num_cls)
        self.num_cls = int(num_cls)
        self.dev = torch.device(device)
        self.thr = torch.tensor(self.thresholds, dtype=torch.float32, device=self.dev)
        self.table = torch.zeros(len(self.betas), len(self.exp_times), len(self.thresholds), self.num_cls, 3, dtype=torch.int64,
                                 device=self.dev)
        self._vmax: List[Tuple[Optional[str], "torch.Tensor"]] = []        # per image: the maxima, read only by all_zero_names()

    @classmethod
    def thresholds_only(cls, device, thresholds: Sequence[float] = DEFAULT_THRESHOLDS, num_cls: int = 21) -> "IrnSweep":
        """The B = E = 1 sweep `add_compact` feeds: the beta and exp_times are whatever produced the compact labels."""
        return cls(device, thresholds=thresholds, num_cls=num_cls, _thresholds_only=True)

    # ---- feeding -----------------------------------------------------------------------------------------------------------
    def _gt(self, gt, H: int, W: int):
        import torch
        from ._lib import MuscleHipError
        if torch.is_tensor(gt):
            if not gt.is_cuda:
                raise MuscleHipError("IrnSweep: gt is a host tensor; the sweep runs on the HIP kernels only (pass a device tensor or a numpy array)")
            g = gt
        else:
            g = torch.from_numpy(np.ascontiguousarray(gt)).to(self.dev)
        if g.dtype != torch.uint8 or tuple(g.shape) != (H, W):
            raise ValueError(f"gt must be uint8 [{H},{W}] (got {g.dtype} {tuple(g.shape)})")
        return g.contiguous()

    def _need_device(self, what: str) -> None:
        from ._lib import MuscleHipError
        if self.dev.type != "cuda":
            raise MuscleHipError(f"IrnSweep.{what} runs on the HIP kernels only: create it with a ROCm device")

    def _count(self, b: int, rw, keys_t, Kp: int, h: int, w: int, g, H: int, W: int, vmax) -> None:
        from ._lib import call, ptr, stream
        E = len(self.exp_times)
        call("mx_irn_sweep_confusion", ptr(rw), E, Kp, ptr(keys_t), h, w, ptr(g), H, W, ptr(self.thr), len(self.thresholds),
             self.num_cls, ptr(vmax), ptr(self.table[b]), stream())

    def add_field(self, edge, cam_dict: Dict[int, np.ndarray], gt, H: int, W: int, name: Optional[str] = None) -> None:
        """edge: the boundary map [1,h,w] (or [h,w]) of EdgeDisplacement on the device; cam_dict: {class 0..num_cls-2: float
        [H,W]}, the dict infer_mcl writes (may be empty); gt: uint8 [H,W] SegmentationClass map (255 = ignore), a device tensor
        or a numpy array.  Adds the image's counts at every grid point.  `name` only labels the image for all_zero_names()."""
        import torch
        from . import ops
        from ._lib import MuscleHipError, call, ptr, stream
        from .indexing import _path_table
        self._need_device("add_field")
        if self.betas[0] is None:
            raise ValueError("IrnSweep.add_field: this is a thresholds-only sweep (add_compact)")
        if not torch.is_tensor(edge) or not edge.is_cuda:
            raise MuscleHipError("IrnSweep.add_field: edge is a host tensor; the sweep runs on the HIP kernels only")
        H, W = int(H), int(W)
        h, w = edge.shape[-2:]
        if edge.numel() != h * w or H > 4 * h or W > 4 * w or H < 1 or W < 1:
            raise ValueError(f"edge must be [1,h,w] with H <= 4h, W <= 4w (got {tuple(edge.shape)} for {H}x{W})")
        keys = sorted(int(k) for k in cam_dict.keys())
        if keys and (keys[0] < 0 or keys[-1] > self.num_cls - 2 or len(set(keys)) != len(keys)):
            raise ValueError(f"IrnSweep.add_field: class keys {keys} outside 0..{self.num_cls - 2}")
        g = self._gt(gt, H, W)
        B, E, Kp, C = len(self.betas), len(self.exp_times), len(keys), self.num_cls - 1
        vmax = torch.zeros(B, E, dtype=torch.int32, device=self.dev)
        self._vmax.append((name, vmax))
        if Kp == 0:                                                     # cam_stack of an empty dict: zeros, background everywhere
            for b in range(B):
                self._count(b, None, None, 0, h, w, g, H, W, vmax[b])
            return
        cams = np.stack([np.asarray(cam_dict[k]) for k in keys]).astype(np.float32, copy=False)
        if cams.shape != (Kp, H, W):
            raise ValueError(f"IrnSweep.add_field: maps must be [{H},{W}] (got {cams.shape[1:]})")
        with torch.no_grad():
            down = ops.resize_planar_halfpixel(torch.from_numpy(np.ascontiguousarray(cams)).to(self.dev), h, w)
            e = edge.reshape(h, w).contiguous().float()
            table = _path_table(RADIUS, self.dev)
            keys_t = torch.tensor(keys, dtype=torch.int32).to(self.dev)
            keys_l = keys_t.long()
            full = torch.zeros(E, C, h, w, dtype=torch.float32, device=self.dev)     # the stack finish_semseg would see
            steps = [2 ** t for t in self.exp_times]
            for b, beta in enumerate(self.betas):
                Wt, cs = ops.irn_walk_weights(e, table, RADIUS, beta)
                rw = ops.irn_walk_snap(down, e, Wt, cs, table, RADIUS, steps)        # [E,Kp,h,w]
                full.index_copy_(1, keys_l, rw)
                for i in range(E):                                                   # the label step's own maximum kernel and geometry
                    call("mx_irn_up_max", ptr(full[i]), C, h, w, H, W, ptr(vmax[b, i:i + 1]), stream())
                self._count(b, rw, keys_t, Kp, h, w, g, H, W, vmax[b])

    def add(self, model, img_pair, cam_dict, gt, name: Optional[str] = None) -> None:
        """One image as infer_irn takes it: img_pair [2,3,H,W] on the device (image + flip), one EdgeDisplacement forward."""
        from ._lib import MuscleHipError
        if not getattr(img_pair, "is_cuda", False):
            raise MuscleHipError("IrnSweep.add: img_pair is a host tensor; the sweep runs on the HIP kernels only")
        H, W = img_pair.shape[2:]
        edge, _ = model(img_pair)
        self.add_field(edge, cam_dict, gt, H, W, name=name)

    def add_compact(self, cs, gt, name: Optional[str] = None) -> None:
        """cs: a softlabel.CompactSoft (`infer_irn --soft_output 2`), or None for an image infer_irn wrote no file for (an
        all-zero walk result): the thresholds-only sweep, B = E = 1.  The table equals the chain run with the beta and
        exp_times that produced the file.  A CompactSoft with vmax == 0 counts as all background."""
        import torch
        self._need_device("add_compact")
        if len(self.betas) != 1 or len(self.exp_times) != 1:
            raise ValueError("IrnSweep.add_compact: a compact soft label holds one (beta, exp_times): the grid must have B = E = 1")
        g = gt if torch.is_tensor(gt) else torch.from_numpy(np.ascontiguousarray(gt))
        H, W = (int(v) for v in g.shape) if cs is None else cs.size
        g = self._gt(gt, H, W)
        vmax = torch.zeros(1, dtype=torch.int32, device=self.dev)
        self._vmax.append((name, vmax.view(1, 1)))
        if cs is None or float(cs.vmax) == 0 or cs.keys.shape[0] == 0:
            self._count(0, None, None, 0, (H + 3) // 4, (W + 3) // 4, g, H, W, vmax)
            return
        if cs.channels != self.num_cls:
            raise ValueError(f"IrnSweep.add_compact: the label has {cs.channels} channels, the sweep {self.num_cls} classes")
        Kp, h, w = cs.rw.shape
        if H > 4 * h or W > 4 * w or int(cs.keys.max()) > self.num_cls - 2 or np.any(np.diff(cs.keys.astype(np.int32)) <= 0):
            raise ValueError("IrnSweep.add_compact: not a valid compact soft label (size beyond the 4x maps, or keys not ascending)")
        vmax = torch.from_numpy(np.asarray([cs.vmax], dtype=np.float32).view(np.int32)).to(self.dev)
        self._vmax[-1] = (name, vmax.view(1, 1))
        rw = torch.from_numpy(cs.rw).to(self.dev)
        keys_t = torch.from_numpy(cs.keys.astype(np.int32)).to(self.dev)
        self._count(0, rw, keys_t, Kp, h, w, g, H, W, vmax)

    # ---- reading -----------------------------------------------------------------------------------------------------------
    def counts(self) -> np.ndarray:
        """int64 [B,E,T,num_cls,3] = (TP, P, T), one read of the device table."""
        return self.table.cpu().numpy()

    def mious(self) -> np.ndarray:
        """float64 [B,E,T]: loglist(b, e, t)['mIoU'] of every grid point, from one read of the table."""
        from .evaluation import miou_loglist
        c = self.counts()
        B, E, T = c.shape[:3]
        return np.array([[[miou_loglist(c[b, e, t])['mIoU'] for t in range(T)] for e in range(E)] for b in range(B)], dtype=np.float64)

    def loglist(self, b: int, e: int, t: int) -> Dict[str, float]:
        """do_python_eval's return value (src/evaluation.py:56-68) at grid point (b, e, t)."""
        from .evaluation import miou_loglist
        return miou_loglist(self.table[b, e, t].cpu().numpy())

    def best(self):
        """(mIoU, beta, exp_times, threshold) of the best grid point; ties break toward the lowest index in grid order."""
        m = self.mious()
        b, e, t = best_of(m)
        return float(m[b, e, t]), self.betas[b], self.exp_times[e], self.thresholds[t]

    def all_zero_names(self) -> List[Optional[str]]:
        """The `name`s of the images fed so far whose walk result was all zero at some grid point (maximum 0: infer_irn writes
        an all-background PNG, and that is what was counted).  One read for all images."""
        import torch
        if not self._vmax:
            return []
        z = torch.stack([(v == 0).any() for _, v in self._vmax]).cpu().numpy()
        return [n for (n, _), bad in zip(self._vmax, z) if bad]


# ---- python -m muscle_amd.irn_sweep ---------------------------------------------------------------------------------------
def parse_args(argv: Optional[List[str]] = None):
    import argparse
    ap = argparse.ArgumentParser(prog="python -m muscle_amd.irn_sweep", description=__doc__.split("\n")[0])
    ap.add_argument("--irn_weights_name", default=None, type=str, help="IRN checkpoint (a state dict), as for infer_irn")
    ap.add_argument("--cam_dir", default=None, type=str)
    ap.add_argument("--from_soft", default=None, type=str,
                    help="sweep only the thresholds of the compact soft labels <name>.npz in this directory (infer_irn --soft_output 2)")
    ap.add_argument("--voc12_root", default="data/VOC2012", type=str)
    ap.add_argument("--infer_list", default="data/train.txt", type=str)
    ap.add_argument("--gt_dir", default=None, type=str, help="default: <voc12_root>/SegmentationClass")
    ap.add_argument("--betas", default=list(DEFAULT_BETAS), type=float, nargs="+")
    ap.add_argument("--exp_times", default=list(DEFAULT_EXP_TIMES), type=int, nargs="+")
    ap.add_argument("--thresholds", default=list(DEFAULT_THRESHOLDS), type=float, nargs="+")
    ap.add_argument("--out_table", default=None, type=str, help="write the int64 [B,E,T,21,3] (TP, P, T) table here as .npy")
    ap.add_argument("--logfile", default=None, type=str, help="append the best grid point's IoU table here")
    args = ap.parse_args(argv)
    if args.from_soft is None and (args.irn_weights_name is None or args.cam_dir is None):
        ap.error("give --irn_weights_name and --cam_dir (the grid sweep), or --from_soft (the thresholds-only sweep)")
    if args.from_soft is not None and (args.irn_weights_name is not None or args.cam_dir is not None):
        ap.error("--from_soft sweeps stored walk results: it takes no --irn_weights_name / --cam_dir")
    try:
        check_grid((1,) if args.from_soft else args.betas, (0,) if args.from_soft else args.exp_times, args.thresholds)
    except ValueError as e:
        ap.error(str(e))
    if args.gt_dir is None:
        args.gt_dir = os.path.join(args.voc12_root, "SegmentationClass")
    return args


def _fmt(v) -> str:
    return "%g" % v


def infer_irn_arguments(beta, exp_times, threshold) -> str:
    """The best grid point as the arguments of `python -m muscle_amd.infer_irn`."""
    return f"--beta {_fmt(beta)} --exp_times {exp_times} --sem_seg_bg_thres {_fmt(threshold)} --walk stencil"


def check_files(paths: Sequence[str]) -> None:
    for p in paths:
        if not os.path.isfile(p):
            raise FileNotFoundError(f"irn_sweep: {p} is missing")


def main(argv: Optional[List[str]] = None) -> int:
    args = parse_args(argv)
    import PIL.Image
    import torch
    from .evaluation import writelog
    from .infer_seg import read_names
    dev = torch.device("cuda:0")
    names = list(read_names(args.infer_list))
    gt_path = lambda n: os.path.join(args.gt_dir, n + ".png")  # noqa: E731
    gt_of = lambda n: np.ascontiguousarray(np.array(PIL.Image.open(gt_path(n))), dtype=np.uint8)  # noqa: E731
    check_files([gt_path(n) for n in names])
    if args.from_soft is not None:
        from .softlabel import load_compact
        sw = IrnSweep.thresholds_only(dev, args.thresholds)
        for n in names:
            p = os.path.join(args.from_soft, n + ".npz")
            sw.add_compact(load_compact(p) if os.path.isfile(p) else None, gt_of(n), name=n)
    else:
        from .data import MSFStager
        from .infer import load_cam_dict
        from .irn import EdgeDisplacement
        check_files([os.path.join(args.cam_dir, n + ".npy") for n in names] +
                    [os.path.join(args.voc12_root, "JPEGImages", n + ".jpg") for n in names])
        sw = IrnSweep(dev, args.betas, args.exp_times, args.thresholds)
        model = EdgeDisplacement()
        model.load_state_dict(torch.load(args.irn_weights_name, map_location="cpu"), strict=False)
        model = model.to(dev).eval()
        stager = MSFStager(dev)
        for n in names:
            img = PIL.Image.open(os.path.join(args.voc12_root, "JPEGImages", n + ".jpg")).convert("RGB")
            pair = torch.cat(stager(img, (1.0,)), dim=0)
            sw.add(model, pair, load_cam_dict(os.path.join(args.cam_dir, n + ".npy")), gt_of(n), name=n)
    for n in sw.all_zero_names():
        print(f"[muscle_amd] {n}: the walk result is all zero, counted as all background (infer_irn writes that PNG)", file=sys.stderr)
    m = sw.mious()
    for b, beta in enumerate(sw.betas):
        for e, et in enumerate(sw.exp_times):
            t = int(np.argmax(m[b, e]))
            head = "stored walk" if beta is None else f"beta {_fmt(beta)} exp_times {et}"
            print(f"{head}: best threshold {_fmt(sw.thresholds[t])}\tmIoU: {m[b, e, t]:.3f}%")
    b, e, t = best_of(m)
    if sw.betas[0] is None:
        print(f"best: --sem_seg_bg_thres {_fmt(sw.thresholds[t])}\tmIoU: {m[b, e, t]:.3f}%")
    else:
        print(f"best: {infer_irn_arguments(sw.betas[b], sw.exp_times[e], sw.thresholds[t])}\tmIoU: {m[b, e, t]:.3f}%")
    if args.out_table:
        np.save(args.out_table, sw.counts())
    if args.logfile:
        writelog(args.logfile, sw.loglist(b, e, t), "irn_sweep best: " + ("--sem_seg_bg_thres " + _fmt(sw.thresholds[t]) if sw.betas[0] is None
                                                                            else infer_irn_arguments(sw.betas[b], sw.exp_times[e], sw.thresholds[t])))
    return 0


if __name__ == "__main__":
    sys.exit(main())
