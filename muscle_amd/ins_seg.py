"""Instance pseudo-labels from the IRN displacement field: IRN's published `make_ins_seg_labels` step on the HIP path.

`train_irn` trains the displacement heads and fills `mean_shift.running_mean`; `infer_irn` used to discard the field.  Here it
splits the class maps into instances before the random walk ("Instance pseudo-labels", is the specification):

  1. centroids   every pixel follows the displacement field `iterations` times (bilinear samples, pure fp32, no fused
                 multiply-add) and rounds to a pixel                                             mx_irn_centroids
  2. clusters    the 4-connected components of |dp| < thres are the instance seeds; a pixel belongs to the component its
                 centroid landed in (or to "background"); ids compressed to 0..I-1               mx_irn_weak, mx_ccl, mx_id_*
  3. scores      x[k*I + i] = cam[k] * (cluster == i), K*I channels                              mx_irn_ins_split
  4. walk        indexing.propagate_to_edge, unchanged
  5. finish      4x up-sample, / global maximum, arg-max over [bg_thres, channels] -> int32 label and the winning value;
                 no [C,H,W] array is written                                                     mx_irn_up_max, mx_irn_ins_finish
  6. segments    4-connected components of the label, ordered by (label, first pixel), with class, area and score
                                                                                                 mx_ccl, mx_id_*, mx_seg_stats, mx_seg_map

What is pinned is this algorithm against a numpy restatement (tests/ins_seg_ref.py); parity with IRN's own files and with
skimage.measure.label is unpinned (neither is available to the tests).

Three synchronising device-to-host reads per image, none larger than a few numbers per segment: the cluster count I (the
walk's channel count K*I has to be known to allocate), the segment count n with the bits of the global maximum, and the
[3,n] segment table (area, score bits, label; skipped when n = 0).  seg_map stays on the device until to_irn_dict() or a
caller copies it.
"""
from __future__ import annotations

import sys
from dataclasses import dataclass
from typing import Tuple

import numpy as np
import torch

from . import indexing, ops
from ._lib import MuscleHipError, call, lib, ptr, stream


def _need_cuda(what: str, *ts):
    if not all(t.is_cuda for t in ts):
        raise MuscleHipError(f"{what} runs on the HIP kernels only")


def _check_dp(what: str, dp):
    if not torch.is_tensor(dp) or dp.dtype != torch.float32 or dp.dim() != 3 or dp.shape[0] != 2 or dp.shape[1] < 1 or dp.shape[2] < 1:
        got = f"{dp.dtype} {tuple(dp.shape)}" if torch.is_tensor(dp) else type(dp).__name__
        raise ValueError(f"{what}: dp must be a float32 [2,h,w] tensor (got {got})")


def _check_count(what: str, name: str, v, lo: int):
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or int(v) != v or v < lo:
        raise ValueError(f"{what}: {name} must be an integer >= {lo} (got {v!r})")


def _check_number(what: str, name: str, v, positive: bool):
    ok = not isinstance(v, bool) and isinstance(v, (int, float, np.integer, np.floating)) and np.isfinite(v)
    if not ok or (v <= 0 if positive else v < 0):
        raise ValueError(f"{what}: {name} must be a {'positive number' if positive else 'number >= 0'} (got {v!r})")


def find_centroids(dp: torch.Tensor, iterations: int = 300) -> torch.Tensor:
    """Step 1.  dp: float32 [2,h,w] (dy, dx; finite) on the device.  Returns int32 [2,h,w]: the (y, x) every pixel ends at."""
    _check_dp("find_centroids", dp)
    _check_count("find_centroids", "iterations", iterations, 0)
    _need_cuda("find_centroids", dp)
    dp = dp.contiguous()
    cent = torch.empty(dp.shape, dtype=torch.int32, device=dp.device)
    call("mx_irn_centroids", ptr(dp), dp.shape[1], dp.shape[2], int(iterations), ptr(cent), stream())
    return cent


def connected_components(label: torch.Tensor) -> torch.Tensor:
    """Steps 2 and 6.  label: int32 [h,w] on the device.  Pixels with the same non-zero label that share an edge form a
    component; returns int32 [h,w]: the smallest linear index y*w + x of the pixel's component, -1 where label is 0."""
    if not torch.is_tensor(label) or label.dtype != torch.int32 or label.dim() != 2 or label.numel() == 0:
        got = f"{label.dtype} {tuple(label.shape)}" if torch.is_tensor(label) else type(label).__name__
        raise ValueError(f"connected_components: label must be a non-empty int32 [h,w] tensor (got {got})")
    _need_cuda("connected_components", label)
    label = label.contiguous()
    h, w = label.shape
    nbytes = lib().mx_ccl_ws(h, w)
    if nbytes < 0:
        raise ValueError(f"connected_components: a {h}x{w} map is too large")
    ws = torch.empty(nbytes // 4, dtype=torch.int32, device=label.device)
    root = torch.empty_like(label)
    call("mx_ccl", ptr(label), h, w, ptr(root), ptr(ws), stream())
    return root


def _compress(root: torch.Tensor, cent, meta: torch.Tensor):
    """marks and rank (int32 [n+1]) of the ids root[...] that occur; meta[0] = their number, meta[1] = 1 if -1 occurs."""
    h, w = root.shape
    marks = torch.empty(h * w + 1, dtype=torch.int32, device=root.device)
    rank = torch.empty_like(marks)
    call("mx_id_mark", ptr(root), ptr(cent), h, w, ptr(marks), stream())
    call("mx_id_rank", ptr(marks), h * w + 1, ptr(rank), ptr(meta), stream())
    return marks, rank


def cluster_centroids(centroids: torch.Tensor, dp: torch.Tensor, thres: float = 2.5) -> Tuple[torch.Tensor, int]:
    """Step 2.  centroids: int32 [2,h,w] of find_centroids (a centroid outside the image counts as background), dp: the field.
    Returns (cluster int32 [h,w] in 0..I-1, I): the weak-displacement component at every pixel's centroid, ids compressed in
    ascending order of the component's first pixel, background (a centroid on a non-weak pixel) first where it occurs.
    Reads I back (one synchronising read of one integer)."""
    _check_dp("cluster_centroids", dp)
    if not torch.is_tensor(centroids) or centroids.dtype != torch.int32 or centroids.shape != dp.shape:
        got = f"{centroids.dtype} {tuple(centroids.shape)}" if torch.is_tensor(centroids) else type(centroids).__name__
        raise ValueError(f"cluster_centroids: centroids must be int32 {tuple(dp.shape)} like dp (got {got})")
    _check_number("cluster_centroids", "thres", thres, True)
    _need_cuda("cluster_centroids", centroids, dp)
    dp, centroids = dp.contiguous(), centroids.contiguous()
    _, h, w = dp.shape
    weak = torch.empty(h, w, dtype=torch.int32, device=dp.device)
    call("mx_irn_weak", ptr(dp), h, w, float(thres), ptr(weak), stream())
    root = connected_components(weak)
    meta = torch.empty(2, dtype=torch.int32, device=dp.device)
    _, rank = _compress(root, centroids, meta)
    cluster = torch.empty(h, w, dtype=torch.int32, device=dp.device)
    call("mx_id_apply", ptr(root), ptr(centroids), h, w, ptr(rank), ptr(cluster), stream())
    return cluster, int(meta[:1].cpu().numpy()[0])


def split_instances(cams: torch.Tensor, cluster: torch.Tensor, I: int) -> torch.Tensor:
    """Step 3.  cams float32 [K,h,w], cluster int32 [h,w] in 0..I-1 -> x float32 [K*I,h,w], class-major."""
    K, h, w = cams.shape
    x = torch.empty(K * I, h, w, dtype=torch.float32, device=cams.device)
    call("mx_irn_ins_split", ptr(cams.contiguous()), ptr(cluster.contiguous()), K, I, h * w, ptr(x), stream())
    return x


def finish_instances(rw: torch.Tensor, H: int, W: int, bg_thres: float, max_scratch: torch.Tensor = None):
    """Step 5.  rw [C,1,h,w] (or [C,h,w]) of the walk -> (label int32 [H,W], win float32 [H,W], max_scratch int32 [1]: the bits of
    the global maximum).  The arithmetic is mx_irn_finish's (csrc/irn_soft.h); any C."""
    C, h, w = rw.shape[0], rw.shape[-2], rw.shape[-1]
    r = rw.reshape(C, h, w).contiguous().float()
    if max_scratch is None:
        max_scratch = torch.empty(1, dtype=torch.int32, device=rw.device)
    label = torch.empty(H, W, dtype=torch.int32, device=rw.device)
    win = torch.empty(H, W, dtype=torch.float32, device=rw.device)
    call("mx_irn_up_max", ptr(r), C, h, w, H, W, ptr(max_scratch), stream())
    call("mx_irn_ins_finish", ptr(r), C, h, w, H, W, float(bg_thres), ptr(max_scratch), ptr(label), ptr(win), stream())
    return label, win, max_scratch


@dataclass
class InstanceLabels:
    """The instance pseudo-label of one image.  seg_map: int32 [H,W] on the device, 0 = no segment, s = segment s-1;
    score float32 [n], cls int64 [n] (0-based class index, as in the CAM dict), area int32 [n]: host arrays, segments ordered
    by (label, first raster pixel).  vmax: the global maximum the walk result was divided by (0: nothing to label)."""
    seg_map: torch.Tensor
    score: np.ndarray
    cls: np.ndarray
    area: np.ndarray
    vmax: float = 1.0

    def __len__(self):
        return int(self.score.shape[0])

    def to_irn_dict(self):
        """{'score' float32 [n], 'mask' bool [n,H,W], 'class' int64 [n]}: what IRN's make_ins_seg_labels np.save's.  n = 0 gives
        shapes (0,), (0,H,W), (0,), where IRN's np.stack of an empty list would raise."""
        sm = self.seg_map.cpu().numpy()
        n = len(self)
        mask = sm[None] == np.arange(1, n + 1, dtype=np.int32)[:, None, None] if n else np.zeros((0,) + sm.shape, bool)
        return {"score": self.score.copy(), "mask": mask, "class": self.cls.copy()}


def label_segments(label: torch.Tensor, win: torch.Tensor, keys, I: int, max_scratch: torch.Tensor = None) -> InstanceLabels:
    """Step 6.  label int32 [H,W] (0 = background, c = channel c-1 of the K*I class-major channels), win float32 [H,W] >= 0,
    keys: the K class indices in ascending order.  Two synchronising reads: the segment count (with the bits of max_scratch) and,
    for n > 0, the [3,n] int32 table (area, score bits, label) in the final order."""
    H, W = label.shape
    n_pix = H * W
    dev = label.device
    root = connected_components(label)
    meta = torch.zeros(3, dtype=torch.int32, device=dev)
    marks, rank = _compress(root, None, meta)
    if max_scratch is not None:
        meta[2:] = max_scratch
    m = meta.cpu().numpy()
    n = int(m[0]) - int(m[1])
    vmax = float(m[2:].view(np.float32)[0]) if max_scratch is not None else 1.0
    if n == 0:
        return InstanceLabels(torch.zeros(H, W, dtype=torch.int32, device=dev), np.zeros(0, np.float32), np.zeros(0, np.int64),
                              np.zeros(0, np.int32), vmax)
    area = torch.empty(n, dtype=torch.int32, device=dev)
    bits = torch.empty(n, dtype=torch.int32, device=dev)
    seg_label = torch.empty(n, dtype=torch.int32, device=dev)
    seg_first = torch.empty(n, dtype=torch.int32, device=dev)
    call("mx_seg_stats", ptr(label.contiguous()), ptr(root), ptr(win.contiguous()), ptr(rank), ptr(marks), n_pix, n, ptr(area), ptr(bits),
         ptr(seg_label), ptr(seg_first), stream())
    # n numbers per array from here on: the order (label, first pixel) and the per-segment table
    idx = torch.argsort(seg_label.long() * n_pix + seg_first.long())
    order = torch.empty(n, dtype=torch.int32, device=dev)
    order[idx] = torch.arange(n, dtype=torch.int32, device=dev)
    seg_map = torch.empty(H, W, dtype=torch.int32, device=dev)
    call("mx_seg_map", ptr(root), ptr(rank), ptr(marks), ptr(order), n_pix, n, ptr(seg_map), stream())
    table = torch.stack([area, bits, seg_label])[:, idx].cpu().numpy()           # the one read of the per-segment numbers
    area = table[0].copy()
    score = table[1].view(np.float32).copy()
    score[area.astype(np.float64) < n_pix * 0.01] = 0.0
    keys = np.asarray(list(keys), np.int64)
    cls = keys[(table[2].astype(np.int64) - 1) // int(I)]
    return InstanceLabels(seg_map, score, cls, area, vmax)


def instances_from_field(edge: torch.Tensor, dp: torch.Tensor, cam_dict, H: int, W: int, *, beta=8, exp_times=6, bg_thres=0.25,
                         iterations=300, dp_thres=2.5, method: str = "dense", down: torch.Tensor = None) -> InstanceLabels:
    """Steps 1-6 from the network's outputs: edge [1,h,w], dp [2,h,w] (eval mode: mean-shifted), the CAM dict of infer_mcl.
    down: the CAMs of the dict's classes (ascending) already down-scaled to [K,h,w] on the device, where the caller has them
    (infer_irn does); without it they are uploaded and down-scaled here."""
    what = "infer_irn_instances"
    if method not in indexing.WALK_METHODS:
        raise ValueError(f"{what}: method must be one of {indexing.WALK_METHODS} (got {method!r})")
    keys = sorted(int(k) for k in cam_dict)
    if not keys:
        raise ValueError(f"{what}: the CAM dict holds no class (K >= 1 is needed)")
    _check_number(what, "bg_thres", bg_thres, False)
    _check_count(what, "iterations", iterations, 0)
    _check_number(what, "dp_thres", dp_thres, True)
    for k in keys:
        if tuple(np.shape(cam_dict[k])) != (H, W):
            raise ValueError(f"{what}: the CAM of class {k} is {np.shape(cam_dict[k])}, the image is {(H, W)}")
    _check_dp(what, dp)
    h, w = dp.shape[1:]
    if down is not None and tuple(down.shape) != (len(keys), h, w):
        raise ValueError(f"{what}: down must be [{len(keys)},{h},{w}] (got {tuple(down.shape)})")
    with torch.no_grad():
        if down is None:
            cams = torch.from_numpy(np.stack([np.asarray(cam_dict[k], np.float32) for k in keys])).to(dp.device)
            down = ops.resize_planar_halfpixel(cams, h, w)
        cent = find_centroids(dp, iterations)
        cluster, I = cluster_centroids(cent, dp, dp_thres)
        x = split_instances(down, cluster, I)
        rw = indexing.propagate_to_edge(x, edge, beta=beta, exp_times=exp_times, radius=5, method=method)
        label, win, scratch = finish_instances(rw, H, W, bg_thres)
        return label_segments(label, win, keys, I, scratch)


def infer_irn_instances(model, img_pair: torch.Tensor, cam_dict, *, beta=8, exp_times=6, bg_thres=0.25, iterations=300,
                        dp_thres=2.5, method: str = "dense") -> InstanceLabels:
    """The instance path of infer_irn for one image: model = EdgeDisplacement in eval mode (so dp is mean-shifted), img_pair
    [2,3,H,W] on the device, cam_dict {class index: float32 [H,W]}.  See the module text for the steps."""
    if getattr(model, "training", False):
        raise ValueError("infer_irn_instances: call model.eval() first (the mean shift is the identity in training mode)")
    H, W = img_pair.shape[2:]
    edge, dp = model(img_pair)
    return instances_from_field(edge[0] if edge.dim() == 4 else edge, dp[0] if dp.dim() == 4 else dp, cam_dict, H, W, beta=beta,
                                exp_times=exp_times, bg_thres=bg_thres, iterations=iterations, dp_thres=dp_thres, method=method)


def save_instances(path: str, ins: InstanceLabels) -> None:
    """np.save of to_irn_dict(): IRN's file format."""
    np.save(path, ins.to_irn_dict())


def warn_all_zero(name: str) -> None:
    print(f"[muscle_amd] {name}: the walk result is all zero, the instance label is empty", file=sys.stderr)
