"""Lovasz-softmax loss for decoder training on label maps: a surrogate of the mean IoU that `validate_seg` reports.  It is OURS,
not the reference's: the loss of Berman, Triki & Blaschko, "The Lovasz-Softmax loss: a tractable surrogate for the optimization
of the intersection-over-union measure in neural networks" (CVPR 2018).  include/muscle_hip.h states the model (mx_lovasz_ws ..):
per (group, class) segment the errors e = |fg - softmax(seg)_c| of the valid pixels are sorted descending (ties by pixel order)
and weighted with the increments of the Jaccard index along that order,

    L = sum_j e_j g_{rank_j},      loss = mean over groups of the mean of L over the counted classes

on a stable, segmented, deterministic radix sort (csrc/lovasz.hip); nothing is read back to the host.  What is pinned is this
model against its numpy restatement (tests/lovasz_ref.py), which in turn matches torch autograd of Berman's published function.
Whether the term raises mIoU is unmeasured.
"""
from __future__ import annotations

from typing import Dict, Tuple

import numpy as np
import torch
from torch import nn

from ._lib import MuscleHipError, call, lib, ptr, stream

MAX_CLASSES = 24
IGNORE_LABEL = 255
CLASSES = ("present", "all")
KEY_ONE = 0x3F800000            # bits(1.0f): key = KEY_ONE - bits(e)
KEY_INVALID = 0x40000000        # the key of an ignored element: above every valid key

_ws: Dict[tuple, torch.Tensor] = {}


def key_of(e) -> np.ndarray:
    """The sort key of csrc/lovasz.hip (lv_key_of) for float32 errors, as uint32: ascending key = descending e; a value outside
    [0,1] (NaN) takes key 0 and sorts as e = 1.  A pure function of fp32 bits: the device and numpy agree exactly."""
    e = np.ascontiguousarray(e, dtype=np.float32)
    bits = e.view(np.uint32) & np.uint32(0x7FFFFFFF)
    with np.errstate(invalid="ignore"):
        ok = (e >= 0) & (e <= 1)
    return np.where(ok, np.uint32(KEY_ONE) - np.where(ok, bits, np.uint32(0)), np.uint32(0)).astype(np.uint32)


def _check(seg, label, classes: str = "present"):
    if classes not in CLASSES:
        raise ValueError(f"classes={classes!r} is not one of {CLASSES}")
    if seg.dim() != 4:
        raise ValueError(f"seg_map must be [N,K,H,W] (got {tuple(seg.shape)})")
    N, K, H, W = seg.shape
    if not 1 <= K <= MAX_CLASSES:
        raise ValueError(f"K={K} outside 1..{MAX_CLASSES}")
    if N < 1 or H * W < 1:
        raise ValueError(f"seg_map {tuple(seg.shape)} is empty")
    if not seg.is_floating_point():
        raise ValueError(f"seg_map must be floating point (got {seg.dtype})")
    if label.dtype != torch.uint8 or tuple(label.shape) != (N, H, W):
        raise ValueError(f"a label map must be [N,H,W] = {(N, H, W)} uint8 (got {label.dtype} {tuple(label.shape)})")
    for name, t in (("seg_map", seg), ("label", label)):
        if not t.is_cuda:
            raise MuscleHipError(f"muscle_amd kernels need CUDA (ROCm) tensors; there is no CPU path ({name} is on {t.device})")


def _shape(N: int, K: int, HW: int, per_image: bool) -> Tuple[int, int]:
    S, P = (N * K, HW) if per_image else (K, N * HW)
    if P >= 2 ** 31 or S * P >= 2 ** 32:
        raise ValueError(f"S*P = {S} * {P}: the sort takes P < 2^31 and S*P < 2^32")
    return S, P


def workspace(S: int, P: int, dev) -> torch.Tensor:
    """The sort's scratch for S segments of P elements (mx_lovasz_ws bytes), cached per (device, S, P, stream)."""
    key = (dev.index, S, P, stream())
    buf = _ws.get(key)
    if buf is None:
        n = lib().mx_lovasz_ws(S, P)
        if n < 0:
            raise MuscleHipError(f"mx_lovasz_ws({S}, {P}) failed: {lib().mx_last_error().decode()}")
        for k in [k for k in _ws if k[0] == dev.index and k[3] == key[3]]:      # one shape per stream is kept
            del _ws[k]
        buf = _ws[key] = torch.empty((n + 7) // 8, dtype=torch.int64, device=dev)
    return buf


def lovasz_errors(seg_map: torch.Tensor, label: torch.Tensor, per_image: bool = False) -> Tuple[torch.Tensor, torch.Tensor]:
    """Stage 1 (mx_lovasz_errors): err fp32 [S,P] and flag uint8 [S,P] (bit 0 foreground, bit 1 valid) of seg_map [N,K,H,W] and
    label uint8 [N,H,W]; S = K segments of N*H*W elements, or with per_image N*K segments of H*W."""
    _check(seg_map, label)
    N, K, H, W = seg_map.shape
    S, P = _shape(N, K, H * W, per_image)
    seg, label = seg_map.contiguous().float(), label.contiguous()
    with torch.cuda.device(seg.device):
        err = torch.empty(S, P, dtype=torch.float32, device=seg.device)
        flag = torch.empty(S, P, dtype=torch.uint8, device=seg.device)
        call("mx_lovasz_errors", ptr(seg), ptr(label), IGNORE_LABEL, N, K, H * W, int(bool(per_image)), ptr(err), ptr(flag), stream())
    return err, flag


def lovasz_core(err: torch.Tensor, flag: torch.Tensor) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """Stages 2 and 3 (mx_lovasz_core) on given errors: err fp32 [S,P], flag uint8 [S,P].  Returns (rank int32 [S,P]: the position
    in the stable descending order, -1 at an ignored element; g fp32 [S,P]: the Jaccard increment at each element, original order;
    seg_loss fp64 [S]; counts int32 [S,2] = (G, V))."""
    if err.dim() != 2 or err.dtype != torch.float32 or flag.dtype != torch.uint8 or flag.shape != err.shape or err.numel() == 0:
        raise ValueError(f"err fp32 [S,P] and flag uint8 [S,P] (got {err.dtype} {tuple(err.shape)}, {flag.dtype} {tuple(flag.shape)})")
    for name, t in (("err", err), ("flag", flag)):
        if not t.is_cuda:
            raise MuscleHipError(f"muscle_amd kernels need CUDA (ROCm) tensors; there is no CPU path ({name} is on {t.device})")
    S, P = err.shape
    _shape(1, S, P, False)
    err, flag, dev = err.contiguous(), flag.contiguous(), err.device
    with torch.cuda.device(dev):
        ws = workspace(S, P, dev)
        rank = torch.empty(S, P, dtype=torch.int32, device=dev)
        g = torch.empty(S, P, dtype=torch.float32, device=dev)
        seg_loss = torch.empty(S, dtype=torch.float64, device=dev)
        counts = torch.empty(S, 2, dtype=torch.int32, device=dev)
        call("mx_lovasz_core", ptr(err), ptr(flag), S, P, ptr(rank), ptr(g), ptr(seg_loss), ptr(counts), ws.data_ptr(), ws.numel() * 8,
             stream())
    return rank, g, seg_loss, counts


class _LovaszFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, label, classes, per_image):
        _check(seg, label, classes)
        seg, label = seg.contiguous().float(), label.contiguous()
        N, K, H, W = seg.shape
        S, P = _shape(N, K, H * W, per_image)
        dev = seg.device
        with torch.cuda.device(dev):
            ws = workspace(S, P, dev)
            err = torch.empty(S, P, dtype=torch.float32, device=dev)
            flag = torch.empty(S, P, dtype=torch.uint8, device=dev)
            g = torch.empty(S, P, dtype=torch.float32, device=dev)
            seg_loss = torch.empty(S, dtype=torch.float64, device=dev)
            counts = torch.empty(S, 2, dtype=torch.int32, device=dev)
            segw = torch.empty(S, dtype=torch.float32, device=dev)
            loss = torch.empty(1, dtype=torch.float32, device=dev)
            call("mx_lovasz_fwd", ptr(seg), ptr(label), IGNORE_LABEL, N, K, H * W, int(per_image), int(classes == "all"), ptr(err),
                 ptr(flag), ptr(g), ptr(seg_loss), ptr(counts), ptr(segw), ptr(loss), ws.data_ptr(), ws.numel() * 8, stream())
        ctx.save_for_backward(seg, label, g, segw)
        ctx.per_image = int(per_image)
        return loss[0]

    @staticmethod
    def backward(ctx, gup):
        seg, label, g, segw = ctx.saved_tensors
        N, K, H, W = seg.shape
        out = torch.empty_like(seg)
        with torch.cuda.device(seg.device):
            call("mx_lovasz_bwd", ptr(seg), ptr(label), IGNORE_LABEL, ptr(g), ptr(segw), ptr(gup.contiguous().float().reshape(1)), N, K,
                 H * W, ctx.per_image, ptr(out), stream())
        return out, None, None, None


def lovasz_softmax(seg_map: torch.Tensor, label: torch.Tensor, classes: str = "present", per_image: bool = False) -> torch.Tensor:
    """The Lovasz-softmax loss of logits seg_map [N,K,H,W] (may be non-contiguous) against a label map uint8 [N,H,W] (255, and any
    value >= K, is ignored): a 0-dim device tensor, differentiable in seg_map.  classes: "present" averages over the classes that
    occur among the valid pixels of a group, "all" over every class; per_image: one group per image instead of one for the batch.
    Nothing valid: loss 0, gradient 0."""
    return _LovaszFn.apply(seg_map, label, classes, bool(per_image))


class LovaszSoftmaxLoss(nn.Module):
    """loss = LovaszSoftmaxLoss(classes="present" | "all", per_image=False)(seg_map, label): `lovasz_softmax` as a module."""

    def __init__(self, classes: str = "present", per_image: bool = False):
        super().__init__()
        if classes not in CLASSES:
            raise ValueError(f"classes={classes!r} is not one of {CLASSES}")
        self.classes, self.per_image = classes, bool(per_image)

    def forward(self, seg_map, label):
        return lovasz_softmax(seg_map, label, self.classes, self.per_image)
