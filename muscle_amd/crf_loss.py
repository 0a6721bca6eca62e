"""Dense-CRF energy loss for decoder training: a training signal for the pixels a label map ignores (255) and an edge-aware term
for the soft path.  It is OURS, not the reference's: the regularised loss of Tang et al. 2018 ("On Regularized Losses for
Weakly-supervised CNN Segmentation") - the Potts energy of a dense bilateral CRF, evaluated on the network's own softmax - with
the pairwise sums evaluated exactly over a square window on the stencil-GEMM of the dense CRFs (csrc/crf_msg.h) instead of on a
permutohedral lattice, and normalised by the affinity mass.  include/muscle_hip.h states the model (mx_crf_loss_fwd):

    loss = 1 - sum_{u,v} k(u,v) sum_c S_c(u) S_c(v) / sum_{u,v} k(u,v) r_u r_v

with S the softmax pooled over f x f cells inside each item's window, r the share of a cell inside it, and k the bilateral
kernel between cells (width sxy / f cells, colour width srgb, cut at ceil(trunc * sxy / f) cells).  It is the share of the affinity
mass that joins differently predicted pixels, a number in [0, 1]; uniform predictions give 1 - 1/K, a constant confident map 0.
Parity with rloss's lattice implementation is not pinned (another approximation of the same sums); what is pinned is this
model against its numpy restatement (tests/crf_loss_ref.py).  Whether the term raises mIoU is unmeasured.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import torch
from torch import nn

from ._lib import MuscleHipError, call, lib, ptr, stream
from .lattice import cached_workspace

MAX_CLASSES = 24            # CRF_MAXL of csrc/crf_msg.h: the share r travels in column K of the 32
SCALES = (1, 2, 4, 8)
_COLS = 32

_ws: Dict[tuple, torch.Tensor] = {}


def _check(seg, img, window, scale: int, sxy: float, srgb: float):
    if seg.dim() != 4:
        raise ValueError(f"seg_map must be [N,K,H,W] (got {tuple(seg.shape)})")
    N, K, H, W = seg.shape
    if tuple(img.shape) != (N, 3, H, W):
        raise ValueError(f"img must be [N,3,H,W] = {(N, 3, H, W)} (got {tuple(img.shape)})")
    if not 2 <= K <= MAX_CLASSES:
        raise ValueError(f"K={K} outside 2..{MAX_CLASSES}")
    if scale not in SCALES:
        raise ValueError(f"scale={scale} is not one of {SCALES}")
    if H % scale or W % scale:
        raise ValueError(f"H={H} and W={W} must be multiples of scale={scale}")
    if not (sxy > 0 and srgb > 0):
        raise ValueError(f"sxy={sxy} and srgb={srgb} must be positive")
    if window is not None and (tuple(window.shape) != (N, 4) or window.dtype != torch.int32):
        raise ValueError(f"window must be int32 [N,4] = {(N, 4)} (got {window.dtype} {tuple(window.shape)})")
    for name, t in (("seg_map", seg), ("img", img), ("window", window)):
        if t is not None and not t.is_cuda:
            raise MuscleHipError(f"muscle_amd kernels need CUDA (ROCm) tensors; there is no CPU path ({name} is on {t.device})")


def energy_forward(seg: torch.Tensor, img: torch.Tensor, window: Optional[torch.Tensor] = None, *, sxy: float = 80.0,
                   srgb: float = 15.0, scale: int = 4, trunc: float = 2.0) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """One enqueue of mx_crf_loss_fwd on the current stream.  seg fp32 [N,K,H,W] contiguous, img fp32 [N,3,H,W], window int32 [N,4]
    or None.  Returns (loss fp32 [1], sums fp64 [2] = (D, sum S . M), M fp32 [N,H/scale,W/scale,32] = [M | Z | 0]) on the device."""
    _check(seg, img, window, scale, sxy, srgb)
    N, K, H, W = seg.shape
    dev = seg.device
    img = img.contiguous().float()
    window = None if window is None else window.contiguous()
    with torch.cuda.device(dev):
        ws = cached_workspace(_ws, lib().mx_crf_loss_ws, dev, (N, K, H, W, scale), 4)
        M = torch.empty(N, H // scale, W // scale, _COLS, dtype=torch.float32, device=dev)
        sums = torch.empty(2, dtype=torch.float64, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        call("mx_crf_loss_fwd", ptr(seg), ptr(img), ptr(window), N, K, H, W, scale, float(sxy), float(srgb), float(trunc), ptr(ws),
             ptr(M), ptr(sums), ptr(loss), stream())
    return loss, sums, M


def energy_backward(seg: torch.Tensor, window: Optional[torch.Tensor], M: torch.Tensor, sums: torch.Tensor, g: torch.Tensor,
                    scale: int) -> torch.Tensor:
    """One enqueue of mx_crf_loss_bwd: d loss / d seg [N,K,H,W] times the upstream scalar g (a device tensor)."""
    N, K, H, W = seg.shape
    out = torch.empty_like(seg)
    with torch.cuda.device(seg.device):
        call("mx_crf_loss_bwd", ptr(seg), ptr(window), ptr(M), ptr(sums), ptr(g.contiguous().float().reshape(1)), N, K, H, W, scale,
             ptr(out), stream())
    return out


class _DenseEnergyFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, img, window, cfg):
        seg = seg.contiguous().float()
        loss, sums, M = energy_forward(seg, img, window, **cfg)
        window = None if window is None else window.contiguous()
        ctx.save_for_backward(seg, M, sums)
        ctx.window, ctx.scale = window, cfg["scale"]
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        seg, M, sums = ctx.saved_tensors
        return energy_backward(seg, ctx.window, M, sums, g, ctx.scale), None, None, None


class DenseEnergyLoss(nn.Module):
    """loss = DenseEnergyLoss(sxy, srgb, scale, trunc)(seg_map, img, window): a 0-dim device tensor in [0, 1], differentiable in
    seg_map (which may be non-contiguous).  sxy is in full-resolution pixels; scale is the pooling factor f.  window: int32 [N,4]
    = (y0, x0, y1, x1), half-open - the part of each crop container that holds image, as `segdata.plan_window` gives it; None:
    the whole map.  Pixels outside it neither count nor get a gradient.  Every window empty: loss 0, gradient 0."""

    def __init__(self, sxy: float = 80.0, srgb: float = 15.0, scale: int = 4, trunc: float = 2.0):
        super().__init__()
        if scale not in SCALES:
            raise ValueError(f"scale={scale} is not one of {SCALES}")
        if not (sxy > 0 and srgb > 0):
            raise ValueError(f"sxy={sxy} and srgb={srgb} must be positive")
        self.sxy, self.srgb, self.scale, self.trunc = float(sxy), float(srgb), int(scale), float(trunc)

    def forward(self, seg_map, img, window=None):
        cfg = dict(sxy=self.sxy, srgb=self.srgb, scale=self.scale, trunc=self.trunc)
        return _DenseEnergyFn.apply(seg_map, img, window, cfg)
