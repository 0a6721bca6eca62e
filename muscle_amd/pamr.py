"""Pixel-adaptive mask refinement (PAMR; Araslanov & Roth, "Single-Stage Semantic Segmentation from Image Labels", CVPR 2020) on the
HIP path (csrc/pamr.hip): a local affinity from the image, once per image, then a few fixed-point iterations of a convex
8 D-neighbour stencil on every channel of a mask.  No window that grows with a bandwidth, no lattice, no cap on the class count.

    neighbour p = 8 j + k of (y,x):  (clamp(y + d_j dy_k, 0, H-1), clamp(x + d_j dx_k, 0, W-1)),  (dy,dx)_k = the 8 offsets around 0
    std_c(y,x) = unbiased standard deviation of channel c over the 9 D taps (centre included) of all dilations, pooled
    a_p(y,x)   = (1/3) sum_c -|I_c(y,x) - I_c(nbr_p)| / (1e-8 + 0.1 std_c(y,x))
    w_p(y,x)   = softmax_p a_p(y,x)
    m_{s+1}[c,y,x] = sum_p w_p(y,x) m_s[c, nbr_p]            s = 0 .. num_iter-1, p in ascending order from 0

Stored values are fp32; the softmax normaliser and the stencil sum are accumulated in fp64 and rounded once, so that a constant
mask stays constant within 1e-6 over 10 iterations.  include/muscle_hip.h states the model in full; tests/pamr_ref.py restates it
in numpy.  The published module also resizes the mask
to the image size first; here both must already have the same H x W.  What is pinned is the model above against its fp64
restatement: parity with the published PAMR code unpinned, effect on mIoU unmeasured.
"""
from __future__ import annotations

import ctypes
from typing import Dict, Sequence, Tuple

import numpy as np
import torch

from ._lib import MuscleHipError, call, lib, ptr, stream
from .lattice import cached_workspace

DEFAULT_DILATIONS = (1, 2, 4, 8, 12, 24)
MAX_DILATIONS, MAX_DILATION = 8, 64

_ws: Dict[tuple, torch.Tensor] = {}


def check_dilations(dilations: Sequence[int]) -> Tuple[int, ...]:
    """The dilations as a tuple of ints: 1..8 of them, each in 1..64; anything else is a ValueError."""
    try:
        d = tuple(dilations)
    except TypeError:
        raise ValueError(f"dilations must be a sequence of integers (got {dilations!r})") from None
    if not 1 <= len(d) <= MAX_DILATIONS:
        raise ValueError(f"PAMR takes 1..{MAX_DILATIONS} dilations (got {len(d)})")
    for v in d:
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= int(v) <= MAX_DILATION:
            raise ValueError(f"every dilation must be an integer in 1..{MAX_DILATION} (got {v!r})")
    return tuple(int(v) for v in d)


def check_iters(num_iter) -> int:
    if isinstance(num_iter, bool) or not isinstance(num_iter, (int, np.integer)) or num_iter < 0:
        raise ValueError(f"num_iter must be an integer >= 0 (got {num_iter!r})")
    return int(num_iter)


def _dil(d: Tuple[int, ...]):
    return (ctypes.c_int * len(d))(*d)


def _check_size(N: int, C: int, P: int, H: int, W: int) -> None:
    if min(N, C, H, W) < 1:
        raise ValueError(f"empty input: N={N}, C={C}, H={H}, W={W}")
    if N * max(C, P) * H * W >= 2 ** 31:
        raise ValueError(f"N max(C,P) H W = {N * max(C, P) * H * W} must stay below 2^31")


def _image(img):
    """(img as a tensor, kind, batched, N, H, W): kind 0 = uint8 [H,W,3] / [N,H,W,3], kind 1 = fp32 [3,H,W] / [N,3,H,W].  Checks only:
    nothing is moved."""
    t = img if torch.is_tensor(img) else torch.from_numpy(np.array(img))          # a copy: PIL-backed arrays are read-only
    if t.dtype == torch.uint8:
        if t.dim() not in (3, 4) or t.shape[-1] != 3:
            raise ValueError(f"a uint8 img must be [H,W,3] or [N,H,W,3] (got {tuple(t.shape)})")
        return t, 0, t.dim() == 4, (int(t.shape[0]) if t.dim() == 4 else 1), int(t.shape[-3]), int(t.shape[-2])
    if t.dtype == torch.float32:
        if t.dim() not in (3, 4) or t.shape[-3] != 3:
            raise ValueError(f"an fp32 img must be [3,H,W] or [N,3,H,W] (got {tuple(t.shape)})")
        return t, 1, t.dim() == 4, (int(t.shape[0]) if t.dim() == 4 else 1), int(t.shape[-2]), int(t.shape[-1])
    raise ValueError(f"img must be uint8 [..,H,W,3] or fp32 [..,3,H,W] (got {t.dtype} {tuple(t.shape)})")


def _mask(mask):
    """(mask, batched, N, C, H, W) for an fp32 tensor [C,H,W] / [N,C,H,W].  Checks only."""
    if not torch.is_tensor(mask):
        raise ValueError(f"mask must be an fp32 tensor [C,H,W] or [N,C,H,W] (got {type(mask).__name__})")
    if mask.dtype != torch.float32 or mask.dim() not in (3, 4):
        raise ValueError(f"mask must be an fp32 tensor [C,H,W] or [N,C,H,W] (got {mask.dtype} {tuple(mask.shape)})")
    N = int(mask.shape[0]) if mask.dim() == 4 else 1
    return mask, mask.dim() == 4, N, int(mask.shape[-3]), int(mask.shape[-2]), int(mask.shape[-1])


def _on_device(t: torch.Tensor, what: str) -> torch.Tensor:
    if not t.is_cuda:
        raise MuscleHipError(f"PAMR runs on the GPU: {what} is a host tensor; there is no CPU path")
    return t.contiguous()


def _place_image(t: torch.Tensor, given, dev) -> torch.Tensor:
    """A numpy (or PIL-backed) uint8 image is uploaded, as crf_run does; a host TENSOR is an error."""
    if not torch.is_tensor(given) and t.dtype == torch.uint8:
        if dev is None:
            dev = torch.device("cuda", torch.cuda.current_device())
        return t.to(dev).contiguous()
    return _on_device(t, "img")


def pamr_affinity(img, dilations: Sequence[int] = DEFAULT_DILATIONS) -> torch.Tensor:
    """w fp32 [P,H,W] (img [H,W,3] / [3,H,W]) or [N,P,H,W] (a batched img), P = 8 len(dilations): the softmax weights of the model
    above, on the device.  img: uint8 [H,W,3] / [N,H,W,3] (numpy array or device tensor) or fp32 [3,H,W] / [N,3,H,W] (device tensor)."""
    d = check_dilations(dilations)
    t, kind, batched, N, H, W = _image(img)
    P = 8 * len(d)
    _check_size(N, 1, P, H, W)
    t = _place_image(t, img, None)
    with torch.cuda.device(t.device):
        w = torch.empty((N, P, H, W) if batched else (P, H, W), dtype=torch.float32, device=t.device)
        call("mx_pamr_affinity", ptr(t), kind, N, H, W, _dil(d), len(d), ptr(w), stream())
    return w


def pamr_apply(w: torch.Tensor, mask: torch.Tensor, num_iter: int = 10, dilations: Sequence[int] = DEFAULT_DILATIONS) -> torch.Tensor:
    """num_iter iterations of the stencil with the weights of pamr_affinity (same dilations) on mask fp32 [C,H,W] / [N,C,H,W]; returns
    a new tensor of the mask's shape on the device.  mask is not written; num_iter = 0 returns a copy."""
    d = check_dilations(dilations)
    it = check_iters(num_iter)
    m, batched, N, C, H, W = _mask(mask)
    P = 8 * len(d)
    if not torch.is_tensor(w) or w.dtype != torch.float32 or tuple(w.shape) != ((N, P, H, W) if w.dim() == 4 else (P, H, W)) \
            or (w.dim() == 3 and N != 1):
        raise ValueError(f"w must be fp32 [{N},{P},{H},{W}] for this mask and these dilations "
                         f"(got {getattr(w, 'dtype', type(w).__name__)} {tuple(getattr(w, 'shape', ()))})")
    _check_size(N, C, P, H, W)
    m = _on_device(m, "mask")
    w = _on_device(w, "w")
    if w.device != m.device:
        raise ValueError(f"w is on {w.device}, mask on {m.device}")
    if it == 0:
        return m.clone()
    with torch.cuda.device(m.device):
        bufs = [torch.empty_like(m), torch.empty_like(m) if it > 1 else None]
        src, dil = m, _dil(d)
        for s in range(it):
            dst = bufs[s & 1]
            call("mx_pamr_step", ptr(w), ptr(src), ptr(dst), N, C, H, W, dil, len(d), stream())
            src = dst
    return src


class PAMR:
    """pamr = PAMR(num_iter=10, dilations=(1,2,4,8,12,24)); refined = pamr(img, mask).  img: uint8 [H,W,3] / [N,H,W,3] (numpy array
    or device tensor) or fp32 [3,H,W] / [N,3,H,W] (device tensor); mask: fp32 [C,H,W] / [N,C,H,W] on the device with the image's
    H x W (and N).  One enqueue of mx_pamr on the current stream; the result is a new tensor of the mask's shape, bit-equal to
    pamr_apply(pamr_affinity(img, dilations), mask, num_iter, dilations)."""

    def __init__(self, num_iter: int = 10, dilations: Sequence[int] = DEFAULT_DILATIONS):
        self.num_iter = check_iters(num_iter)
        self.dilations = check_dilations(dilations)

    def __repr__(self) -> str:
        return f"PAMR(num_iter={self.num_iter}, dilations={self.dilations})"

    def affinity(self, img) -> torch.Tensor:
        return pamr_affinity(img, self.dilations)

    def apply(self, w: torch.Tensor, mask: torch.Tensor) -> torch.Tensor:
        return pamr_apply(w, mask, self.num_iter, self.dilations)

    def __call__(self, img, mask: torch.Tensor) -> torch.Tensor:
        d = self.dilations
        t, kind, ibatched, Ni, Hi, Wi = _image(img)
        m, batched, N, C, H, W = _mask(mask)
        if (Hi, Wi) != (H, W):
            raise ValueError(f"img is {(Hi, Wi)}, mask {(H, W)}: PAMR here does not resize, both must have the same H x W")
        if Ni != N or (ibatched != batched and N != 1):
            raise ValueError(f"img holds {Ni} image(s), mask {N}")
        _check_size(N, C, 8 * len(d), H, W)
        m = _on_device(m, "mask")
        t = _place_image(t, img, m.device)
        if t.device != m.device:
            raise ValueError(f"img is on {t.device}, mask on {m.device}")
        with torch.cuda.device(m.device):
            out = torch.empty_like(m)
            ws = cached_workspace(_ws, lib().mx_pamr_ws, m.device, (N, C, H, W, len(d)), 4) if self.num_iter else None
            call("mx_pamr", ptr(t), kind, ptr(m), ptr(out), N, C, H, W, _dil(d), len(d), self.num_iter, ptr(ws),
                 ws.numel() * 4 if ws is not None else 0, stream())
        return out


def planar_argmax(m: torch.Tensor) -> torch.Tensor:
    """uint8 [H,W] (or [N,H,W]) = argmax over the channels of m fp32 [C,H,W] (or [N,C,H,W]) on the device, first maximum wins."""
    m, batched, N, C, H, W = _mask(m)
    if C > 256:
        raise ValueError(f"a uint8 argmax holds at most 256 channels (got {C})")
    _check_size(N, C, 1, H, W)
    m = _on_device(m, "m")
    with torch.cuda.device(m.device):
        pred = torch.empty((N, H, W) if batched else (H, W), dtype=torch.uint8, device=m.device)
        call("mx_planar_argmax", ptr(m), N, C, H, W, ptr(pred), stream())
    return pred


def check_pamr_args(pamr, pamr_img, H: int, W: int):
    """The `pamr=` / `pamr_img=` pair of infer.infer_cam_fused and infer.infer_seg: None, or a PAMR with a uint8 image [H,W,3] of the
    output size.  Returns the image as a tensor (not moved), or None.  ValueError before anything touches a device."""
    if pamr is None:
        if pamr_img is not None:
            raise ValueError("pamr_img is given without pamr")
        return None
    if not isinstance(pamr, PAMR):
        raise ValueError(f"pamr must be a muscle_amd.PAMR (got {type(pamr).__name__})")
    if pamr_img is None:
        raise ValueError("pamr needs pamr_img, the original uint8 image [H,W,3]")
    t, kind, batched, _, Hi, Wi = _image(pamr_img)
    if kind != 0 or batched:
        raise ValueError(f"pamr_img must be one uint8 image [H,W,3] (got {t.dtype} {tuple(t.shape)})")
    if (Hi, Wi) != (int(H), int(W)):
        raise ValueError(f"pamr_img is {(Hi, Wi)}, the output {(int(H), int(W))}")
    return t
