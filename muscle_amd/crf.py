"""Dense CRF refinement of a probability map (src/imutils.py:439-456, `crf_inference`) on the HIP path.

The reference hands the model below to pydensecrf (Kraehenbuehl & Koltun 2011, pydensecrf defaults: diagonal kernels,
symmetric normalisation, Potts compatibility):

    U[l,i]   = -log(clip(confidence * probs[l,i] + (1 - confidence) / L, 1e-5, 1))
    k_m(i,j) = exp(-0.5 * |f_m(i) - f_m(j)|^2)                  m in {gauss, bilateral}; j == i included
               f_gauss = (x, y) / (3 / scale_factor),  weight 1
               f_bilateral = (x / s, y / s, r / 10, g / 10, b / 10) with s = 32 / scale_factor,  weight 10
    n_m(i)   = 1 / sqrt(sum_j k_m(i,j) + 1e-20)
    Q_0      = softmax_l(-U)
    Q_{s+1}  = softmax_l(-U + sum_m w_m n_m(i) sum_j k_m(i,j) n_m(j) Q_s[l,j])         s = 0 .. t-1

pydensecrf evaluates the sums over j approximately, on a permutohedral lattice.  Here they are evaluated exactly over a
square window: j contributes to i iff |x_i - x_j| <= R_m and |y_i - y_j| <= R_m with R_m = ceil(trunc * sxy_m); trunc <= 0,
or a window that covers the image, means all pairs.  The window is part of the model (it enters n_m too).  Label maps are
therefore not bit-identical with pydensecrf's; what is pinned is this model against an fp64 restatement
(tests/crf_ref.py).  With the default trunc = 4 the windowed result differs from the all-pairs one by less than 1e-4.

pairwise="lattice" selects pydensecrf's own approximation instead (muscle_amd.lattice, csrc/lattice.hip): both kernels on
permutohedral lattices, n_m = 1 / sqrt(filter_m(1) + 1e-20), message w_m n_m filter_m(n_m Q); trunc is ignored.  It is a
different model (label maps differ from the windowed ones in a few per cent of the pixels), pinned against its own numpy
restatement (tests/lattice_ref.py); parity with pydensecrf itself is not pinned.  "window" stays the default everywhere.
"""
from __future__ import annotations

from typing import Dict, Optional, Tuple

import numpy as np
import torch

from ._lib import call, lib, ptr, stream
from .lattice import cached_workspace, check_pairwise, crf_lattice_workspace, device_image

# imutils.py:452-453: addPairwiseGaussian(sxy=3/scale_factor, compat=1), addPairwiseBilateral(sxy=32/scale_factor, srgb=10, compat=10)
GAUSS_SXY, GAUSS_W = 3.0, 1.0
BILATERAL_SXY, BILATERAL_SRGB, BILATERAL_W = 32.0, 10.0, 10.0

_ws: Dict[tuple, torch.Tensor] = {}


def _workspace(dev: torch.device, H: int, W: int) -> torch.Tensor:
    return cached_workspace(_ws, lib().mx_crf_workspace_bytes, dev, (1, H, W), 4)


def crf_run(img, probs, t: int, scale_factor: float, labels: int, confidence: float, trunc: float, want_q: bool = True,
            want_pred: bool = False, *, pairwise: str = "window") -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One enqueue of mx_crf_inference (pairwise="lattice": mx_crf_inference_lattice) on the current stream; returns
    (Q fp32 [L,H,W] or None, argmax uint8 [H,W] or None)."""
    lattice = check_pairwise(pairwise)
    if torch.is_tensor(probs):
        p = probs
        dev = p.device if p.is_cuda else torch.device("cuda", torch.cuda.current_device())
    else:
        p = torch.as_tensor(np.ascontiguousarray(probs, dtype=np.float32))
        dev = torch.device("cuda", torch.cuda.current_device())
    if p.dim() != 3 or p.shape[0] != labels:
        raise ValueError(f"probs must be [labels={labels},H,W] (got {tuple(p.shape)})")
    p = p.to(dev, torch.float32).contiguous()
    L, H, W = p.shape
    im = device_image(img, dev)
    if tuple(im.shape[:2]) != (H, W):
        raise ValueError(f"img is {tuple(im.shape[:2])}, probs {(H, W)}")
    if not scale_factor > 0:
        raise ValueError("scale_factor must be positive")
    with torch.cuda.device(dev):
        q = torch.empty(L, H, W, dtype=torch.float32, device=dev) if want_q else None
        pred = torch.empty(H, W, dtype=torch.uint8, device=dev) if want_pred else None
        if lattice:
            ws = crf_lattice_workspace(dev, L, H, W)
            call("mx_crf_inference_lattice", ptr(im), ptr(p), L, H, W, int(t), float(confidence), GAUSS_SXY / scale_factor, GAUSS_W,
                 BILATERAL_SXY / scale_factor, BILATERAL_SRGB, BILATERAL_W, ptr(ws), ptr(q), ptr(pred), stream())
            return q, pred
        ws = _workspace(dev, H, W)
        call("mx_crf_inference", ptr(im), ptr(p), L, H, W, int(t), float(confidence), GAUSS_SXY / scale_factor, GAUSS_W,
             BILATERAL_SXY / scale_factor, BILATERAL_SRGB, BILATERAL_W, float(trunc), ptr(ws), ptr(q), ptr(pred), stream())
    return q, pred


def crf_inference(img, probs, t: int = 2, scale_factor: float = 1.5, labels: int = 21, confidence: float = 0.5, *,
                  trunc: float = 4.0, pairwise: str = "window") -> torch.Tensor:
    """src/imutils.py:439 (same name, arguments and defaults).  img: uint8 [H,W,3] numpy array or tensor; probs: [labels,H,W]
    numpy array or tensor (it may be un-normalised: the formula is applied as it stands).  Returns Q_t fp32 [labels,H,W] on
    the device.  pairwise: "window" (the exact windowed sums) or "lattice" (the permutohedral lattice; trunc is ignored)."""
    return crf_run(img, probs, t, scale_factor, labels, confidence, trunc, pairwise=pairwise)[0]


# imutils.py:487-488: addPairwiseGaussian(sxy=3, compat=3), addPairwiseBilateral(sxy=50, srgb=5, compat=10)
LABEL_GAUSS_SXY, LABEL_GAUSS_W = 3.0, 3.0
LABEL_BILATERAL_SXY, LABEL_BILATERAL_SRGB, LABEL_BILATERAL_W = 50.0, 5.0, 10.0
LABEL_MODEL = (LABEL_GAUSS_SXY, LABEL_GAUSS_W, LABEL_BILATERAL_SXY, LABEL_BILATERAL_SRGB, LABEL_BILATERAL_W)

_label_ws: Dict[tuple, torch.Tensor] = {}


def label_workspace(dev: torch.device, H: int, W: int) -> torch.Tensor:
    """The workspace of mx_ir_label / mx_crf_label for an image size (it does not depend on L); one is kept per size."""
    return cached_workspace(_label_ws, lib().mx_ir_label_ws, dev, (2, H, W), 4)


def crf_label_run(img, labels, t: int, n_labels: int, gt_prob: float, trunc: float, want_q: bool = False,
                  want_pred: bool = True, *, pairwise: str = "window") -> Tuple[Optional[torch.Tensor], Optional[torch.Tensor]]:
    """One enqueue of mx_crf_label (pairwise="lattice": mx_crf_label_lattice) on the current stream; returns (Q_t fp32 [L,H,W] or
    None, argmax uint8 [H,W] or None)."""
    lattice = check_pairwise(pairwise)
    lab = labels if torch.is_tensor(labels) else torch.from_numpy(np.ascontiguousarray(labels))
    if lab.dim() != 2 or lab.dtype.is_floating_point or lab.dtype == torch.bool:
        raise ValueError(f"labels must be an integer map [H,W] (got {lab.dtype} {tuple(lab.shape)})")
    dev = lab.device if lab.is_cuda else torch.device("cuda", torch.cuda.current_device())
    lab = lab.to(dev, torch.int32).contiguous()
    H, W = lab.shape
    im = device_image(img, dev)
    if tuple(im.shape[:2]) != (H, W):
        raise ValueError(f"img is {tuple(im.shape[:2])}, labels {(H, W)}")
    L = int(n_labels)
    with torch.cuda.device(dev):
        q = torch.empty(L, H, W, dtype=torch.float32, device=dev) if want_q else None
        pred = torch.empty(H, W, dtype=torch.uint8, device=dev) if want_pred else None
        if lattice:
            ws = crf_lattice_workspace(dev, L, H, W)
            call("mx_crf_label_lattice", ptr(im), ptr(lab), L, H, W, int(t), float(gt_prob), *LABEL_MODEL, ptr(ws), ptr(pred), ptr(q),
                 stream())
            return q, pred
        ws = label_workspace(dev, H, W)
        call("mx_crf_label", ptr(im), ptr(lab), L, H, W, int(t), float(gt_prob), *LABEL_MODEL, float(trunc), ptr(ws), ptr(pred),
             ptr(q), stream())
    return q, pred


def crf_inference_label(img, labels, t: int = 10, n_labels: int = 21, gt_prob: float = 0.7, *, trunc: float = 4.0,
                        pairwise: str = "window") -> torch.Tensor:
    """src/imutils.py:477 (same name, arguments and defaults): the CRF whose unary is unary_from_labels(labels, n_labels, gt_prob,
    zero_unsure=False), Gaussian term sxy 3 / weight 3, bilateral term sxy 50, srgb 5 / weight 10.  img: uint8 [H,W,3] numpy array
    or tensor; labels: int [H,W] numpy array or tensor with values 0..n_labels-1.  Returns argmax_l Q_t as a uint8 [H,W] tensor on
    the device.  As for crf_inference, the sums run exactly over the window R_m = ceil(trunc * sxy_m), which is part of the model:
    label maps are not bit-identical with pydensecrf's; what is pinned is this model against an fp64 restatement
    (tests/ir_label_ref.py).  pairwise="lattice" runs both kernels on permutohedral lattices instead (trunc is ignored): see the
    module docstring."""
    return crf_label_run(img, labels, t, n_labels, gt_prob, trunc, pairwise=pairwise)[1]
