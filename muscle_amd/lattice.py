"""Permutohedral-lattice filter on the HIP path (csrc/lattice.hip; Adams, Baek & Davis 2010): the approximation of

    out[c,i] = sum_j exp(-0.5 |f(i) - f(j)|^2) x[c,j]        f = (x, y) / sxy  or  (x / sxy, y / sxy, r / srgb, g / srgb, b / srgb)

that pydensecrf evaluates the CRFs of src/imutils.py:439-456 and :477-491 with.  Its cost does not grow with sxy.  It is a
different model from the exact windowed sums of muscle_amd.crf (include/muscle_hip.h states the algorithm; tests/lattice_ref.py
restates it in numpy), selectable there with pairwise="lattice".  Parity with pydensecrf itself is not pinned.
"""
from __future__ import annotations

from typing import Callable, Dict, Optional

import numpy as np
import torch

from ._lib import MuscleHipError, call, lib, ptr, stream

PAIRWISE = ("window", "lattice")


def check_pairwise(pairwise: str) -> bool:
    """True for "lattice", False for "window"; anything else is a ValueError (before the device is touched)."""
    if pairwise not in PAIRWISE:
        raise ValueError(f"pairwise must be one of {PAIRWISE} (got {pairwise!r})")
    return pairwise == "lattice"


def device_image(img, dev: Optional[torch.device] = None) -> torch.Tensor:
    """img (numpy array, PIL-backed array or tensor) checked as uint8 [H,W,3], contiguous on dev (None: the tensor's own device
    if it is on one, else the current one)."""
    t = img if torch.is_tensor(img) else torch.from_numpy(np.array(img))       # a copy: PIL-backed arrays are read-only
    if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
        raise ValueError(f"img must be uint8 [H,W,3] (got {t.dtype} {tuple(t.shape)})")
    if dev is None:
        dev = t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())
    return t.to(dev).contiguous()


def cached_workspace(cache: Dict[tuple, torch.Tensor], size_fn: Callable[..., int], dev: torch.device, args: tuple,
                     keep: int) -> torch.Tensor:
    """The workspace of size_fn(*args) bytes on dev out of cache, which holds at most `keep` of them (the oldest one goes): a few
    image sizes at most stay resident."""
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),) + args
    ws = cache.get(key)
    if ws is None:
        nbytes = size_fn(*args)
        if nbytes < 0:
            raise MuscleHipError(f"{size_fn.__name__} failed: {lib().mx_last_error().decode()}")
        if len(cache) >= keep:
            cache.pop(next(iter(cache)))
        ws = cache[key] = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
    return ws


class PermutohedralLattice:
    """The lattice of one uint8 image [H,W,3] (numpy array or tensor) and one kernel: srgb None (or <= 0) is the spatial kernel
    (D = 2), else the bilateral one (D = 5).  Built once; `filter` may be called any number of times with up to max_channels
    channels."""

    def __init__(self, img, sxy: float, srgb: Optional[float] = None, *, max_channels: int = 32):
        self.img = device_image(img)
        dev = self.img.device
        self.H, self.W = int(self.img.shape[0]), int(self.img.shape[1])
        self.D = 5 if (srgb is not None and srgb > 0) else 2
        self.sxy, self.srgb = float(sxy), float(srgb) if self.D == 5 else 0.0
        self.max_channels = int(max_channels)
        nbytes = lib().mx_lattice_ws(self.D, self.H, self.W, self.max_channels)
        if nbytes < 0:
            raise MuscleHipError(f"mx_lattice_ws failed: {lib().mx_last_error().decode()}")
        with torch.cuda.device(dev):
            self.ws = torch.empty((nbytes + 3) // 4, dtype=torch.float32, device=dev)
            call("mx_lattice_build", ptr(self.img), self.H, self.W, self.sxy, self.srgb, ptr(self.ws), stream())

    def filter(self, x: torch.Tensor) -> torch.Tensor:
        """x fp32 [C,H,W] (or [H,W]) -> the filtered maps, same shape, on the device."""
        flat = x.dim() == 2
        v = (x[None] if flat else x).to(self.ws.device, torch.float32).contiguous()
        if v.dim() != 3 or tuple(v.shape[1:]) != (self.H, self.W) or not 1 <= v.shape[0] <= self.max_channels:
            raise ValueError(f"x must be [C<={self.max_channels},{self.H},{self.W}] (got {tuple(x.shape)})")
        out = torch.empty_like(v)
        with torch.cuda.device(self.ws.device):
            call("mx_lattice_filter", ptr(self.ws), ptr(v), ptr(out), int(v.shape[0]), stream())
        return out[0] if flat else out

    def export(self):
        """(vid int32 [N,D+1], weight fp32 [N,D+1], keys int32 [M,D], nbr int32 [2(D+1),cap], M) as tensors on the device, keys cut
        to the M vertices; for tests."""
        N, D1 = self.H * self.W, self.D + 1
        cap, dev = N * D1, self.ws.device
        vid = torch.empty(N, D1, dtype=torch.int32, device=dev)
        w = torch.empty(N, D1, dtype=torch.float32, device=dev)
        keys = torch.empty(cap, self.D, dtype=torch.int32, device=dev)
        nbr = torch.empty(2 * D1, cap, dtype=torch.int32, device=dev)
        count = torch.empty(1, dtype=torch.int32, device=dev)
        with torch.cuda.device(dev):
            call("mx_lattice_export", ptr(self.ws), ptr(vid), ptr(w), ptr(keys), ptr(nbr), ptr(count), stream())
        M = int(count.item())
        return vid, w, keys[:M], nbr, M


_crf_ws: Dict[tuple, torch.Tensor] = {}


def crf_lattice_workspace(dev: torch.device, L: int, H: int, W: int) -> torch.Tensor:
    """The workspace of the mx_*_lattice CRF entries for L labels and an image size; a few are kept."""
    return cached_workspace(_crf_ws, lib().mx_crf_lattice_ws, dev, (L, H, W), 2)
