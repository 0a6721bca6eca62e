"""Numpy restatement of the dense-CRF energy loss (include/muscle_hip.h, mx_crf_loss_fwd / mx_crf_loss_bwd; muscle_amd/crf_loss.py)
in a chosen dtype: float64 is the truth, float32 the rounding yardstick of the GPU tests.  All pairs of cells of an item are
formed as one dense [hw, hw] matrix, so it is for small maps only.  The colours are integers (rint) and their cell means exact
in either dtype; everything else - softmax, pooling, kernel, messages, the sums D and S . M, the gradient - is computed in dtype."""
import math

import numpy as np

MEAN = np.array([0.485, 0.456, 0.406])
STD = np.array([0.229, 0.224, 0.225])
COLS = 32


def color_norm(u8):
    """uint8 [N,H,W,3] -> the normalised float32 [N,3,H,W] batch image (src/imutils.py:383)."""
    x = (np.asarray(u8, np.float64) / 255.0 - MEAN) / STD
    return np.ascontiguousarray(np.moveaxis(x, -1, 1)).astype(np.float32)


def rgb_of(img):
    """clamp(rint((img * std + mean) * 255), 0, 255) of a normalised [N,3,H,W] image, float64 (integers)."""
    x = (np.asarray(img, np.float64) * STD[None, :, None, None] + MEAN[None, :, None, None]) * 255.0
    return np.clip(np.rint(x), 0, 255)


def inside(window, N, H, W, dtype):
    m = np.zeros((N, H, W), dtype)
    for n in range(N):
        y0, x0, y1, x1 = (0, 0, H, W) if window is None else (int(v) for v in window[n])
        y0, x0, y1, x1 = max(y0, 0), max(x0, 0), min(y1, H), min(x1, W)
        if y1 > y0 and x1 > x0:
            m[n, y0:y1, x0:x1] = 1
    return m


def _pool(a, f, dtype):
    *lead, H, W = a.shape
    return a.reshape(*lead, H // f, f, W // f, f).sum(axis=(-3, -1), dtype=dtype) * dtype(1.0 / (f * f))


def radius(trunc, sxy, f, h, w):
    return max(h, w) if not trunc > 0 else int(math.ceil(trunc * sxy / f))


def energy(seg, img, window=None, f=1, sxy=80.0, srgb=15.0, trunc=2.0, dtype=np.float64, g=1.0):
    """seg [N,K,H,W], img [N,3,H,W] (normalised), window [N,4] or None.
    Returns {"loss", "D", "SM" (scalars of dtype), "M" [N,h,w,K], "Z" [N,h,w], "gseg" [N,K,H,W] = g * d loss / d seg, "P", "S", "r"}."""
    dtype = np.dtype(dtype).type
    seg = np.asarray(seg)
    N, K, H, W = seg.shape
    assert H % f == 0 and W % f == 0
    h, w = H // f, W // f
    x = seg.astype(dtype)
    e = np.exp(x - x.max(1, keepdims=True))
    P = e / e.sum(1, keepdims=True, dtype=dtype)
    inm = inside(window, N, H, W, dtype)
    r = _pool(inm, f, dtype)
    S = _pool(P * inm[:, None], f, dtype)
    col = _pool(rgb_of(img), f, np.float64).astype(dtype)                  # exact: f^2 is a power of two, sums below 2^24
    s = dtype(sxy) / dtype(f)
    R = radius(trunc, sxy, f, h, w)
    yy, xx = (a.reshape(-1) for a in np.mgrid[0:h, 0:w])
    dy, dx = yy[:, None] - yy[None, :], xx[:, None] - xx[None, :]
    inwin = (np.abs(dx) <= R) & (np.abs(dy) <= R)
    d2 = (dx * dx + dy * dy).astype(dtype) / (dtype(2) * s * s)
    M = np.zeros((N, h * w, K), dtype)
    Z = np.zeros((N, h * w), dtype)
    for n in range(N):
        c = col[n].reshape(3, -1).T
        dc = c[:, None, :] - c[None, :, :]
        dc2 = (dc * dc).sum(-1, dtype=dtype) / (dtype(2) * dtype(srgb) * dtype(srgb))
        k = np.where(inwin, np.exp(-d2 - dc2), dtype(0)).astype(dtype)
        M[n] = k @ S[n].reshape(K, -1).T
        Z[n] = k @ r[n].reshape(-1)
    D = (r.reshape(N, -1) * Z).sum(dtype=dtype)
    SM = (np.moveaxis(S.reshape(N, K, -1), 1, 2) * M).sum(dtype=dtype)
    loss = (D - SM) / D if D > 0 else dtype(0)
    M = M.reshape(N, h, w, K)
    Mp = np.moveaxis(M, -1, 1).repeat(f, 2).repeat(f, 3)                   # M at the pixel's cell, [N,K,H,W]
    dot = (P * Mp).sum(1, keepdims=True, dtype=dtype)
    coef = dtype(g) * dtype(-2) / (D * dtype(f * f)) if D > 0 else dtype(0)
    gseg = coef * inm[:, None] * P * (Mp - dot)
    assert gseg.dtype == dtype and M.dtype == dtype
    return {"loss": loss, "D": D, "SM": SM, "M": M, "Z": Z.reshape(N, h, w), "gseg": gseg, "P": P, "S": S, "r": r}
