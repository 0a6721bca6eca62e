"""Numpy restatement of the dense-CRF model of muscle_amd.crf (the model src/imutils.py:439-456 hands to pydensecrf, with
the sums over j taken exactly over a square window), written from its definition:

    U[l,i]   = -log(clip(confidence * probs[l,i] + (1 - confidence) / L, 1e-5, 1))
    k_m(i,j) = exp(-0.5 * |f_m(i) - f_m(j)|^2)  if |x_i-x_j| <= R_m and |y_i-y_j| <= R_m else 0       (j == i included)
               f_gauss = (x, y) / sxy_g;  f_bilateral = (x / sxy_b, y / sxy_b, r / srgb, g / srgb, b / srgb)
               sxy_g = 3 / scale_factor (weight 1), sxy_b = 32 / scale_factor, srgb = 10 (weight 10)
               R_m = ceil(trunc * sxy_m); trunc <= 0: all pairs
    n_m(i)   = 1 / sqrt(sum_j k_m(i,j) + 1e-20)
    Q_0      = softmax_l(-U)
    Q_{s+1}  = softmax_l(-U + sum_m w_m n_m(i) sum_j k_m(i,j) n_m(j) Q_s[l,j])

Dense N x N kernel matrices, built in chunks of rows.  `dtype` switches the whole arithmetic (np.float64 is the reference;
np.float32 measures what fp32 rounding alone does to the same model)."""
import math

import numpy as np

GAUSS_SXY, GAUSS_W = 3.0, 1.0
BILATERAL_SXY, BILATERAL_SRGB, BILATERAL_W = 32.0, 10.0, 10.0
_KEEP_BYTES = 160 << 20          # kernel matrices up to this size are built once and kept for the iterations


def standard_input():
    """The standard image: three colour regions with noise, and a smooth probability map whose label borders are
    deliberately off the colour edges.  Returns (img uint8 [40,56,3], probs float64 [21,40,56])."""
    import scipy.ndimage
    g = np.random.default_rng(0)
    H, W, L = 40, 56, 21
    img = np.zeros((H, W, 3))
    img[:, :20] = [200, 30, 30]
    img[10:30, 20:45] = [20, 180, 60]
    img[:, 45:] = [30, 40, 200]
    img = np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    lab = np.zeros((H, W), int)
    lab[:, :23] = 3
    lab[8:33, 17:48] = 7
    lab[:, 43:] = 15
    logit = g.normal(0, 1.0, (L, H, W))
    for k in range(L):
        logit[k] += 2.5 * (lab == k)
    logit = scipy.ndimage.gaussian_filter(logit, (0, 3, 3)) * 3
    probs = np.exp(logit)
    probs /= probs.sum(0, keepdims=True)
    return img, probs


def radius(trunc, sxy):
    return None if not trunc > 0 else int(math.ceil(trunc * sxy))


def unary(probs, confidence=0.5, dtype=np.float64):
    p = np.asarray(probs, dtype=dtype)
    L = p.shape[0]
    c = np.clip(dtype(confidence) * p + dtype(1.0 - confidence) / dtype(L), dtype(1e-5), dtype(1.0))
    return -np.log(c)


def softmax0(x):
    e = np.exp(x - x.max(0, keepdims=True))
    return e / e.sum(0, keepdims=True)


class Kernel:
    """k(i, .) for rows of pixels; feats [N,D] already divided by their widths, xy integer coordinates [N,2]."""

    def __init__(self, feats, xy, R, dtype, chunk=256):
        self.f = np.ascontiguousarray(feats, dtype=dtype)
        self.xy, self.R, self.dtype, self.chunk = xy, R, dtype, chunk
        self.N = self.f.shape[0]
        self.kept = None
        if self.N * self.N * np.dtype(dtype).itemsize <= _KEEP_BYTES:
            self.kept = [self._rows(a, min(a + chunk, self.N)) for a in range(0, self.N, chunk)]

    def _rows(self, a, b):
        d2 = np.zeros((b - a, self.N), dtype=self.dtype)
        for d in range(self.f.shape[1]):
            diff = self.f[a:b, d, None] - self.f[None, :, d]
            d2 += diff * diff
        k = np.exp(self.dtype(-0.5) * d2)
        if self.R is not None:
            for d in range(2):
                k *= np.abs(self.xy[a:b, d, None] - self.xy[None, :, d]) <= self.R
        return k

    def apply(self, v):
        """sum_j k(i,j) v[j] for v [N] or [N,C]."""
        out = np.empty((self.N,) + v.shape[1:], dtype=self.dtype)
        for n, a in enumerate(range(0, self.N, self.chunk)):
            b = min(a + self.chunk, self.N)
            k = self.kept[n] if self.kept is not None else self._rows(a, b)
            out[a:b] = k @ v
        return out


def kernels(img, scale_factor=1.5, trunc=4.0, dtype=np.float64):
    """(gauss, bilateral) Kernel objects of the uint8 image img [H,W,3]."""
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int64)
    sg, sb = GAUSS_SXY / scale_factor, BILATERAL_SXY / scale_factor
    pos = xy.astype(dtype)
    rgb = img.reshape(-1, 3).astype(dtype)
    fg = pos / dtype(sg)
    fb = np.concatenate([pos / dtype(sb), rgb / dtype(BILATERAL_SRGB)], 1)
    return Kernel(fg, xy, radius(trunc, sg), dtype), Kernel(fb, xy, radius(trunc, sb), dtype)


def normalizers(img, scale_factor=1.5, trunc=4.0, dtype=np.float64, ks=None):
    """(n_gauss, n_bilateral) [H,W]."""
    H, W = img.shape[:2]
    ks = ks or kernels(img, scale_factor, trunc, dtype)
    one = np.ones(H * W, dtype=dtype)
    return tuple((dtype(1.0) / np.sqrt(k.apply(one) + dtype(1e-20))).reshape(H, W) for k in ks)


def crf_ref(img, probs, t, scale_factor=1.5, confidence=0.5, trunc=4.0, dtype=np.float64):
    """Q_t [L,H,W] in `dtype`."""
    L, H, W = probs.shape
    U = unary(probs, confidence, dtype).reshape(L, -1)
    Q = softmax0(-U)
    if t == 0:
        return Q.reshape(L, H, W)
    ks = kernels(img, scale_factor, trunc, dtype)
    ns = [n.ravel() for n in normalizers(img, scale_factor, trunc, dtype, ks)]
    ws = (dtype(GAUSS_W), dtype(BILATERAL_W))
    for _ in range(t):
        x = -U
        for k, n, w in zip(ks, ns, ws):
            x = x + w * (n[:, None] * k.apply(n[:, None] * Q.T)).T
        Q = softmax0(x)
    return Q.reshape(L, H, W)
