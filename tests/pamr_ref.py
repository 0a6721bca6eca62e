"""Numpy restatement of the PAMR model that include/muscle_hip.h states (mx_pamr_affinity ..), with a dtype switch: in float64 it is
the reference of the kernels, in float32 it measures what fp32 rounding alone does to the model on the same input (the yardstick e32
of tests/test_gpu_pamr.py)."""
import numpy as np

OFFSETS = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 1), (1, -1), (1, 0), (1, 1))         # (dy, dx), neighbour k of a dilation
NINE = ((-1, -1), (-1, 0), (-1, 1), (0, -1), (0, 0), (0, 1), (1, -1), (1, 0), (1, 1))    # the sample of the deviation: centre included
DEFAULT_DILATIONS = (1, 2, 4, 8, 12, 24)


def planar(img, dtype=np.float64):
    """uint8 [H,W,3] / [N,H,W,3] or float [3,H,W] / [N,3,H,W] -> dtype [N,3,H,W]."""
    a = np.asarray(img)
    if a.dtype == np.uint8:
        a = a[None] if a.ndim == 3 else a
        return np.ascontiguousarray(a.transpose(0, 3, 1, 2)).astype(dtype)
    a = a[None] if a.ndim == 3 else a
    return a.astype(dtype)


def shifted(x, dy, dx):
    """x[..., clamp(y + dy), clamp(x + dx)]: replicate padding."""
    H, W = x.shape[-2:]
    ys = np.clip(np.arange(H) + dy, 0, H - 1)
    xs = np.clip(np.arange(W) + dx, 0, W - 1)
    return x[..., ys[:, None], xs[None, :]]


def affinity(img, dilations=DEFAULT_DILATIONS, dtype=np.float64):
    """w [N,P,H,W], P = 8 len(dilations), in dtype."""
    I = planar(img, dtype)                                                               # [N,3,H,W]
    D = len(dilations)
    sample = np.stack([shifted(I, d * dy, d * dx) for d in dilations for dy, dx in NINE], axis=0)      # [9D,N,3,H,W]
    cnt = dtype(9 * D)
    mean = sample.sum(axis=0, dtype=dtype) / cnt
    var = ((sample - mean) ** 2).sum(axis=0, dtype=dtype) / (cnt - dtype(1))
    den = dtype(1e-8) + dtype(0.1) * np.sqrt(var)                                        # [N,3,H,W]
    a = np.stack([(-np.abs(I - shifted(I, d * dy, d * dx)) / den).sum(axis=1, dtype=dtype) / dtype(3)
                  for d in dilations for dy, dx in OFFSETS], axis=1)                     # [N,P,H,W]
    e = np.exp(a - a.max(axis=1, keepdims=True))
    w = e / e.sum(axis=1, keepdims=True, dtype=dtype)
    assert w.dtype == dtype
    return w


def step(w, m, dilations=DEFAULT_DILATIONS):
    """One iteration: m [N,C,H,W] -> sum_p w_p m[nbr_p], p ascending from zero, in w's dtype."""
    out = np.zeros_like(m)
    p = 0
    for d in dilations:
        for dy, dx in OFFSETS:
            out = out + w[:, p:p + 1] * shifted(m, d * dy, d * dx)
            p += 1
    return out


def pamr(img, mask, num_iter=10, dilations=DEFAULT_DILATIONS, dtype=np.float64):
    """mask [C,H,W] / [N,C,H,W] -> m_{num_iter}, same shape, in dtype; (w is returned too)."""
    m = np.asarray(mask)
    flat = m.ndim == 3
    m = (m[None] if flat else m).astype(dtype)
    w = affinity(img, dilations, dtype)
    if w.shape[0] != m.shape[0] or w.shape[2:] != m.shape[2:]:
        raise ValueError(f"img gives w {w.shape}, mask is {m.shape}")
    for _ in range(num_iter):
        m = step(w, m, dilations)
    assert m.dtype == dtype
    return (m[0] if flat else m), w
