"""numpy restatement of the rule muscle_amd.irn_sweep counts by (infer_irn.py:78-92 + src/evaluation.py:36-50), in fp32 with the
operation order of csrc/irn_soft.h: the 4x half-pixel upsample as lerp_b(lerp_b(m00, m01, wx), lerp_b(m10, m11, wx), wy) with
lerp_b(a, b, w) = fma(1 - w, a, rn(w * b)), the division by the maximum, then - per threshold, one plain loop, no binning - the
label kernel's `v > best` scan and the (TP, P, T) counts of seg_confusion_kernel.  The maximum is an input: the label step
takes it from its own kernel (mx_irn_up_max), and so does the sweep.
"""
import numpy as np


def _fma32(x, a, p):
    """rn32(x * a + p) for fp32 arrays, exactly: the product is exact in fp64, the sum is rounded to odd in fp64 (TwoSum tells
    whether and on which side it was inexact), and 53 >= 2 * 24 + 2 bits make the final rounding to fp32 the fused one."""
    xa = x.astype(np.float64) * a.astype(np.float64)
    p = p.astype(np.float64)
    with np.errstate(invalid="ignore", over="ignore"):
        s = xa + p
        bb = s - xa
        err = (xa - (s - bb)) + (p - bb)
        even = (s.view(np.int64) & 1) == 0
        fix = np.isfinite(s) & (err != 0) & even
        toward = np.where(err > 0, np.inf, -np.inf)
        s = np.where(fix, np.nextafter(s, toward), s)
    return s.astype(np.float32)


def _lerp_b(a, b, w):
    p = (w * b).astype(np.float32)                       # rn(w * b), fp32 operands
    return _fma32((np.float32(1) - w).astype(np.float32), a, p)


def up4(m, H, W):
    """m fp32 [h,w] -> the top-left HxW crop of its 4x bilinear (align_corners=False) upsample, irn_up4 of irn_soft.h."""
    m = np.asarray(m, np.float32)
    h, w = m.shape

    def taps(n_out, n_in):
        s = ((np.arange(n_out, dtype=np.float32) + np.float32(0.5)) * np.float32(0.25) - np.float32(0.5)).astype(np.float32)
        s = np.maximum(s, np.float32(0))
        i0 = np.minimum(s.astype(np.int32), n_in - 1)
        i1 = i0 + (i0 < n_in - 1)
        return i0, i1, (s - i0.astype(np.float32)).astype(np.float32)

    y0, y1, wy = taps(H, h)
    x0, x1, wx = taps(W, w)
    wxb, wyb = np.broadcast_to(wx[None, :], (H, W)), np.broadcast_to(wy[:, None], (H, W))
    r0 = _lerp_b(m[y0][:, x0], m[y0][:, x1], wxb)
    r1 = _lerp_b(m[y1][:, x0], m[y1][:, x1], wxb)
    return _lerp_b(r0, r1, wyb)


def soft_values(rw, H, W, mx):
    """rw fp32 [C,h,w], mx the fp32 maximum -> v fp32 [C,H,W] = up4 / mx (irn_soft_value); mx = 0 gives NaN where up4 is 0."""
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.stack([up4(m, H, W) / np.float32(mx) for m in rw]).astype(np.float32) if len(rw) else np.zeros((0, H, W), np.float32)


def label_from_values(v, keys, t):
    """irn_label_kernel's scan: best = t, label 0; channel by channel `if v > best`: the first maximum above t wins, a tie with t
    stays background, a NaN never wins.  v [Kp,H,W], keys[j] + 1 = the label of map j."""
    best = np.full(v.shape[1:], np.float32(t), np.float32)
    lab = np.zeros(v.shape[1:], np.uint8)
    with np.errstate(invalid="ignore"):
        for j, k in enumerate(keys):
            win = v[j] > best
            best = np.where(win, v[j], best)
            lab = np.where(win, np.uint8(int(k) + 1), lab)
    return lab


def confusion(label, gt, K):
    """seg_confusion_kernel: over pixels with gt < 255, P[pred]++ (pred < K), T[gt]++ and TP[gt] += (pred == gt) (gt < K)."""
    c = np.zeros((K, 3), np.int64)
    ok = gt < 255
    for k in range(K):
        c[k, 0] = np.count_nonzero(ok & (gt == k) & (label == k))
        c[k, 1] = np.count_nonzero(ok & (label == k))
        c[k, 2] = np.count_nonzero(ok & (gt == k))
    return c


def counts_from_values(v, keys, gt, thresholds, K):
    """int64 [T,K,3]: one plain loop over the thresholds."""
    return np.stack([confusion(label_from_values(v, keys, t), gt, K) for t in thresholds])


def sweep_counts(rw, keys, vmax, gt, H, W, thresholds, K):
    """rw fp32 [E,Kp,h,w] (the kept channels), keys [Kp], vmax fp32 [E] -> int64 [E,T,K,3]."""
    return np.stack([counts_from_values(soft_values(rw[e], H, W, vmax[e]), keys, gt, thresholds, K) for e in range(len(rw))])
