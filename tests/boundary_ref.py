"""A numpy restatement of the boundary evaluation ("Boundary evaluation"), written straight from the definition and
independently of muscle_amd/evaluation.py: a brute-force window scan for the distance maps, boolean masks for the six-row table,
scalar float64 arithmetic for the metrics.  Slow and obvious on purpose; the tests compare the product with it exactly.
`edge_dist_erosion` / `tables_erosion` are the same maps from per-class scipy erosions, the form a host implementation takes
(tools/bench_boundary_eval.py times it; tests/test_cpu_boundary_eval.py shows the two forms agree)."""
import math

import numpy as np


def edge_dist(label, dmax, edge):
    """dist[p] = min(dmax + 1, min over q with label[q] != label[p] of max(|dy|, |dx|)); with edge, q also runs over the positions
    outside the image.  Every offset of the (2 dmax + 1)^2 window is visited."""
    L = np.asarray(label).astype(np.int32)
    H, W = L.shape
    pad = np.full((H + 2 * dmax, W + 2 * dmax), -1, np.int32)               # -1: outside the image
    pad[dmax:dmax + H, dmax:dmax + W] = L
    dist = np.full((H, W), dmax + 1, np.int32)
    for dy in range(-dmax, dmax + 1):
        for dx in range(-dmax, dmax + 1):
            d = max(abs(dy), abs(dx))
            if d == 0:
                continue
            q = pad[dmax + dy:dmax + dy + H, dmax + dx:dmax + dx + W]
            hit = ((q >= 0) & (q != L)) | ((q < 0) & bool(edge))
            dist[hit & (dist > d)] = d
    return dist.astype(np.uint8)


def edge_dist_erosion(label, dmax, edge):
    """The same map from d erosions of every value's mask with a 3x3 square: border_value 0 makes the outside count (edge = 1),
    border_value 1 leaves it out (edge = 0)."""
    from scipy.ndimage import binary_erosion
    L = np.asarray(label)
    dist = np.full(L.shape, dmax + 1, np.uint8)
    sq = np.ones((3, 3), bool)
    for c in np.unique(L):
        mask = L == c
        er = mask
        for d in range(1, dmax + 1):
            er = binary_erosion(er, sq, border_value=0 if edge else 1)
            dist[mask & ~er & (dist == dmax + 1)] = d
            if not er.any():
                break
    return dist


def image_radius(H, W, ratio, dmax):
    return min(dmax, max(1, round(ratio * math.hypot(H, W))))


def tables(pred, gt, K, dmax, ratio=0.02, dist=edge_dist):
    """(hist int64 [6, K, dmax + 2], ratio int64 [3, K]) of one image, row by row as the specification's table states them."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    H, W = gt.shape
    dt = dist(gt, dmax, 0).astype(np.int64)
    db = dist(gt, dmax, 1).astype(np.int64)
    dp = dist(pred, dmax, 1).astype(np.int64)
    hist = np.zeros((6, K, dmax + 2), np.int64)
    rat = np.zeros((3, K), np.int64)
    d_img = image_radius(H, W, ratio, dmax)
    live = gt != 255
    for c in range(K):
        g, p = live & (gt == c), live & (pred == c)
        tp = g & p
        for b in range(1, dmax + 2):
            hist[0, c, b] = (g & (dt == b)).sum()
            hist[1, c, b] = (p & (dt == b)).sum()
            hist[2, c, b] = (tp & (dt == b)).sum()
            hist[3, c, b] = (g & (db == b)).sum()
            hist[4, c, b] = (p & (dp == b)).sum()
            hist[5, c, b] = (tp & (np.maximum(db, dp) == b)).sum()
        rat[0, c] = (g & (db <= d_img)).sum()
        rat[1, c] = (p & (dp <= d_img)).sum()
        rat[2, c] = (tp & (db <= d_img) & (dp <= d_img)).sum()
    return hist, rat


def tables_erosion(pred, gt, K, dmax, ratio=0.02):
    return tables(pred, gt, K, dmax, ratio, dist=edge_dist_erosion)


def confusion(pred, gt, K):
    """The (TP, P, T) table [K, 3] of the whole-image mIoU: pixels with gt == 255 are skipped."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    live = gt != 255
    return np.array([[(live & (gt == c) & (pred == c)).sum(), (live & (pred == c)).sum(), (live & (gt == c)).sum()] for c in range(K)],
                    np.int64)


def mean_iou(T, P, TP):
    """Mean over ALL classes of TP / (T + P - TP + 1e-10), in per cent."""
    iou = [int(TP[c]) / (int(T[c]) + int(P[c]) - int(TP[c]) + 1e-10) for c in range(len(T))]
    return float(np.mean(np.array(iou)) * 100), [v * 100 for v in iou]


def within(hist, d):
    """The six count rows [6, K] within distance d: bins 1..d."""
    return np.asarray(hist)[:, :, 1:d + 1].sum(axis=2)


def trimap_miou(hist, d):
    c = within(hist, d)
    return mean_iou(c[0], c[1], c[2])[0]


def boundary_miou(hist, d):
    c = within(hist, d)
    return mean_iou(c[3], c[4], c[5])[0]


def ratio_miou(rat):
    """(mean, per-class list) of Boundary IoU at the per-image radius."""
    return mean_iou(rat[0], rat[1], rat[2])


def blobs(H, W, n, K, seed, void_rows=()):
    """A label map of n Voronoi cells with classes drawn from 0..K-1, rows `void_rows` set to 255."""
    rng = np.random.RandomState(seed)
    cy, cx = rng.randint(0, H, n), rng.randint(0, W, n)
    cls = rng.randint(0, K, n)
    yy, xx = np.mgrid[0:H, 0:W]
    near = np.argmin((yy[None] - cy[:, None, None]) ** 2 + (xx[None] - cx[:, None, None]) ** 2, axis=0)
    out = cls[near].astype(np.uint8)
    for r in void_rows:
        out[r] = 255
    return out
