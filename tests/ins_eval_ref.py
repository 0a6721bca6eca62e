"""A numpy restatement of the instance evaluation ("Instance evaluation"), written independently of
muscle_amd/ins_eval.py: plain loops over pixels, objects and predictions, no helper shared with the product.  Slow and obvious
on purpose; the tests compare the product with it (tables exactly, AP to 1e-12)."""
import math

import numpy as np


def label_table(a, b, A, B):
    """table[a[i], b[i]] += 1; returns (table int64 [A+1, B+1], number of pixels with a value outside 0..A / 0..B)."""
    t = np.zeros((A + 1, B + 1), np.int64)
    a = np.asarray(a).reshape(-1).astype(np.int64)
    b = np.asarray(b).reshape(-1).astype(np.int64)
    ok = (a >= 0) & (a <= A) & (b <= B)
    np.add.at(t, (a[ok], b[ok]), 1)
    return t, int((~ok).sum())


def mask_table(masks, b, B):
    """Row 0: every pixel by its b value; row p+1: the set pixels of mask p by their b value.  Returns (table, bad pixels)."""
    masks = np.asarray(masks)
    b = np.asarray(b).reshape(-1).astype(np.int64)
    n = masks.shape[0]
    t = np.zeros((n + 1, B + 1), np.int64)
    ok = b <= B
    np.add.at(t[0], b[ok], 1)
    for p in range(n):
        on = (masks[p].reshape(-1) != 0) & ok
        np.add.at(t[p + 1], b[on], 1)
    return t, int((~ok).sum())


def iou_from_masks(masks, G, m):
    """[n, m] IoU of boolean masks against the objects 1..m of G, by forming every intersection and union."""
    masks = np.asarray(masks) != 0
    out = np.zeros((masks.shape[0], m))
    for p in range(masks.shape[0]):
        for j in range(m):
            g = G == j + 1
            union = int((masks[p] | g).sum())
            out[p, j] = int((masks[p] & g).sum()) / union if union else 0.0
    return out


def iou_from_table(t, overlapping):
    t = np.asarray(t, np.int64)
    n, m = t.shape[0] - 1, t.shape[1] - 1
    out = np.zeros((n, m))
    for p in range(n):
        area_p = int(t[p + 1].sum())
        for j in range(m):
            area_g = int(t[0, j + 1]) if overlapping else int(t[:, j + 1].sum())
            inter = int(t[p + 1, j + 1])
            union = area_p + area_g - inter
            out[p, j] = inter / union if union else 0.0
    return out


def gt_instances(cls_png, obj_png, num_cls=20):
    cls_png, obj_png = np.asarray(cls_png), np.asarray(obj_png)
    G = np.zeros(obj_png.shape, np.uint8)
    classes = []
    for o in range(1, 255):
        under = cls_png[obj_png == o]
        best, best_count = 0, 0
        for c in range(1, num_cls + 1):
            k = int((under == c).sum())
            if k > best_count:
                best, best_count = c, k
        if best_count == 0:
            continue
        classes.append(best - 1)
        G[obj_png == o] = len(classes)
    return G, np.asarray(classes, np.int64)


def match_image(iou, score, cls, gt_cls, c, t):
    """[(score, is_tp), ...] of the image's predictions of class c at threshold t, in the per-image order."""
    preds = sorted((i for i in range(len(score)) if cls[i] == c), key=lambda i: (-float(score[i]), i))
    objs = [j for j in range(len(gt_cls)) if gt_cls[j] == c]
    taken = set()
    out = []
    for i in preds:
        hit = False
        if objs:
            j = objs[0]
            for k in objs[1:]:
                if iou[i, k] > iou[i, j]:
                    j = k
            if iou[i, j] >= t and j not in taken:
                taken.add(j)
                hit = True
        out.append((float(score[i]), hit))
    return out


def ap_from_matches(matches, n_pos):
    """matches: the pooled [(score, is_tp)] in order of arrival."""
    if n_pos == 0:
        return math.nan
    ranked = sorted(range(len(matches)), key=lambda k: (-matches[k][0], k))
    tp = fp = 0
    prec, rec = [0.0], [0.0]
    for k in ranked:
        if matches[k][1]:
            tp += 1
        else:
            fp += 1
        prec.append(tp / (tp + fp))
        rec.append(tp / n_pos)
    prec.append(0.0)
    rec.append(1.0)
    for k in range(len(prec) - 2, -1, -1):
        prec[k] = max(prec[k], prec[k + 1])
    return sum((rec[k] - rec[k - 1]) * prec[k] for k in range(1, len(rec)) if rec[k] != rec[k - 1])


def evaluate(images, num_cls, thresholds):
    """images: [(iou [n,m], score [n], cls [n], gt_cls [m]), ...] -> {'ap': [T, num_cls], 'map': [T]}."""
    ap = np.full((len(thresholds), num_cls), np.nan)
    for ti, t in enumerate(thresholds):
        for c in range(num_cls):
            pooled, n_pos = [], 0
            for iou, score, cls, gt_cls in images:
                pooled += match_image(iou, score, cls, gt_cls, c, t)
                n_pos += sum(1 for g in gt_cls if g == c)
            ap[ti, c] = ap_from_matches(pooled, n_pos)
    mean = np.array([np.nanmean(r) if not np.isnan(r).all() else np.nan for r in ap])
    return {"ap": ap, "map": mean}


# ---- synthetic inputs shared by the CPU and GPU tests -----------------------------------------------------------------------------
def blobs(H, W, count, seed):
    """A non-overlapping int32 label map [H,W] with values 0..count: `count` axis-aligned rectangles painted in turn over 0, so
    neighbouring pixels mostly share their value and a later rectangle may hide an earlier one."""
    rng = np.random.RandomState(seed)
    out = np.zeros((H, W), np.int32)
    for k in range(1, count + 1):
        y0, x0 = rng.randint(0, H), rng.randint(0, W)
        y1, x1 = rng.randint(y0, H) + 1, rng.randint(x0, W) + 1
        out[y0:y1, x0:x1] = k
    return out


def synthetic_image(H, W, n, m, seed, num_cls=20):
    """(seg_map int32 [H,W] with segments 1..n, score [n], cls [n], cls_png, obj_png): objects and segments are rectangles, the
    object PNG carries a void rim (255) and the class PNG the objects' classes."""
    rng = np.random.RandomState(seed)
    obj = blobs(H, W, m, seed + 1).astype(np.uint8)
    obj_cls = rng.randint(1, num_cls + 1, m + 1)
    cls_png = np.where(obj > 0, obj_cls[obj], 0).astype(np.uint8)
    obj[0, :] = 255
    cls_png[0, :] = 255
    seg = blobs(H, W, n, seed + 2)
    for j in range(1, min(n, m) + 1):                                       # some segments cover their object exactly
        if rng.rand() < 0.6:
            seg[obj == j] = j
    score = np.round(rng.rand(n), 1).astype(np.float32)                     # one decimal: ties occur
    cls = np.where(rng.rand(n) < 0.7, obj_cls[np.minimum(np.arange(1, n + 1), m)] - 1, rng.randint(0, num_cls, n)).astype(np.int64)
    return seg, score, cls, cls_png, obj
