"""numpy restatement of the self-training label rule (DESIGN.md "Self-training labels"; csrc/selflabel.hip): the scan argmax,
the confidence code through an np.float32 subtraction and .view(np.uint32), the three tables, the thresholds, the quality
curve and the selection.  Written from the rule, independent of muscle_amd/selflabel.py; loops where a loop is the rule."""
import math

import numpy as np

TOP = 193


def scan_argmax(prob):
    """prob fp32 [K,H,W] -> (label uint8 [H,W], conf fp32 [H,W]): best = prob[0]; a later channel wins only if strictly
    greater - so a NaN in channel 0 stays, a NaN elsewhere never wins."""
    prob = np.asarray(prob, dtype=np.float32)
    best = prob[0].copy()
    label = np.zeros(prob.shape[1:], dtype=np.uint8)
    for c in range(1, prob.shape[0]):
        with np.errstate(invalid="ignore"):
            win = prob[c] > best
        best[win] = prob[c][win]
        label[win] = c
    return label, best


def code(conf):
    conf = np.ascontiguousarray(conf, dtype=np.float32)
    out = np.zeros(conf.shape, dtype=np.uint8)
    flat, o = conf.reshape(-1), out.reshape(-1)
    for i in range(flat.size):
        c = flat[i]
        if np.isnan(c):
            o[i] = 255
            continue
        with np.errstate(invalid="ignore", over="ignore"):
            u = np.float32(1.0) - c                                       # one fp32 subtraction
        if u <= 0:
            o[i] = 0
            continue
        b = int(np.array([u], dtype=np.float32).view(np.uint32)[0]) >> 20  # sign, 8 exponent bits, top 3 mantissa bits
        o[i] = min(max(b - 823, 1), TOP)
    return out


def code_fast(conf):
    """`code` without the Python loop (the GPU tests' maps); test_cpu_selflabel.py pins it to `code`."""
    conf = np.ascontiguousarray(conf, dtype=np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        u = np.float32(1.0) - conf
    b = (u.view(np.uint32) >> np.uint32(20)).astype(np.int64) - 823
    out = np.clip(b, 1, TOP)
    out[~(u > 0)] = 0
    out[np.isnan(conf)] = 255
    return out.astype(np.uint8)


def tables(label, cd, gt, K):
    """hist / val / hit int64 [K,256]; gt None: val and hit stay zero.  A label >= K is counted nowhere."""
    hist, val, hit = (np.zeros((K, 256), dtype=np.int64) for _ in range(3))
    lab, cd = np.asarray(label).reshape(-1).astype(np.int64), np.asarray(cd).reshape(-1).astype(np.int64)
    ok = lab < K
    np.add.at(hist, (lab[ok], cd[ok]), 1)
    if gt is not None:
        g = np.asarray(gt).reshape(-1).astype(np.int64)
        v = ok & (g != 255)
        np.add.at(val, (lab[v], cd[v]), 1)
        h = ok & (g == lab)
        np.add.at(hit, (lab[h], cd[h]), 1)
    return hist, val, hit


def thresholds(hist, portion, min_conf=None):
    hist = np.asarray(hist, dtype=np.int64)
    K = hist.shape[0]
    por = [float(portion)] * K if np.ndim(portion) == 0 else [float(p) for p in portion]
    out = np.zeros(K, dtype=np.uint8)
    for c in range(K):
        n = int(hist[c].sum())
        if n == 0:
            continue
        need = min(n, max(1, math.ceil(por[c] * n)))
        run, t = 0, TOP
        for k in range(TOP + 1):
            run += int(hist[c, k])
            if run >= need:
                t = k
                break
        if min_conf is not None:
            t = min(t, int(code(np.float32(min_conf).reshape(1))[0]))
        out[c] = t
    return out


def select(label, cd, tcode):
    """(out uint8, kept int64 [K,2] = (kept, total))."""
    label, cd = np.asarray(label), np.asarray(cd)
    K = len(tcode)
    out = np.full(label.shape, 255, dtype=np.uint8)
    kept = np.zeros((K, 2), dtype=np.int64)
    for c in range(K):
        m = label == c
        k = m & (cd <= tcode[c])
        out[k] = c
        kept[c] = (k.sum(), m.sum())
    return out, kept


def curve_brute(label, cd, gt, K, portions):
    """Per portion, counted over the pixels: (kept [K], total [K], valid kept [K], confirmed kept [K])."""
    hist = tables(label, cd, None, K)[0]
    label, cd, gt = (np.asarray(a).reshape(-1) for a in (label, cd, gt))
    rows = []
    for p in portions:
        t = thresholds(hist, p)
        kept, total, kv, kh = (np.zeros(K, dtype=np.int64) for _ in range(4))
        for i in range(label.size):
            c = int(label[i])
            if c >= K:
                continue
            total[c] += 1
            if cd[i] <= t[c]:
                kept[c] += 1
                kv[c] += gt[i] != 255
                kh[c] += gt[i] == c
        rows.append((kept, total, kv, kh))
    return rows
