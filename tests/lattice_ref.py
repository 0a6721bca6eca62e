"""Numpy restatement of the permutohedral-lattice filter of muscle_amd.lattice (Adams, Baek & Davis 2010; the filter pydensecrf
evaluates the CRFs of src/imutils.py:439-456 and :477-491 on) and of the two CRFs on it, written from the definition.

Construction, per pixel with features f[0..D-1] (np.float32, this operation order, one rounding per operation):

    sf[i] = (D+1) sqrt(2/3) / sqrt((i+1)(i+2))                         double, rounded to float32 once
    sm = 0;  for j = D..1: cf = f[j-1]*sf[j-1]; el[j] = sm - j*cf; sm += cf;   el[0] = sm
    rd[i] = floor(el[i] * float32(1/(D+1)) + 0.5);  rem0[i] = rd[i]*(D+1);  sum = sum_i rd[i]
    rank: for i < j: rank[i]++ if el[i]-rem0[i] < el[j]-rem0[j] else rank[j]++
    sum > 0: rank >= D+1-sum -> rem0 -= D+1, rank += sum-(D+1); others rank += sum
    sum < 0: rank < -sum     -> rem0 += D+1, rank += D+1+sum;   others rank += sum
    b[0..D+1] = 0; for i = 0..D: v = (el[i]-rem0[i])/(D+1); b[D-rank[i]] += v; b[D+1-rank[i]] -= v;   b[0] += 1 + b[D+1]
    vertex r = 0..D: key[i] = rem0[i] + canon[r][rank[i]] (i < D), canon[r][k] = r if k <= D-r else r-(D+1); weight b[r]

Filter: splat val[vertex] += b[r]*in[pixel]; blur for j = 0..D in this order val' = val + 0.5*(val[n1_j] + val[n2_j]) (n1: key-1 in
every coordinate except key[j]+D, n2: key+1 except key[j]-D; absent neighbours count 0); slice out = alpha * sum_r b[r]*val[vertex_r],
alpha = 1/(1 + 2^-D).  The construction is float32 always; `dtype` switches the arithmetic of the filter and of the CRFs."""
import math

import numpy as np

import crf_ref as R
import ir_label_ref as IR


def scale_factors(D):
    return np.array([(D + 1) * math.sqrt(2.0 / 3.0) / math.sqrt((i + 1) * (i + 2)) for i in range(D)], dtype=np.float64).astype(np.float32)


def features(img_or_hw, sxy, srgb=None):
    """float32 [N,D]: (x/sxy, y/sxy) for an (H, W) pair or srgb None, else (x/sxy, y/sxy, r/srgb, g/srgb, b/srgb) of the uint8 image."""
    if isinstance(img_or_hw, tuple):
        H, W = img_or_hw
        img = None
    else:
        img = np.asarray(img_or_hw)
        H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    cols = [xx.ravel().astype(np.float32) / np.float32(sxy), yy.ravel().astype(np.float32) / np.float32(sxy)]
    if srgb is not None and srgb > 0:
        rgb = img.reshape(-1, 3).astype(np.float32)
        cols += [rgb[:, c] / np.float32(srgb) for c in range(3)]
    f = np.stack(cols, 1)
    assert f.dtype == np.float32
    return f


class Lattice:
    """vid int [N,D+1], w float32 [N,D+1], keys int [M,D] (sorted rows), n1 / n2 int [M,D+1] (-1: absent)."""

    def __init__(self, feats):
        f = np.ascontiguousarray(feats, dtype=np.float32)
        N, D = f.shape
        D1 = D + 1
        f32 = np.float32
        sf = scale_factors(D)
        el = np.zeros((N, D1), f32)
        sm = np.zeros(N, f32)
        for j in range(D, 0, -1):
            cf = f[:, j - 1] * sf[j - 1]
            el[:, j] = sm - f32(j) * cf
            sm = sm + cf
        el[:, 0] = sm
        rd = np.floor(el * f32(1.0 / D1) + f32(0.5))
        rem0 = rd * f32(D1)
        s = rd.astype(np.int64).sum(1)
        rank = np.zeros((N, D1), np.int64)
        diff = el - rem0
        for i in range(D1):
            for j in range(i + 1, D1):
                lt = diff[:, i] < diff[:, j]
                rank[:, i] += lt
                rank[:, j] += ~lt
        sc = s[:, None]
        up = (sc > 0) & (rank >= D1 - sc)
        dn = (sc < 0) & (rank < -sc)
        rem0 = np.where(up, rem0 - f32(D1), np.where(dn, rem0 + f32(D1), rem0)).astype(f32)
        rank = rank + sc + np.where(up, -D1, 0) + np.where(dn, D1, 0)
        assert rank.min() >= 0 and rank.max() <= D and (np.sort(rank, 1) == np.arange(D1)).all()
        b = np.zeros((N, D + 2), f32)
        rows = np.arange(N)
        for i in range(D1):
            v = (el[:, i] - rem0[:, i]) / f32(D1)
            b[rows, D - rank[:, i]] += v
            b[rows, D1 - rank[:, i]] -= v
        b[:, 0] += f32(1.0) + b[:, D1]
        assert b.dtype == f32
        canon = np.array([[r if k <= D - r else r - D1 for k in range(D1)] for r in range(D1)], np.int64)
        ri = rem0.astype(np.int64)
        key = ri[:, None, :D] + canon[:, rank[:, :D]].transpose(1, 0, 2)           # [N, r, i]
        keys, inv = np.unique(key.reshape(-1, D), axis=0, return_inverse=True)
        self.D, self.N, self.M = D, N, len(keys)
        self.vid = inv.reshape(N, D1)
        self.w = np.ascontiguousarray(b[:, :D1])
        self.keys = keys
        self.pixel_keys = key
        index = {tuple(k): n for n, k in enumerate(keys.tolist())}
        self.index = index
        n1 = np.full((self.M, D1), -1, np.int64)
        n2 = np.full((self.M, D1), -1, np.int64)
        for j in range(D1):
            k1, k2 = keys - 1, keys + 1
            if j < D:
                k1[:, j] = keys[:, j] + D
                k2[:, j] = keys[:, j] - D
            n1[:, j] = [index.get(tuple(k), -1) for k in k1.tolist()]
            n2[:, j] = [index.get(tuple(k), -1) for k in k2.tolist()]
        self.n1, self.n2 = n1, n2
        self.alpha = 1.0 / (1.0 + 2.0 ** (-D))

    def filter(self, x, dtype=np.float64):
        """x [N] or [N,C] -> the filtered values, same shape, in `dtype`."""
        x = np.asarray(x, dtype=dtype)
        flat = x.ndim == 1
        x2 = x[:, None] if flat else x
        D1 = self.D + 1
        w = self.w.astype(dtype)
        val = np.zeros((self.M, x2.shape[1]), dtype)
        for r in range(D1):
            np.add.at(val, self.vid[:, r], w[:, r, None] * x2)
        zero = np.zeros((1, x2.shape[1]), dtype)
        for j in range(D1):
            ext = np.concatenate([val, zero], 0)                                     # index -1: the absent neighbour
            val = val + dtype(0.5) * (ext[self.n1[:, j]] + ext[self.n2[:, j]])
        out = np.zeros_like(x2)
        for r in range(D1):
            out = out + w[:, r, None] * val[self.vid[:, r]]
        out = dtype(self.alpha) * out
        assert out.dtype == dtype
        return out[:, 0] if flat else out


def lattices(img, sxy_g, sxy_b, srgb):
    """(spatial D = 2, bilateral D = 5) lattices of the uint8 image img [H,W,3]."""
    return Lattice(features(tuple(img.shape[:2]), sxy_g)), Lattice(features(img, sxy_b, srgb))


def _mean_field(U, lats, ws, t, dtype):
    """U [G,L,N] -> Q_t [G,L,N]; the problems are iterated as columns of one matrix."""
    G, L, N = U.shape
    Q = np.stack([R.softmax0(-u) for u in U])
    if t > 0:
        one = np.ones(N, dtype)
        ns = [dtype(1.0) / np.sqrt(lat.filter(one, dtype) + dtype(1e-20)) for lat in lats]
        for _ in range(t):
            B = Q.reshape(G * L, N).T
            x = -U.reshape(G * L, N)
            for lat, n, w in zip(lats, ns, ws):
                x = x + dtype(w) * (n[:, None] * lat.filter(np.ascontiguousarray(n[:, None] * B), dtype)).T
            Q = np.stack([R.softmax0(xg) for xg in x.reshape(G, L, N)])
    assert Q.dtype == dtype
    return Q


def crf_lattice_ref(img, probs, t, scale_factor=1.5, confidence=0.5, dtype=np.float64, lats=None):
    """crf_inference(pairwise="lattice"): Q_t [L,H,W] in `dtype`."""
    L, H, W = probs.shape
    lats = lats or lattices(img, R.GAUSS_SXY / scale_factor, R.BILATERAL_SXY / scale_factor, R.BILATERAL_SRGB)
    U = R.unary(probs, confidence, dtype).reshape(1, L, -1)
    return _mean_field(U, lats, (R.GAUSS_W, R.BILATERAL_W), t, dtype).reshape(L, H, W)


def crf_labels_lattice_ref(img, labs, L, t=IR.T, gt_prob=IR.GT_PROB, dtype=np.float64, lats=None):
    """Q_t [G,L,H,W] of the label CRFs of labs [G,H,W] on one image."""
    labs = np.asarray(labs)
    G, H, W = labs.shape
    lats = lats or lattices(img, IR.GAUSS_SXY, IR.BILATERAL_SXY, IR.BILATERAL_SRGB)
    U = np.stack([IR.unary_from_labels(lab, L, gt_prob, dtype) for lab in labs]).reshape(G, L, -1)
    return _mean_field(U, lats, (IR.GAUSS_W, IR.BILATERAL_W), t, dtype).reshape(G, L, H, W)


def ir_label_lattice_ref(img, cams, keys, t=IR.T, gt_prob=IR.GT_PROB, fg_thres=IR.FG_THRES, bg_thres=IR.BG_THRES, dtype=np.float64,
                         lats=None):
    """{"labs" [2,H,W], "q" Q_t [2,L,H,W], "pred" [2,H,W], "conf" uint8 [H,W]} of ir_label_run(pairwise="lattice")."""
    keys = np.asarray(keys)
    labs = IR.label_maps(cams, fg_thres, bg_thres)
    q = crf_labels_lattice_ref(img, labs, len(keys), t, gt_prob, dtype, lats)
    pred = q.argmax(1)
    return {"labs": labs, "q": q, "pred": pred, "conf": IR.combine_conf(keys[pred[0]], keys[pred[1]])}
