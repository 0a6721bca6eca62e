"""Numpy restatement of IR-label generation (muscle_amd.ir_label; IRN's cam_to_ir_label around src/imutils.py:477-491), written
from its definition.  With cams float32 [C,H,W], L = C + 1 and keys = [0, k_1+1, ..., k_C+1]:

    fg_lab = argmax([fg_thres, cams...], axis 0)   bg_lab = argmax([bg_thres, cams...], axis 0)       first maximum wins;
                                                                          the thresholds are float32 values, as the ABI takes them
    U[l,i]   = -log(gt_prob) if l == lab(i) else -log((1 - gt_prob) / (L - 1))                 unary_from_labels(zero_unsure=False)
    k_m, n_m, the window R_m = ceil(trunc * sxy_m) and the update as in crf_ref.py, with
               sxy_g = 3 (weight 3), sxy_b = 50, srgb = 5 (weight 10), t = 10, gt_prob = 0.7
    pred_g   = argmax_l Q_t                                                                     first maximum wins
    conf     = keys[pred_fg];  conf[keys[pred_fg] == 0] = 255;  conf[keys[pred_bg] + keys[pred_fg] == 0] = 0

`dtype` switches the whole arithmetic of the CRF (np.float64 is the reference; np.float32 measures what fp32 rounding alone does
to the same model).  The two problems of an image share the kernel matrices; they are iterated as columns of one matrix."""
import numpy as np

import crf_ref as R

GAUSS_SXY, GAUSS_W = 3.0, 3.0
BILATERAL_SXY, BILATERAL_SRGB, BILATERAL_W = 50.0, 5.0, 10.0
T, GT_PROB = 10, 0.7
FG_THRES, BG_THRES = 0.30, 0.05

# the cases of tests/golden/ir_label.npz and tests/test_gpu_ir_label.py: name -> (seed, H, W, C, trunc, noise sigma)
CASES = {
    "a_40x56": (11, 40, 56, 3, 4.0, 12.0),        # the window covers the image: all pairs
    "b_48x72": (12, 48, 72, 3, 0.5, 8.0),         # R_b = 25, R_g = 2: the window is cut inside the image
    "c_37x53": (13, 37, 53, 1, 4.0, 4.0),         # ragged size; L = 2, the smallest
    "d_24x40": (14, 24, 40, 15, 4.0, 12.0),       # L = 16, the fused limit: 32 columns
    "e_24x40": (15, 24, 40, 16, 4.0, 12.0),       # L = 17: one problem per pass
    "f_9x45": (16, 9, 45, 2, 4.0, 6.0),           # extreme aspect ratios
    "f_70x5": (17, 70, 5, 2, 4.0, 10.0),
}


def synthetic(seed, H, W, C, sigma=12.0):
    """Three colour regions with noise (the construction of crf_ref.standard_input) and C CAMs: smooth blobs normalised to a
    maximum of 1 per class, rounded to float16 values (exact in float32; the fixture stores them as float16).  Returns
    (img uint8 [H,W,3], cams float32 [C,H,W], keys int [C+1])."""
    g = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    img[:, :W // 3] = [200, 30, 30]
    img[H // 4:3 * H // 4, W // 3:4 * W // 5] = [20, 180, 60]
    img[:, 4 * W // 5:] = [30, 40, 200]
    img = np.clip(img + g.normal(0, sigma, img.shape), 0, 255).astype(np.uint8)
    yy, xx = np.mgrid[0:H, 0:W]
    cams = np.empty((C, H, W))
    for c in range(C):
        cx, cy = g.uniform(0.1, 0.9) * W, g.uniform(0.1, 0.9) * H
        sx, sy = g.uniform(0.12, 0.25) * max(W, 8), g.uniform(0.12, 0.25) * max(H, 8)
        cams[c] = np.exp(-0.5 * (((xx - cx) / sx) ** 2 + ((yy - cy) / sy) ** 2)) + 0.03 * g.random((H, W))
        cams[c] /= cams[c].max()
    cams = cams.astype(np.float16).astype(np.float32)
    classes = np.sort(g.choice(20, C, replace=False))
    keys = np.concatenate([[0], classes + 1]).astype(np.int64)
    return img, cams, keys


def case(name):
    """(img, cams, keys, trunc) of a named case."""
    seed, H, W, C, trunc, sigma = CASES[name]
    return synthetic(seed, H, W, C, sigma) + (trunc,)


def label_maps(cams, fg_thres=FG_THRES, bg_thres=BG_THRES):
    """The two thresholded argmax maps [2,H,W] (0 = the threshold won), compared in float32."""
    cams = np.asarray(cams, dtype=np.float32)
    out = []
    for thres in (fg_thres, bg_thres):
        stack = np.concatenate([np.full((1,) + cams.shape[1:], np.float32(thres), np.float32), cams], 0)
        out.append(stack.argmax(0))
    return np.stack(out)


def unary_from_labels(labels, L, gt_prob=GT_PROB, dtype=np.float64):
    """pydensecrf.utils.unary_from_labels(labels, L, gt_prob, zero_unsure=False): U [L,H,W]."""
    labels = np.asarray(labels)
    own = -np.log(dtype(gt_prob))
    oth = -np.log((dtype(1.0) - dtype(gt_prob)) / dtype(L - 1))
    U = np.full((L,) + labels.shape, oth, dtype=dtype)
    for l in range(L):
        U[l][labels == l] = own
    return U


def one_hot_confidence(L, gt_prob=GT_PROB):
    """The `confidence` at which crf_ref.unary of a one-hot map is the label unary: c + (1 - c) / L = gt_prob."""
    return (gt_prob - 1.0 / L) / (1.0 - 1.0 / L)


def kernels(img, trunc=4.0, dtype=np.float64):
    """(gauss, bilateral) crf_ref.Kernel objects of this model for the uint8 image img [H,W,3]."""
    H, W = img.shape[:2]
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int64)
    pos = xy.astype(dtype)
    rgb = img.reshape(-1, 3).astype(dtype)
    fg = pos / dtype(GAUSS_SXY)
    fb = np.concatenate([pos / dtype(BILATERAL_SXY), rgb / dtype(BILATERAL_SRGB)], 1)
    return R.Kernel(fg, xy, R.radius(trunc, GAUSS_SXY), dtype), R.Kernel(fb, xy, R.radius(trunc, BILATERAL_SXY), dtype)


def crf_labels(img, labs, L, t=T, gt_prob=GT_PROB, trunc=4.0, dtype=np.float64):
    """Q_t [G,L,H,W] in `dtype` of the label CRFs of labs [G,H,W] on one image."""
    labs = np.asarray(labs)
    G, H, W = labs.shape
    U = np.stack([unary_from_labels(lab, L, gt_prob, dtype) for lab in labs]).reshape(G, L, -1)
    Q = np.stack([R.softmax0(-u) for u in U])
    if t > 0:
        ks = kernels(img, trunc, dtype)
        one = np.ones(H * W, dtype=dtype)
        ns = [dtype(1.0) / np.sqrt(k.apply(one) + dtype(1e-20)) for k in ks]
        ws = (dtype(GAUSS_W), dtype(BILATERAL_W))
        for _ in range(t):
            B = Q.reshape(G * L, -1).T                          # the problems as columns of one matrix
            x = -U.reshape(G * L, -1)
            for k, n, w in zip(ks, ns, ws):
                x = x + w * (n[:, None] * k.apply(np.ascontiguousarray(n[:, None] * B))).T
            Q = np.stack([R.softmax0(xg) for xg in x.reshape(G, L, -1)])
    assert Q.dtype == dtype
    return Q.reshape(G, L, H, W)


def combine_conf(fg_conf, bg_conf):
    conf = np.array(fg_conf, dtype=np.int64)
    conf[np.asarray(fg_conf) == 0] = 255
    conf[np.asarray(bg_conf, dtype=np.int64) + np.asarray(fg_conf, dtype=np.int64) == 0] = 0
    return conf.astype(np.uint8)


def ir_label(img, cams, keys, t=T, gt_prob=GT_PROB, trunc=4.0, fg_thres=FG_THRES, bg_thres=BG_THRES, dtype=np.float64):
    """{"labs" [2,H,W], "q" Q_t [2,L,H,W], "pred" [2,H,W], "conf" uint8 [H,W]}"""
    keys = np.asarray(keys)
    labs = label_maps(cams, fg_thres, bg_thres)
    q = crf_labels(img, labs, len(keys), t, gt_prob, trunc, dtype)
    pred = q.argmax(1)
    return {"labs": labs, "q": q, "pred": pred, "conf": combine_conf(keys[pred[0]], keys[pred[1]])}


def top2_gap(q):
    """Top-two gap of Q [..., L, H, W] over the label axis."""
    s = np.sort(q, -3)
    return s[..., -1, :, :] - s[..., -2, :, :]
