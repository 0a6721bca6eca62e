"""Numpy restatement of the Lovasz-softmax model that include/muscle_hip.h states (mx_lovasz_ws ..), with a dtype switch: in
float32 mode EVERY floating-point step runs in float32 (softmax, errors, increments, sums, gradient).  `order_from` (fp32 errors
[S,P]) makes either evaluation take the stable order from those given errors instead of its own, so that a float32 and a float64
evaluation (or a kernel and a restatement) of near-tied inputs weight the same elements with the same increments.

Layout as the header: S = groups * K segments of P elements; per_image: groups = N, P = H*W, else one group of N*H*W pixels in
(n, hw) order."""
import numpy as np

IGNORE = 255


def softmax(x, dtype):
    x = x.astype(dtype)
    ex = np.exp(x - x.max(1, keepdims=True))
    assert ex.dtype == dtype
    return ex / ex.sum(1, keepdims=True, dtype=dtype)


def segment(e, fg, valid, dtype, order_e=None):
    """One segment: e [P] (dtype), fg / valid bool [P].  Returns rank int64 [P] (-1 ignored), g dtype [P] (original order), L, G, V."""
    P = e.shape[0]
    vi = np.flatnonzero(valid)
    V = int(vi.size)
    fg = fg & valid
    G = int(fg.sum())
    rank = np.full(P, -1, np.int64)
    g = np.zeros(P, dtype)
    if V == 0:
        return rank, g, dtype(0), G, V
    key = e if order_e is None else order_e
    order = vi[np.argsort(-key[vi], kind="stable")]
    rank[order] = np.arange(V)
    fgs = fg[order]
    i = np.arange(1, V + 1, dtype=np.int64)
    F = np.cumsum(fgs.astype(np.int64))
    I, U = G - F, G + i - F
    if G == 0:
        gs = np.zeros(V, dtype)
        gs[0] = 1
    else:
        Uf, If = U.astype(dtype), I.astype(dtype)
        with np.errstate(divide="ignore", invalid="ignore"):
            gs = np.where(fgs, dtype(1) / Uf, If / (Uf * (Uf - dtype(1)))).astype(dtype)
    g[order] = gs
    L = np.sum(e[order].astype(dtype) * gs, dtype=dtype)
    return rank, g, L, G, V


def core(err, flag, dtype=np.float64):
    """mx_lovasz_core on given fp32 errors [S,P] and flags uint8 [S,P] (bit 0 foreground, bit 1 valid)."""
    S, P = err.shape
    out = dict(rank=np.empty((S, P), np.int64), g=np.empty((S, P), dtype), seg_loss=np.empty(S, dtype), counts=np.empty((S, 2), np.int64))
    for s in range(S):
        valid = (flag[s] & 2) != 0
        r, g, L, G, V = segment(err[s].astype(dtype), (flag[s] & 1) != 0, valid, dtype, order_e=err[s])
        out["rank"][s], out["g"][s], out["seg_loss"][s], out["counts"][s] = r, g, L, (G, V)
    return out


def lovasz(seg, label, classes="present", per_image=False, dtype=np.float64, order_from=None, gup=1.0):
    """The whole model.  seg [N,K,H,W], label uint8 [N,H,W].  Returns loss, gseg [N,K,H,W] (times gup), err / flag / rank / g [S,P],
    seg_loss [S], counts [S,2], all floating-point values in dtype."""
    assert classes in ("present", "all")
    N, K, H, W = seg.shape
    HW = H * W
    p = softmax(seg.reshape(N, K, HW), dtype)
    lab = label.reshape(N, HW).astype(np.int64)
    valid = (lab != IGNORE) & (lab < K)
    groups, P = (N, HW) if per_image else (1, N * HW)
    pg = p if per_image else p.transpose(1, 0, 2).reshape(1, K, P)
    labg, vg = lab.reshape(groups, P), valid.reshape(groups, P)
    S = groups * K
    err, flag = np.zeros((S, P), dtype), np.zeros((S, P), np.uint8)
    rank, g = np.empty((S, P), np.int64), np.empty((S, P), dtype)
    seg_loss, counts = np.empty(S, dtype), np.empty((S, 2), np.int64)
    coef = np.zeros((groups, K, P), dtype)
    loss = dtype(0)
    for grp in range(groups):
        v = vg[grp]
        on = []
        for c in range(K):
            s = grp * K + c
            fg = (labg[grp] == c) & v
            e = np.where(v, np.abs(fg.astype(dtype) - pg[grp, c]), dtype(0)).astype(dtype)
            err[s], flag[s] = e, 2 * v + fg
            rank[s], g[s], seg_loss[s], G, V = segment(e, fg, v, dtype, None if order_from is None else order_from[s])
            counts[s] = (G, V)
            if V > 0 and (classes == "all" or G > 0):
                on.append(c)
        if not on:
            continue
        w = dtype(1) / (dtype(groups) * dtype(len(on)))
        for c in on:
            s = grp * K + c
            fg = (labg[grp] == c) & v
            sgn = np.where(fg, -(pg[grp, c] < 1).astype(dtype), (pg[grp, c] > 0).astype(dtype)) * v
            coef[grp, c] = (w * sgn.astype(dtype) * g[s]).astype(dtype)
            loss = dtype(loss + w * seg_loss[s])
    cn = coef if per_image else coef.reshape(K, N, HW).transpose(1, 0, 2)                     # [N,K,HW]
    dot = np.sum(cn * p, axis=1, keepdims=True, dtype=dtype)
    gseg = (dtype(gup) * p * (cn - dot) * valid[:, None]).astype(dtype)
    assert gseg.dtype == dtype and err.dtype == dtype
    return dict(loss=loss, gseg=gseg.reshape(N, K, H, W), err=err, flag=flag, rank=rank, g=g, seg_loss=seg_loss, counts=counts, p=p)


def order_margin(r):
    """Of a float64 evaluation: the smallest (gap - (d_i + d_j)) over neighbours in sorted order of every segment, d = 2^-18 for a
    foreground element and 2^-18 * e for a background one - positive: fp32 rounding cannot reorder anything."""
    worst = np.inf
    for s in range(r["err"].shape[0]):
        vi = np.flatnonzero(r["rank"][s] >= 0)
        if vi.size < 2:
            continue
        o = vi[np.argsort(r["rank"][s][vi])]
        e, fg = r["err"][s][o], (r["flag"][s][o] & 1) != 0
        d = np.where(fg, 2.0 ** -18, 2.0 ** -18 * e)
        worst = min(worst, float(np.min((e[:-1] - e[1:]) - (d[:-1] + d[1:]))))
    return worst


def make_case(N, K, H, W, seed, ignored=0.15, absent=(), flipped=0.2):
    """Blocky logits N(0, 2.5) + 3 * onehot(block class), labels = the block classes with a share flipped to a random class and a
    share ignored (255); classes in `absent` never occur as a label."""
    g = np.random.default_rng(seed)
    blocks = g.integers(0, K, (N, (H + 3) // 4, (W + 4) // 5)).repeat(4, 1).repeat(5, 2)[:, :H, :W]
    seg = (g.normal(0, 2.5, (N, K, H, W)) + 3.0 * (blocks[:, None] == np.arange(K)[None, :, None, None])).astype(np.float32)
    lab = np.where(g.random((N, H, W)) < flipped, g.integers(0, K, (N, H, W)), blocks)
    keep = [c for c in range(K) if c not in absent]
    for c in absent:
        lab[lab == c] = keep[c % len(keep)]
    lab = np.where(g.random((N, H, W)) < ignored, IGNORE, lab).astype(np.uint8)
    return seg, lab
