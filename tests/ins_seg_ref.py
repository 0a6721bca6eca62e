"""The instance pseudo-label algorithm ("Instance pseudo-labels", steps 1-6) restated in numpy: the yardstick of
muscle_amd/ins_seg.py.  Written from the specification; imports nothing from muscle_amd.  Also the synthetic displacement fields
and label patterns the CPU and GPU tests share."""
import numpy as np

F = np.float32


# ---- step 1 ---------------------------------------------------------------------------------------------------------------
def find_centroids(dp, iterations=300, products64=False):
    """dp float32 [2,h,w] -> int32 [2,h,w].  Every product and sum is one fp32 operation, left to right (numpy evaluates
    a*b*c + ... exactly so on float32 arrays).  products64: the four tap terms formed in fp64 and rounded once - the variant that
    shows how little it takes to move a centroid."""
    dp = np.asarray(dp, F)
    _, h, w = dp.shape
    cy, cx = np.mgrid[0:h, 0:w].astype(F)
    one = F(1)
    for _ in range(int(iterations)):
        uy, dy = np.ceil(cy), np.floor(cy)
        ux, dx = np.ceil(cx), np.floor(cx)
        yc, xc = cy - dy, cx - dx
        iuy, idy, iux, idx = uy.astype(np.int64), dy.astype(np.int64), ux.astype(np.int64), dx.astype(np.int64)

        def m(d):
            if products64:
                t = [d[iuy, iux].astype(np.float64) * yc * xc, d[idy, iux].astype(np.float64) * (one - yc) * xc,
                     d[iuy, idx].astype(np.float64) * yc * (one - xc), d[idy, idx].astype(np.float64) * (one - yc) * (one - xc)]
                t = [v.astype(F) for v in t]
                return t[0] + t[1] + t[2] + t[3]
            return d[iuy, iux] * yc * xc + d[idy, iux] * (one - yc) * xc + d[iuy, idx] * yc * (one - xc) + d[idy, idx] * (one - yc) * (one - xc)

        my, mx = m(dp[0]), m(dp[1])
        assert my.dtype == F and mx.dtype == F
        cy = np.clip(cy + my, F(0), F(h - 1))
        cx = np.clip(cx + mx, F(0), F(w - 1))
    return np.stack([np.rint(cy), np.rint(cx)]).astype(np.int32)                 # np.rint: half to even


# ---- components (steps 2 and 6) ---------------------------------------------------------------------------------------------
def label_components(lab):
    """int [h,w] -> int32 [h,w]: the linear index of the first raster pixel of the 4-connected component of equal non-zero
    labels the pixel lies in, -1 where lab is 0.  A flood fill started from every unvisited pixel in raster order."""
    lab = np.asarray(lab)
    h, w = lab.shape
    a = lab.ravel().tolist()
    root = [-1] * (h * w)
    for s in range(h * w):
        if a[s] == 0 or root[s] >= 0:
            continue
        L = a[s]
        root[s] = s
        stack = [s]
        while stack:
            p = stack.pop()
            y, x = divmod(p, w)
            if x > 0 and root[p - 1] < 0 and a[p - 1] == L:
                root[p - 1] = s
                stack.append(p - 1)
            if x < w - 1 and root[p + 1] < 0 and a[p + 1] == L:
                root[p + 1] = s
                stack.append(p + 1)
            if y > 0 and root[p - w] < 0 and a[p - w] == L:
                root[p - w] = s
                stack.append(p - w)
            if y < h - 1 and root[p + w] < 0 and a[p + w] == L:
                root[p + w] = s
                stack.append(p + w)
    return np.asarray(root, np.int32).reshape(h, w)


# ---- step 2 ---------------------------------------------------------------------------------------------------------------
def weak_map(dp, thres=2.5):
    dp = np.asarray(dp, F)
    return np.sqrt(dp[1] ** 2 + dp[0] ** 2) < F(thres)


def cluster_centroids(cent, dp, thres=2.5):
    """(cluster int32 [h,w], I): the weak component at every pixel's centroid, ids compressed ascending, background first."""
    root = label_components(weak_map(dp, thres).astype(np.int32))
    ids = root[cent[0], cent[1]]
    uniq, inv = np.unique(ids, return_inverse=True)                               # ascending; -1 (background) sorts first
    return inv.reshape(ids.shape).astype(np.int32), int(len(uniq))


# ---- step 3 ---------------------------------------------------------------------------------------------------------------
def split_instances(cam, cluster, I):
    """cam [K,h,w], cluster [h,w] -> [K*I,h,w] class-major."""
    K = cam.shape[0]
    onehot = (cluster[None] == np.arange(I)[:, None, None])
    return (cam[:, None].astype(F) * onehot[None].astype(F)).reshape(K * I, *cluster.shape)


# ---- step 5 ---------------------------------------------------------------------------------------------------------------
def upsample4(rw, H, W):
    """rw float32 [C,h,w] -> [C,H,W]: 4x half-pixel bilinear (align_corners=False), top-left crop, fp32."""
    rw = np.asarray(rw, F)
    _, h, w = rw.shape

    def taps(n_out, n_in):
        s = np.maximum((np.arange(n_out, dtype=F) + F(0.5)) * F(0.25) - F(0.5), F(0))
        i0 = np.minimum(s.astype(np.int64), n_in - 1)
        i1 = np.minimum(i0 + 1, n_in - 1)
        return i0, i1, (s - i0.astype(F)).astype(F)

    y0, y1, wy = taps(H, h)
    x0, x1, wx = taps(W, w)
    wy, wx = wy[None, :, None], wx[None, None, :]
    one = F(1)
    r0 = (one - wx) * rw[:, y0][:, :, x0] + wx * rw[:, y0][:, :, x1]
    r1 = (one - wx) * rw[:, y1][:, :, x0] + wx * rw[:, y1][:, :, x1]
    return ((one - wy) * r0 + wy * r1).astype(F)


def finish(rw, H, W, bg_thres=0.25):
    """(label int32 [H,W], win float32 [H,W], vmax, margin float32 [H,W]): margin = the winner's lead over the runner-up among
    [bg_thres, channels], in units of the normalised values."""
    up = upsample4(rw, H, W)
    vmax = up.max()
    full = np.concatenate([np.full((1, H, W), bg_thres, F), up / vmax if vmax > 0 else np.zeros_like(up)], 0)
    label = np.argmax(full, 0).astype(np.int32)                                  # first maximum wins
    srt = np.sort(full, 0)
    return label, srt[-1], vmax, srt[-1] - srt[-2]


# ---- step 6 ---------------------------------------------------------------------------------------------------------------
def segments(label, win, keys, I):
    """label int32 [H,W], win float32 [H,W] -> dict(seg_map int32 [H,W], score f32 [n], cls int64 [n], area int32 [n])."""
    label = np.asarray(label)
    H, W = label.shape
    root = label_components(label)
    firsts = np.unique(root[root >= 0])
    order = sorted(firsts.tolist(), key=lambda r: (int(label.ravel()[r]), r))
    seg_map = np.zeros((H, W), np.int32)
    score, cls, area = [], [], []
    for s, r in enumerate(order):
        m = root == r
        a = int(m.sum())
        seg_map[m] = s + 1
        area.append(a)
        cls.append(keys[(int(label.ravel()[r]) - 1) // I])
        score.append(F(0) if np.float64(a) < H * W * 0.01 else win[m].max())
    return dict(seg_map=seg_map, score=np.asarray(score, F).reshape(-1), cls=np.asarray(cls, np.int64).reshape(-1),
                area=np.asarray(area, np.int32).reshape(-1))


# ---- the shared test fields -------------------------------------------------------------------------------------------------
def attractors(h, w, seed, swirl=False, outward=False):
    """dp = 0.5 * (nearest centre - p), capped at magnitude 6, plus N(0, 0.3) noise.  swirl: columns >= 2w/3 hold a unit
    tangential field x 3.5 around the centre of that block (two centres lie inside it, so the pixels to its left are pushed
    in and orbit: that part of the iteration is chaotic and ends on non-weak pixels).  outward: the border pixels are pushed out
    of the image."""
    g = np.random.default_rng(seed)
    centres = np.array([[0.25 * h, 0.2 * w], [0.7 * h, 0.3 * w], [0.3 * h, 0.85 * w], [0.75 * h, 0.85 * w]])
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    d = centres[:, :, None, None] - np.stack([yy, xx])[None]                      # [n,2,h,w]
    near = np.argmin((d ** 2).sum(1), 0)
    v = 0.5 * np.take_along_axis(d, near[None, None], 0)[0]
    mag = np.sqrt((v ** 2).sum(0))
    v = v * np.minimum(1.0, 6.0 / np.maximum(mag, 1e-12))
    v = v + g.normal(0.0, 0.3, v.shape)
    if swirl:
        c0 = (2 * w + 2) // 3
        if c0 < w:
            by, bx = (h - 1) / 2.0, (c0 + w - 1) / 2.0
            ry, rx = yy[:, c0:] - by, xx[:, c0:] - bx
            r = np.maximum(np.sqrt(ry ** 2 + rx ** 2), 1e-12)
            v[0][:, c0:], v[1][:, c0:] = 3.5 * rx / r, -3.5 * ry / r
    if outward:
        v[0][0, :], v[0][-1, :] = -3.0, 3.0
        v[1][:, 0], v[1][:, -1] = -3.0, 3.0
    return v.astype(F)


def walk_maps(C, h, w, seed):
    """float32 [C,h,w] stand-ins for a walk result: uniform(0,1)^2."""
    return (np.random.default_rng(seed).random((C, h, w)) ** 2).astype(F)


# the 300-channel finish case (more channels than a uint8 label holds): the seed is chosen so that at most 1 % of the pixels have a
# top-two margin below 1e-6 in the restatement itself (tests/test_cpu_ins_seg.py asserts it)
CASE4 = dict(C=300, h=6, w=7, H=23, W=27, seed=3, bg=0.25)


def pattern(name, h, w, seed=0):
    """int32 [h,w] label maps for the component tests."""
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    if name == "noise":                                         # Bernoulli(0.6): near site percolation, long winding components
        a = g.random((h, w)) < 0.6
    elif name == "spiral":                                      # a one-pixel path that winds inwards: the minimum index is far away
        a = np.zeros((h, w), bool)
        y, x, dy, dx, turns = 0, 0, 0, 1, 0
        a[0, 0] = True
        while turns < 2:                                        # walk on until the path would touch itself, then turn right
            ny, nx, ny2, nx2 = y + dy, x + dx, y + 2 * dy, x + 2 * dx
            if 0 <= ny < h and 0 <= nx < w and not a[ny, nx] and not (0 <= ny2 < h and 0 <= nx2 < w and a[ny2, nx2]):
                y, x, turns = ny, nx, 0
                a[y, x] = True
            else:
                dy, dx, turns = dx, -dy, turns + 1
    elif name == "comb":
        a = (xx % 2 == 0) | (yy == h - 1)
    elif name == "checker":
        a = (yy + xx) % 2 == 0
    elif name == "ones":
        a = np.ones((h, w), bool)
    elif name == "zeros":
        a = np.zeros((h, w), bool)
    elif name == "three":                                       # a 3-label random map: equal neighbours join, different ones do not
        return g.integers(0, 4, (h, w)).astype(np.int32)
    else:
        raise KeyError(name)
    return a.astype(np.int32)


PATTERNS = ("noise", "spiral", "comb", "checker", "ones", "zeros", "three")


def renumber_by_first_pixel(lab):
    """Any component labelling (0 = background) -> 1, 2, ... in the order of each component's first raster pixel."""
    flat = np.asarray(lab).ravel()
    uniq, first = np.unique(flat, return_index=True)
    keep = uniq != 0
    uniq, first = uniq[keep], first[keep]
    new = np.zeros(len(uniq), np.int64)
    new[np.argsort(first)] = np.arange(1, len(uniq) + 1)
    out = np.zeros(flat.shape, np.int64)
    nz = flat != 0
    out[nz] = new[np.searchsorted(uniq, flat[nz])]
    return out.reshape(np.shape(lab))
