"""numpy restatement of the matrix-free IRN random walk (muscle_amd/csrc/irn_walk.hip), operation for operation: fp32 weights
by repeated multiplication, fp64 column sums, fp64 state, and the kernels' summation order (per pixel: the centre, then for
every one-sided direction d in path-table order the forward tap j+d, then the mirrored tap j-d; one rounded product and one
rounded addition per tap, no fused multiply-add).  The CPU yardstick the GPU test prints next to the kernel's result;
tests/test_cpu_irn_walk.py pins it against the reference's fixture and the dense fp64 oracle.
"""
import numpy as np


def directions(radius=5):
    """[(path, (dy, dx))] in the order of muscle_amd.indexing.search_paths: path = (dy, dx) offsets, the destination first."""
    from muscle_amd.indexing import search_paths
    return [(p, p[0]) for p in search_paths(radius)]


def power_f32(v, beta):
    """v ** beta in fp32 as irn_pow_colsum_kernel forms it: square-and-multiply for an integral beta in 1..64, else powf with 0 -> 0."""
    v = np.asarray(v, np.float32)
    if 0 < beta <= 64 and float(beta) == int(beta):
        r, b, e = np.ones_like(v), v.copy(), int(beta)
        while e:
            if e & 1:
                r = (r * b).astype(np.float32)
            b = (b * b).astype(np.float32)
            e >>= 1
        return r
    return np.where(v == 0, np.float32(0), np.power(v, np.float32(beta))).astype(np.float32)


def _shift(h, w, dy, dx):
    """Slices (dst, src) with dst = the pixels p whose p + (dy, dx) lies inside an h x w image, src = those p + (dy, dx)."""
    y0, y1 = max(0, -dy), min(h, h - dy)
    x0, x1 = max(0, -dx), min(w, w - dx)
    if y0 >= y1 or x0 >= x1:
        return None
    return (slice(y0, y1), slice(x0, x1)), (slice(y0 + dy, y1 + dy), slice(x0 + dx, x1 + dx))


def walk_weights(edge, radius=5, beta=10):
    """edge [h,w] -> (W fp32 [nd,h,w], cs fp64 [h,w]).  W[d][p] = (1 - max of the edge along the path p -> p+d)^beta, 0 where
    p+d is outside; cs[j] = 1 + sum_d (W[d][j] + W[d][j-d]) in that order, fp64."""
    edge = np.asarray(edge, np.float32)
    h, w = edge.shape
    dirs = directions(radius)
    W = np.zeros((len(dirs), h, w), np.float32)
    for d, (path, (dy, dx)) in enumerate(dirs):
        s = _shift(h, w, dy, dx)
        if s is None:
            continue
        dst, _ = s
        mx = np.full((dst[0].stop - dst[0].start, dst[1].stop - dst[1].start), -np.inf, np.float32)
        for py, px in path:                                    # every path point is inside the box of p and p+d
            mx = np.maximum(mx, edge[dst[0].start + py:dst[0].stop + py, dst[1].start + px:dst[1].stop + px])
        W[d][dst] = power_f32(np.float32(1) - mx, beta)
    cs = np.ones((h, w), np.float64)
    for d, (_path, (dy, dx)) in enumerate(dirs):
        cs += W[d].astype(np.float64)
        s = _shift(h, w, -dy, -dx)
        if s is not None:
            cs[s[0]] += W[d][s[1]].astype(np.float64)
    return W, cs


def walk(x, edge, radius=5, beta=10, exp_times=8, state_dtype=np.float64):
    """x [C,h,w] (or anything reshaping to it), edge [h,w] or [1,h,w] -> rw fp32 [C,1,h,w] after 2^exp_times stencil steps."""
    edge = np.asarray(edge, np.float32).reshape(edge.shape[-2:])
    h, w = edge.shape
    x = np.asarray(x, np.float32).reshape(-1, h, w)
    W, cs = walk_weights(edge, radius, beta)
    dirs = directions(radius)
    taps = [(_shift(h, w, dy, dx), _shift(h, w, -dy, -dx)) for _p, (dy, dx) in dirs]
    Wd = W.astype(state_dtype)
    v = (x * (np.float32(1) - edge)).astype(np.float32).astype(state_dtype)
    for _ in range(2 ** exp_times):
        s = v.copy()
        for d, (fwd, bwd) in enumerate(taps):
            if fwd is not None:
                dst, src = fwd
                s[:, dst[0], dst[1]] += v[:, src[0], src[1]] * Wd[d][dst]
            if bwd is not None:
                dst, src = bwd
                s[:, dst[0], dst[1]] += v[:, src[0], src[1]] * Wd[d][src]
        v = (s / cs.astype(state_dtype)).astype(state_dtype)
    return v.astype(np.float32).reshape(-1, 1, h, w)


def dense_from_weights(W, radius=5):
    """The symmetric n x n matrix the weights stand for (unit diagonal): what `scaled = dense ** beta` of the dense path is."""
    nd, h, w = W.shape
    n = h * w
    idx = np.arange(n).reshape(h, w)
    D = np.zeros((n, n), W.dtype)
    D[np.arange(n), np.arange(n)] = 1
    for d, (_p, (dy, dx)) in enumerate(directions(radius)):
        s = _shift(h, w, dy, dx)
        if s is None:
            continue
        f, t = idx[s[0]].reshape(-1), idx[s[1]].reshape(-1)
        D[f, t] = W[d][s[0]].reshape(-1)
        D[t, f] = W[d][s[0]].reshape(-1)
    return D
