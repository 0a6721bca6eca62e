"""Plain restatement of the dense IRN random walk and of the tail of infer_irn, with the number format as a parameter: the
yardstick of tests/test_gpu_irn_dense.py for the kernels of muscle_amd/csrc/irn.hip, pinned on the CPU by
tests/test_cpu_irn_dense.py (against the oracle in fp64, the reference's fixture and F.interpolate).

It follows the formulation of the model project's indexing.py (search paths -> the edge map padded with 1.0 -> the maximum
along every path -> a symmetric matrix with a unit diagonal -> ** beta -> columns divided by their sums -> exp_times
squarings -> one product with the masked class maps) and of infer_irn.py:78-94 (x4 half-pixel bilinear, crop, division by the
global maximum).  Nothing here comes from a HIP path and nothing is imported from muscle_amd: the path list is built here
and the CPU test asserts that it equals muscle_amd.indexing.search_paths.

dtype is numpy's float32 or float64.  In float32 every operation is one rounded fp32 operation in the order written here,
which is the order of the formulas above and not necessarily a kernel's; the one exception is the integral power, formed by
irn_walk_ref.power_f32 in irn_pow_colsum_kernel's multiplication order so that `scaled` can be compared bit for bit.
"""
import os
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
from irn_walk_ref import power_f32  # noqa: E402


# ---- search paths -------------------------------------------------------------------------------------------------------
def search_paths(radius=5):
    """[[(dy, dx), ...], ...]: for every one-sided search direction inside the open disc of `radius` the lattice points of the
    bounding box that lie less than one pixel from the straight line source -> destination, the farthest (the destination)
    first; directions with equally long paths stay together, shortest paths first, as the model project lists them."""
    r = int(radius)
    targets = [(0, dx) for dx in range(1, r)]
    targets += [(dy, dx) for dy in range(1, r) for dx in range(1 - r, r) if dy * dy + dx * dx < r * r]
    groups = {}
    for dy, dx in targets:
        box = [(y, x) for y in range(0, dy + 1) for x in range(min(dx, 0), max(dx, 0) + 1)]
        near = [(y, x) for y, x in box if (dy * x - dx * y) ** 2 / (dy * dy + dx * dx) < 1]      # squared distance to the line
        near = sorted(near, key=lambda p: -(abs(p[0]) + abs(p[1])))                              # stable: ties keep scan order
        groups.setdefault(len(near), []).append(near)
    return [path for length in sorted(groups) for path in groups[length]]


# ---- affinity -----------------------------------------------------------------------------------------------------------
def affinity(edge, radius=5, dtype=np.float64):
    """edge [h,w] or [1,h,w] -> dense [n,n], n = h*w: 1 on the diagonal; for every source pixel and every direction whose
    destination lies inside the image, dense[src][dst] = dense[dst][src] = 1 - max(edge along the path); 0 elsewhere.
    The edge map is padded with 1.0 (radius columns either side, radius rows below) as the model project pads it."""
    e = np.asarray(edge, dtype)
    h, w = e.shape[-2:]
    e = e.reshape(h, w)
    n = h * w
    r = int(radius)
    padded = np.ones((h + r, w + 2 * r), dtype)
    padded[:h, r:r + w] = e
    number = np.arange(n).reshape(h, w)
    dense = np.zeros((n, n), dtype)
    dense[np.arange(n), np.arange(n)] = 1
    for path in search_paths(r):
        dy, dx = path[0]
        rows, cols = h - dy, w - abs(dx)                       # sources whose destination is inside: a rows x cols window
        if rows <= 0 or cols <= 0:
            continue
        x0 = max(0, -dx)                                       # first source column of that window
        along = np.stack([padded[py:py + rows, r + x0 + px:r + x0 + px + cols] for py, px in path])
        aff = (dtype(1) - along.max(axis=0)).astype(dtype)
        src = number[0:rows, x0:x0 + cols].reshape(-1)
        dst = number[dy:dy + rows, x0 + dx:x0 + dx + cols].reshape(-1)
        dense[src, dst] = aff.reshape(-1)
        dense[dst, src] = aff.reshape(-1)
    return dense


def padded_affinity(dense, n4, ld=None, fill=0.0):
    """dense [n,n] -> [n4, ld] as mx_irn_affinity lays it out: rows / columns n..n4-1 are isolated vertices with a unit diagonal,
    columns n4..ld-1 hold `fill`."""
    n = dense.shape[0]
    ld = n4 if ld is None else ld
    out = np.zeros((n4, ld), dense.dtype)
    out[:, n4:] = fill
    out[:n, :n] = dense
    v = np.arange(n, n4)
    out[v, v] = 1
    return out


# ---- transition ---------------------------------------------------------------------------------------------------------
def transition(dense, beta, dtype=np.float64):
    """(scaled, colsum, T): scaled = dense ** beta, colsum[j] = sum_i scaled[i][j], T = scaled / colsum.  float64: a plain **.
    float32: an integral beta in 1..64 by irn_walk_ref.power_f32, any other beta by torch's fp32 pow on the CPU; the column sums
    are torch's fp32 sums."""
    d = np.asarray(dense, dtype)
    if dtype == np.float64:
        scaled = d ** np.float64(beta)
        colsum = scaled.sum(axis=0)
        return scaled, colsum, scaled / colsum
    if 0 < beta <= 64 and float(beta) == int(beta):
        scaled = power_f32(d, int(beta))
    else:
        scaled = torch.pow(torch.from_numpy(d), float(beta)).numpy()
    colsum = torch.from_numpy(scaled).sum(dim=0).numpy()
    return scaled, colsum, (scaled / colsum).astype(np.float32)


# ---- the walk -----------------------------------------------------------------------------------------------------------
def walk(x, edge, radius=5, beta=10, exp_times=8, dtype=np.float64):
    """x [..., C, h, w], edge [h,w] or [1,h,w] -> rw [C,1,h,w] = (x * (1 - edge)) @ T^(2^exp_times), all in `dtype`."""
    e = np.asarray(edge, dtype)
    h, w = e.shape[-2:]
    e = e.reshape(h, w)
    _, _, T = transition(affinity(e, radius, dtype), beta, dtype)
    T = torch.from_numpy(np.ascontiguousarray(T))
    for _ in range(int(exp_times)):
        T = T @ T
    masked = (np.asarray(x, dtype).reshape(-1, h, w) * (dtype(1) - e)).astype(dtype)
    rw = torch.from_numpy(masked.reshape(-1, h * w)) @ T
    return rw.numpy().reshape(-1, 1, h, w)


# ---- the tail of infer_irn ----------------------------------------------------------------------------------------------
def _taps(size_in, size_out, dtype):
    """Half-pixel x4 source coordinates of the first size_out output positions: (i0, i1, weight of i1).  The coordinate is a
    scaling by 1/4, exact in either format."""
    src = (np.arange(size_out, dtype=np.float64) + 0.5) * 0.25 - 0.5
    src = np.maximum(src, 0.0)
    i0 = np.minimum(np.floor(src).astype(np.int64), size_in - 1)
    i1 = np.minimum(i0 + 1, size_in - 1)
    return i0, i1, (src - i0).astype(dtype)


def upsample4(rw, H, W, dtype=np.float64):
    """rw [C,1,h,w] or [C,h,w] -> [C,H,W]: the top-left H x W of the x4 bilinear (align_corners=False) upsampling, tap by tap:
    (1-wy) * ((1-wx) * m00 + wx * m01) + wy * ((1-wx) * m10 + wx * m11)."""
    m = np.asarray(rw, dtype)
    h, w = m.shape[-2:]
    m = m.reshape(-1, h, w)
    assert 0 < H <= 4 * h and 0 < W <= 4 * w
    y0, y1, wy = _taps(h, H, dtype)
    x0, x1, wx = _taps(w, W, dtype)
    wy = wy[None, :, None]
    wx = wx[None, None, :]
    one = dtype(1)
    top = (one - wx) * m[:, y0][:, :, x0] + wx * m[:, y0][:, :, x1]
    bot = (one - wx) * m[:, y1][:, :, x0] + wx * m[:, y1][:, :, x1]
    return ((one - wy) * top + wy * bot).astype(dtype)


def finish_values(rw, H, W, dtype=np.float64):
    """[C,H,W]: upsample4 divided by its maximum, the values infer_irn compares with bg_thres and stores as the soft label."""
    up = upsample4(rw, H, W, dtype)
    return (up / up.max()).astype(dtype)


def top_two(values, bg_thres):
    """values [C,H,W] fp64 -> (stack [C+1,H,W] with the threshold plane in front, arg-max (first maximum), best, gap to the
    second best) per pixel."""
    v = np.asarray(values, np.float64)
    stack = np.concatenate([np.full((1,) + v.shape[1:], float(bg_thres)), v], axis=0)
    order = np.sort(stack, axis=0)
    return stack, stack.argmax(axis=0), order[-1], order[-1] - order[-2]


# (C, h, w, H, W) of the finish cases shared by the CPU and the GPU test
FINISH_CASES = [(20, 19, 23, 74, 90), (20, 19, 23, 76, 92), (1, 1, 1, 1, 1), (3, 1, 9, 4, 33), (3, 9, 1, 33, 4),
                (254, 3, 3, 12, 12), (5, 128, 128, 512, 512), (1, 257, 256, 1025, 1024)]


def finish_input(uniform, C, h, w):
    """The class maps of a finish case, fp32 [C,1,h,w]: uniform(9, "rw", ...) ** 2 (`uniform` = muscle_amd.synth.uniform, handed
    in), one absent class where C > 2, and at C = 254 a winner planted in the last class so that label 254 occurs."""
    rw = (uniform(9, "rw", (C, 1, h, w)).astype(np.float32) ** 2).astype(np.float32)
    if C > 2:
        rw[3 if C > 3 else 1] = 0
    if C == 254:
        rw[253, 0, h // 2, w // 2] = 1.5
    return rw
