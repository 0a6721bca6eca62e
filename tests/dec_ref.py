"""Plain restatements of the decoder kernels of muscle_amd/csrc/dec.hip and of the support kernels at the top of
muscle_amd/csrc/head.hip, in torch and numpy on CPU tensors, for tests/test_gpu_dec_kernels.py, tests/test_gpu_head_kernels.py
and tests/test_cpu_dec_ref.py (which checks every restatement against an independent statement of the same operation).

As in tests/bn_ref.py: functions that take `dtype` give the reference at float64 and the "plain fp32 restatement" at float32
(the same expressions, every operation rounded to fp32), whose own error against float64 calibrates the tolerances.  Where a
function returns (value, magnitude), the magnitude is the same expression with absolute values: one rounding error is at most
U = 2^-24 of it.  The case tables the GPU tests run are here too, so that the CPU checks of their input conditions cannot
drift away from them.
"""
import functools
import math

import numpy as np
import torch
import torch.nn.functional as F

U = 2.0 ** -24
F64, F32 = torch.float64, torch.float32
GRID_CAP = 8192 * 256          # gs() of dec.hip / head.hip: at most 8192 workgroups of 256 threads per sweep


def _c(t, dtype):
    return None if t is None else t.to(dtype)


# ---- avgpool3s2 -------------------------------------------------------------------------------------------------------------------
def _windows(H, W):
    """Output (o) covers the padded rows 2o + dy, dy = 0..2 (input rows 2o-1 .. 2o+1): the nine strided views of a padded map."""
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    return [(slice(dy, dy + 2 * Ho - 1, 2), slice(dx, dx + 2 * Wo - 1, 2)) for dy in range(3) for dx in range(3)]


def avgpool3s2(x, dtype=F64):
    """x [N,H,W,C] -> (window sum / 9, sum |x| / 9) [N,Ho,Wo,C] (pad 1, count_include_pad: always nine)."""
    xp = F.pad(x.to(dtype), (0, 0, 1, 1, 1, 1))
    s, m = 0, 0
    for sy, sx in _windows(x.shape[1], x.shape[2]):
        s, m = s + xp[:, sy, sx], m + xp[:, sy, sx].abs()
    return s / 9.0, m / 9.0


def avgpool3s2_bwd(g, H, W, dtype=F64):
    """g [N,Ho,Wo,C] -> gradient of the input [N,H,W,C]: the transpose - every window adds its output's gradient to its inputs."""
    g = g.to(dtype)
    gp = torch.zeros(g.shape[0], H + 2, W + 2, g.shape[3], dtype=dtype)
    mp = torch.zeros_like(gp)
    for sy, sx in _windows(H, W):
        gp[:, sy, sx] += g
        mp[:, sy, sx] += g.abs()
    return gp[:, 1:H + 1, 1:W + 1] / 9.0, mp[:, 1:H + 1, 1:W + 1] / 9.0


AVGPOOL_SHAPES = [(1, 1, 1, 4), (2, 2, 3, 4), (1, 5, 4, 8), (2, 7, 7, 36), (1, 257, 257, 512)]


def avgpool3s2_exact(x, bwd=False, H=None, W=None):
    """The kernel's result for integer-valued inputs below 2^20: the (exact) sum, rounded product with float32(1/9)."""
    s = (avgpool3s2_bwd(x, H, W)[0] if bwd else avgpool3s2(x)[0]) * 9.0
    s = torch.round(s)
    assert float(s.abs().max()) < 2 ** 24
    return s.float() * torch.tensor(1.0, dtype=F32).div(9.0)


# ---- bilinear, align_corners=True ---------------------------------------------------------------------------------------------
def bil_matrix(n_in, n_out, dtype=F64):
    """[n_out, n_in] weights of torch's upsample_bilinear2d(align_corners=True) along one axis: source coordinate
    s = d * (in-1)/(out-1) (0 when out == 1), i0 = floor(s) clamped to in-1, i1 = min(i0+1, in-1), weights 1-f and f."""
    W = torch.zeros(n_out, n_in, dtype=dtype)
    scale = (torch.tensor(float(n_in - 1), dtype=dtype) / torch.tensor(float(n_out - 1), dtype=dtype)) if n_out > 1 \
        else torch.tensor(0.0, dtype=dtype)
    s = scale * torch.arange(n_out, dtype=dtype)
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    f = s - i0.to(dtype)
    d = torch.arange(n_out)
    W[d, i0] += 1.0 - f
    W[d, i1] += torch.where(i1 != i0, f, torch.zeros_like(f))
    return W


def resize_nhwc(src, Hd, Wd, relu=False, dtype=F64):
    """src [N,Hs,Ws,C] -> (bilinear [N,Hd,Wd,C] with the optional relu, the same blend of |src|)."""
    Wy, Wx = bil_matrix(src.shape[1], Hd, dtype), bil_matrix(src.shape[2], Wd, dtype)
    src = src.to(dtype)
    v, m = (torch.einsum("bx,naxc->nabc", Wx, torch.einsum("ay,nyxc->naxc", Wy, t)) for t in (src, src.abs()))     # rows, then columns
    return (v.clamp_min(0.0) if relu else v), m


def resize_nhwc_bwd(g, Hs, Ws, dtype=F64):
    """g [N,Hd,Wd,C] -> (W_y (x) W_x)^T g [N,Hs,Ws,C], and the same with |g| (= sum |term| per source element)."""
    Wy, Wx = bil_matrix(Hs, g.shape[1], dtype), bil_matrix(Ws, g.shape[2], dtype)
    g = g.to(dtype)
    return tuple(torch.einsum("bx,nybc->nyxc", Wx, torch.einsum("ay,nabc->nybc", Wy, t)) for t in (g, g.abs()))


def upsample_to_nchw(src, K, Hd, Wd, dtype=F64):
    """src [N,Hs,Ws,lds] (the first K columns are classes) -> bilinear [N,K,Hd,Wd]."""
    v, m = resize_nhwc(src[..., :K], Hd, Wd, False, dtype)
    return v.permute(0, 3, 1, 2).contiguous(), m.permute(0, 3, 1, 2).contiguous()


def upsample_to_nchw_bwd(g, Hs, Ws, dtype=F64):
    """g [N,K,Hd,Wd] -> the transpose [N,Hs,Ws,K] (the K used columns of gsrc)."""
    return resize_nhwc_bwd(g.permute(0, 2, 3, 1), Hs, Ws, dtype)


def bil_slope_units(src, Hd, Wd):
    """The part of a bilinear output's error that comes from the source coordinate, in absolute terms per unit U: the coordinate
    (a rounded quotient times an index: two roundings) is off by at most 2U(in-1) source pixels, and the value is piecewise
    linear with a slope of at most the largest difference of neighbours along that axis of the actual source array."""
    src = src.double()
    dy = float((src[:, 1:] - src[:, :-1]).abs().max()) if src.shape[1] > 1 and Hd > 1 else 0.0
    dx = float((src[:, :, 1:] - src[:, :, :-1]).abs().max()) if src.shape[2] > 1 and Wd > 1 else 0.0
    return 2.0 * (src.shape[1] - 1) * dy + 2.0 * (src.shape[2] - 1) * dx


BLEND_OPS = 8        # 1-wx, two products and a sum per row, 1-wy, two products and a sum (contraction only removes some)


def adjoint_row_share(n_in, n_out):
    """The smallest share that one destination index (a whole destination row or column: what a gather range that is one index
    too tight drops) has in a source index's sum of weights: min over source indices of (smallest weight) / (sum of weights).
    Weights below the coordinate's own rounding error 4U(in-1) do not count: no fp32 evaluation resolves them."""
    W = bil_matrix(n_in, n_out)
    floor = 4.0 * U * max(n_in - 1, 1)
    big = torch.where(W > floor, W, torch.full_like(W, float("inf")))
    return float((big.min(0).values / W.sum(0)).min())


# (Hs, Ws, Hd, Wd): the BiFPN ladder at 96 px, a non-integer ratio, downsampling, identity, extents of 1, a large ratio
RESIZE_SIZES = [(3, 3, 6, 6), (6, 6, 12, 12), (7, 9, 13, 17), (13, 17, 7, 9), (5, 5, 5, 5), (1, 4, 5, 9), (4, 1, 9, 5),
                (4, 5, 1, 1), (4, 5, 1, 7), (2, 2, 64, 64)]
# (N, C, Hs, Ws, Hd, Wd): the lists above at both C and N, and one case above the grid cap in each direction
RESIZE_CASES = [(n, c) + s for s in RESIZE_SIZES for (n, c) in ((1, 4), (3, 36), (1, 36), (3, 4))] + \
    [(1, 4, 16, 16, 1449, 1449),          # forward: 1449*1449 float4s > 2 097 152
     (1, 4, 1449, 1449, 16, 16)]          # backward of the downsampling: 1449*1449 source float4s
# (N, K, lds, Hs, Ws, Hd, Wd); (28,28)->(448,448): Hd*Ws*4 = 50 176 B above the 48 KB threshold; (40,40)->(250,250): 40 000 B below
UPSAMPLE_CASES = [(n, k, l) + s for s in RESIZE_SIZES for (n, k, l) in ((1, 1, 1), (2, 21, 24), (1, 21, 21), (2, 1, 24))] + \
    [(1, 2, 2, 28, 28, 448, 448), (1, 1, 1, 40, 40, 250, 250), (1, 3, 4, 16, 16, 840, 840)]     # the last: forward above the grid cap


def case_seed(*ints):
    s = 12345
    for v in ints:
        s = (s * 1000003 + int(v)) % (2 ** 31 - 1)
    return s


def signed_unit(shape, gen):
    """+-(0.5 .. 1.5): every |value| within a factor 3 of every other, so that a term's share follows from its weight."""
    return (torch.rand(shape, generator=gen) + 0.5) * (torch.randint(0, 2, shape, generator=gen) * 2 - 1).float()


RESIZE_FWD_ONLY = (1, 4, 16, 16, 1449, 1449)          # the cases that exist for the forward sweep alone
UPSAMPLE_FWD_ONLY = (1, 3, 4, 16, 16, 840, 840)


def resize_inputs(case):
    """(src, g, base) of a RESIZE case (N, C, Hs, Ws, Hd, Wd): source, destination gradient, the non-zero starting gradient."""
    N, C, Hs, Ws, Hd, Wd = case
    gen = torch.Generator().manual_seed(case_seed(*case))
    return torch.randn(N, Hs, Ws, C, generator=gen), signed_unit((N, Hd, Wd, C), gen), torch.randn(N, Hs, Ws, C, generator=gen)


def upsample_inputs(case):
    """(src [N,Hs,Ws,lds], g [N,K,Hd,Wd], base [N,Hs,Ws,lds]) of an UPSAMPLE case."""
    N, K, lds, Hs, Ws, Hd, Wd = case
    gen = torch.Generator().manual_seed(case_seed(*case))
    return torch.randn(N, Hs, Ws, lds, generator=gen), signed_unit((N, K, Hd, Wd), gen), torch.randn(N, Hs, Ws, lds, generator=gen)


def sum_rule(ref32, ref, mag):
    """(e_ref, relative allowance 4 e_ref + 2U) of the sum rule, both relative to sum |term|."""
    e_ref = float(((ref32.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    return e_ref, 4.0 * e_ref + 2.0 * U


def adjoint_rule(g_nhwc, Hs, Ws):
    """For a bilinear adjoint on destination gradient g [N,Hd,Wd,C]: (reference, sum |term|, e_ref, allowance, share), share = the
    smallest share a whole destination row or column has in a source element's sum: the weight share of adjoint_row_share over
    3 (|g| lies in 0.5 .. 1.5).  The allowance must stay below a tenth of it (asserted by the tests, here and on the GPU)."""
    ref, mag = resize_nhwc_bwd(g_nhwc, Hs, Ws)
    e_ref, rel = sum_rule(resize_nhwc_bwd(g_nhwc, Hs, Ws, F32)[0], ref, mag)
    share = min(adjoint_row_share(Hs, g_nhwc.shape[1]), adjoint_row_share(Ws, g_nhwc.shape[2])) / 3.0
    return ref, mag, e_ref, rel, share


# ---- cross entropy against the arg-max label ----------------------------------------------------------------------------------
def ce_argmax(seg, mask, dtype=F64):
    """seg, mask [N,K,HW].  Label = the FIRST maximum of mask over K (np.argmax guarantees the first).  Returns
    (mean loss, magnitude of the mean = mean of |max| + |log sum exp| + |seg_t|, labels [N,HW])."""
    t = torch.from_numpy(np.argmax(mask.numpy(), axis=1))
    s = seg.to(dtype)
    mx = s.max(1).values
    lse = mx + torch.log(torch.exp(s - mx[:, None]).sum(1))
    st = s.gather(1, t[:, None]).squeeze(1)
    term = lse - st
    return term.mean(), (mx.abs() + (lse - mx).abs() + st.abs()).double().mean(), t


def ce_argmax_bwd(seg, mask, gup, dtype=F64):
    """gup * (softmax(seg) - onehot(label)) / (N*HW); magnitude gup * (softmax + onehot) / (N*HW)."""
    t = torch.from_numpy(np.argmax(mask.numpy(), axis=1))
    s = seg.to(dtype)
    mx = s.max(1, keepdim=True).values
    lse = mx + torch.log(torch.exp(s - mx).sum(1, keepdim=True))
    p = torch.exp(s - lse)
    oh = torch.zeros_like(p).scatter_(1, t[:, None], 1.0)
    inv = torch.tensor(1.0, dtype=dtype) / (seg.shape[0] * seg.shape[2])
    g = torch.tensor(gup, dtype=dtype) * inv
    return g * (p - oh), g.abs() * (p + oh)


CE_SHAPES = [(1, 2, 1), (2, 21, 323), (3, 21, 70001), (1, 2, GRID_CAP + 77)]


def ce_inputs(shape, kind):
    """kind 'spread': logits over +-40, masks with zero pixels (label 0), two and three equal maxima.
    kind 'confident': one-hot logits of +-6 on the label: the loss is near zero (about 1e-4)."""
    N, K, HW = shape
    gen = torch.Generator().manual_seed(case_seed(N, K, HW, kind == "spread"))
    mask = torch.randint(0, 8, (N, K, HW), generator=gen).float() / 8.0            # exactly representable: ties are exact
    r = torch.rand(N, 1, HW, generator=gen)
    mask = torch.where(r < 0.2, torch.zeros_like(mask), mask)                         # all-zero pixels: label 0
    top = mask.max(1, keepdim=True).values
    k2 = torch.randint(0, K, (N, 1, HW), generator=gen)
    k3 = torch.randint(0, K, (N, 1, HW), generator=gen)
    idx = torch.arange(K).view(1, K, 1)
    mask = torch.where((r > 0.6) & (idx == k2), top.expand_as(mask), mask)            # a second equal maximum
    mask = torch.where((r > 0.8) & (idx == k3), top.expand_as(mask), mask)            # and a third
    if kind == "spread":
        seg = (torch.rand(N, K, HW, generator=gen) * 2 - 1) * 40.0
    else:
        t = torch.from_numpy(np.argmax(mask.numpy(), axis=1))
        seg = torch.full((N, K, HW), -6.0).scatter_(1, t[:, None], 6.0) + torch.randn(N, K, HW, generator=gen) * 0.1
    return seg.contiguous(), mask.contiguous()


# ---- clip_grad_norm -------------------------------------------------------------------------------------------------------------
def clip_grad_norm(x, max_norm, dtype=F64):
    """(norm, scaled vector, coef): coef = min(1, max_norm / (norm + 1e-6)); the vector is multiplied only when coef < 1."""
    x = x.to(dtype)
    total = torch.sqrt((x * x).sum())
    coef = torch.clamp(max_norm / (total + 1e-6), max=1.0)
    return total, (x * coef if float(coef) < 1.0 else x.clone()), coef


CLIP_N = [1, 255, 1001, 2048 * 256 + 3, 4096 * 256 + 5]


# ---- FieldLoss stage 1: edges -------------------------------------------------------------------------------------------------
def sobel5(dtype=F64):
    """[2,1,5,5]: the 5x5 Sobel pair with the reference's 1e-6 for its "zero" entries (the centre of Gx is 0.0), as fp32 holds them."""
    gx = torch.tensor([[2.0, 1.0, 1e-6, -1.0, -2.0], [3.0, 2.0, 1e-6, -2.0, -3.0], [4.0, 3.0, 0.0, -3.0, -4.0],
                       [3.0, 2.0, 1e-6, -2.0, -3.0], [2.0, 1.0, 1e-6, -1.0, -2.0]], dtype=F32)
    gy = torch.tensor([[2.0, 3.0, 4.0, 3.0, 2.0], [1.0, 2.0, 3.0, 2.0, 1.0], [1e-6] * 5,
                       [-1.0, -2.0, -3.0, -2.0, -1.0], [-2.0, -3.0, -4.0, -3.0, -2.0]], dtype=F32)
    return torch.stack([gx, gy]).unsqueeze(1).to(dtype)


_DIV32 = np.float32(3.1416) / np.float32(8.0)
# the sector boundaries as the kernel's fp32 constants: k * div for odd k in -7..7, and +-8 * div
SECTOR_BOUNDS = np.array([float(np.float32(k) * _DIV32) for k in (-8, -7, -5, -3, -1, 1, 3, 5, 7, 8)])
M_ZERO = float(np.sqrt(np.float32(1e-8)))          # the magnitude of an unlabelled class: sqrtf(1e-8f)


def sector(ang):
    """The sector 0..7 of an angle (float64 tensor) by OrientQuantize's intervals; angles outside +-8*div fall to 7, as the
    kernel's final return does."""
    b = SECTOR_BOUNDS
    q = torch.full(ang.shape, 7, dtype=torch.long)
    for lo, hi, v in ((b[5], b[6], 0), (b[6], b[7], 1), (b[7], b[8], 2), (b[8], b[9], 3), (b[0], b[1], 3), (b[1], b[2], 4),
                      (b[2], b[3], 5), (b[3], b[4], 6)):
        q[(ang >= lo) & (ang < hi)] = v
    return q


def boundary_distance(ang):
    return (ang.double()[..., None] - torch.from_numpy(SECTOR_BOUNDS)).abs().min(-1).values


def field_edges(seg, lab, beta, dtype=F64):
    """seg [N,K,H,W], lab [N,K-1].  Returns a dict: prob [N,F,H,W], mag, mag_m (magnitude of mag: |l| * sum |kernel| p, + 1e-4),
    ang (atan2), orient (sector), mx [N,F] (0 where unlabelled), edge_fg [N,H,W], gx, gy."""
    N, K, H, W = seg.shape
    Fg = K - 1
    s = seg.to(dtype) * torch.tensor(beta, dtype=dtype)
    p = torch.softmax(s, 1)[:, 1:]
    k = sobel5(dtype)
    e = F.conv2d(p.reshape(N * Fg, 1, H, W), k, padding=2).view(N, Fg, 2, H, W)
    em = F.conv2d(p.reshape(N * Fg, 1, H, W), k.abs(), padding=2).view(N, Fg, 2, H, W)
    l = lab.to(dtype).view(N, Fg, 1, 1)
    labelled = (lab != 0).view(N, Fg, 1, 1)
    zero = torch.zeros((), dtype=dtype)
    gx, gy = torch.where(labelled, e[:, :, 0] * l, zero), torch.where(labelled, e[:, :, 1] * l, zero)   # unlabelled: +0, angle 0, sector 7
    mag = torch.sqrt(gx * gx + gy * gy + 1e-8)
    ang = torch.atan2(gy, gx)
    mx = torch.where(labelled.view(N, Fg), mag.view(N, Fg, -1).max(-1).values, torch.zeros(N, Fg, dtype=dtype))
    return dict(prob=p, mag=mag, mag_m=(em[:, :, 0] + em[:, :, 1]) * l.abs() + 1e-4, ang=ang, orient=sector(ang.double()), mx=mx,
                edge_fg=mag.sum(1), gx=gx, gy=gy, labelled=labelled.expand(N, Fg, H, W))


def smooth_field(seed, shape, passes=3):
    """Unit-variance noise smoothed by `passes` 5x5 box filters (as _smooth_field of tests/test_oracle_golden.py)."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen)
    k = torch.ones(shape[1], 1, 5, 5) / 25.0
    for _ in range(passes):
        x = F.conv2d(x, k, padding=2, groups=shape[1])
    return (x / x.std()).contiguous()


# (N, K, H, W): HW = 99, two samples in one workgroup; one workgroup per sample; a straddle of two; F = 65 (LDS and direct path);
# above the grid cap; HW = 99 with a third sample in the first workgroup
EDGE_SHAPES = [(2, 21, 9, 11), (3, 4, 16, 16), (2, 21, 37, 41), (1, 66, 8, 8), (1, 2, 1449, 1449), (3, 21, 9, 11)]
EDGE_BETAS = [100.0, 2.0]
EDGE_CALIB = (2, 21, 64, 64)


def edge_empty_sample(N):
    """The sample without any labelled class: none at N = 1, the first at N = 2, the second from N = 3 - so that the samples a
    workgroup reaches after its first one (the direct atomicMax path) do have labelled classes."""
    return None if N == 1 else (0 if N == 2 else 1)


def edge_inputs(shape, beta):
    """Smoothed logits (x 0.05 at beta = 100, as the golden field inputs; x 1 at beta = 2) and label rows with zeros, ones and one
    0.5; one sample of a batch of more than one (edge_empty_sample) has no labelled class at all."""
    N, K, H, W = shape
    seg = smooth_field(case_seed(N, K, H, W), shape) * (0.05 if beta > 10 else 1.0)
    gen = torch.Generator().manual_seed(case_seed(N, K, H, W, 7))
    lab = (torch.rand(N, K - 1, generator=gen) < 0.4).float()
    lab[:, 0] = 1.0
    empty = edge_empty_sample(N)
    first = 1 if empty == 0 else 0
    if K - 1 > 1:
        lab[first, 1] = 0.5
    if K - 1 >= 65:
        lab[first, 64] = 1.0                             # the direct path of f >= 64 is labelled
    if empty is not None:
        lab[empty] = 0.0
    return seg.contiguous(), lab.contiguous()


def orient_compare_mask(ref, ang_err):
    """Where the sector is compared: labelled, float64 magnitude at least 1e-3 of its plane's maximum, float64 angle farther from
    every sector boundary than 4 x the measured angle error.  Returns (mask, floor mask)."""
    mag = ref["mag"].double()
    floor = ref["labelled"] & (mag >= 1e-3 * mag.flatten(2).max(-1).values[..., None, None])
    return floor & (boundary_distance(ref["ang"]) > 4.0 * ang_err), floor


def angle_error(seg, lab, beta, ref=None):
    """The largest angle error of the fp32 restatement on the labelled pixels above the magnitude floor (wrapped to +-pi)."""
    ref = ref or field_edges(seg, lab, beta)
    r32 = field_edges(seg, lab, beta, F32)
    floor = orient_compare_mask(ref, 0.0)[1]
    if not bool(floor.any()):
        return 0.0
    d = (r32["ang"].double() - ref["ang"]).abs()
    d = torch.minimum(d, 2 * math.pi - d)
    return float(d[floor].max())


# ---- FieldLoss stage 2: point lists -------------------------------------------------------------------------------------------
def field_select(mag, orient, mx, slots, step, H, W):
    """mag fp32 [N,F,HW], orient uint8 [N,F,HW], mx fp32 [N,F] (numpy).  Per slot (n,f): positives by the kernel's fp32
    comparison mag >= 0.8f*m && m > 1 in row-major order, FieldLoss.in_out_div's indices, margins removed.
    Returns (out lists, in lists, counts [S,3] = n_out, n_in, n_pos)."""
    HW = H * W
    outs, ins, counts = [], [], []
    ind = np.arange(HW, dtype=np.int64)
    for n, f in slots:
        m = np.float32(mx[n, f])
        pos = (mag[n, f].astype(np.float32) >= np.float32(0.8) * m) & bool(m > np.float32(1.0))
        o = orient[n, f].astype(np.int64) + 1
        o4, o26 = (o % 4 == 0).astype(np.int64), ((o == 2) | (o == 6)).astype(np.int64)
        lt4 = (o < 4).astype(np.int64)
        oi = ind + np.where(lt4 == 1, step * step, -step) * (o4 * W) + np.where((1 + o) % 2 == 1, -1, 1) * o26
        ii = ind + np.where(lt4 == 1, -step, 1) * (o4 * W) + np.where(o % 2 == 1, -1, 1) * o26

        def keep(x):
            r = np.mod(x, W - 1)
            return (r != 0) & (r != 1) & (x > 0) & (x < HW - 1)
        outs.append(oi[pos & keep(oi)].astype(np.int32))
        ins.append(ii[pos & keep(ii)].astype(np.int32))
        counts.append([len(outs[-1]), len(ins[-1]), int(pos.sum())])
    return outs, ins, np.array(counts, dtype=np.int32)


SELECT_HW = [(3, 3), (5, 7), (16, 16), (17, 19), (40, 33)]
SELECT_STEPS = [1, 7, 40]


def select_inputs(H, W):
    """Synthetic planes [N=2, F=3]: all eight sectors; magnitudes drawn from {0.5, 1.59, 1.6, 1.61, 2.0} x the plane's scale, so
    that the fp32 comparison with 0.8f * m is decided at its edge; plane (0,1) has m <= 1 (no positives), plane (1,2) is all
    positive.  Slots in non-sorted order."""
    gen = torch.Generator().manual_seed(case_seed(H, W, 3))
    N, Fg, HW = 2, 3, H * W
    orient = torch.randint(0, 8, (N, Fg, HW), generator=gen).to(torch.uint8)
    orient[:, :, :8] = torch.arange(8, dtype=torch.uint8)[:HW][None, None] if HW >= 8 else orient[:, :, :8]
    table = torch.tensor([0.5, 1.59, 1.6, 1.61, 2.0])
    mag = table[torch.randint(0, 5, (N, Fg, HW), generator=gen)]
    mag[0, 1] *= 0.5                                      # maximum 1.0: m > 1 fails
    mag[1, 2] = 2.0 - torch.rand(HW, generator=gen) * 0.25      # every pixel >= 0.8 * max
    mag[:, :, HW - 1] = torch.where(mag[:, :, HW - 1] > 0, mag.flatten(2).max(-1).values, mag[:, :, HW - 1])
    mx = mag.max(-1).values
    slots = [(1, 2), (0, 0), (0, 1), (1, 0), (0, 2)]
    return mag.contiguous(), orient.contiguous(), mx.contiguous(), slots


# ---- FieldLoss stage 3: features at points ------------------------------------------------------------------------------------
def point_values(dense, mode, pts, H, W, dtype=F64):
    """The channel vectors at the points [npts, CH] (and the same blend of |dense|): mode 0 reads NCHW [N,CH,H,W], mode 1 the
    align_corners bilinear value of a low-resolution NHWC map [N,h,w,CH]."""
    n, p = pts[:, 0].long(), pts[:, 1].long()
    y, x = p // W, p % W
    d = dense.to(dtype)
    if mode == 0:
        v = d[n, :, y, x]
        return v, v.abs()
    Wy, Wx = bil_matrix(d.shape[1], H, dtype)[y], bil_matrix(d.shape[2], W, dtype)[x]      # [npts, h], [npts, w]
    return torch.einsum("qa,qb,qabc->qc", Wy, Wx, d[n]), torch.einsum("qa,qb,qabc->qc", Wy, Wx, d[n].abs())


def field_gather(dense, mode, mask, pts, K, ML, H, W, dtype=F64):
    """(softmax over channels of the point values [npts,CH], softmax over the K classes of mask [N,K,H,W] at the points padded
    with zeros to ML columns)."""
    v, _ = point_values(dense, mode, pts, H, W, dtype)
    n, p = pts[:, 0].long(), pts[:, 1].long()
    mf = torch.zeros(pts.shape[0], ML, dtype=dtype)
    mf[:, :K] = torch.softmax(mask.to(dtype)[n, :, p // W, p % W], 1)
    return torch.softmax(v, 1), mf


# ---- FieldLoss stage 5: the eight terms ---------------------------------------------------------------------------------------
def field_terms(sim, simm, inv_n, dtype=F64):
    """sim, simm [S,k,k].  Per slot and direction (rows: mean over columns; columns: mean over rows) the classes FP (mask above its
    mean, features not: -), FN (+), TP (neither: +), TN (both: -), each the mean of the feature means of its members; empty
    classes are skipped.  Returns dict: slot_loss [S] (x inv_n), terms [S,2,4], counts [S,2,4], gsim (autograd), margins
    (|row mean - total mean| and |column mean - total mean|, smallest per slot, for sim and simm: [S,2,2])."""
    S, k, _ = sim.shape
    sim = sim.to(dtype).clone().requires_grad_(True)
    simm = simm.to(dtype)
    terms, counts, margins, losses = torch.zeros(S, 2, 4, dtype=dtype), torch.zeros(S, 2, 4, dtype=torch.long), \
        torch.zeros(S, 2, 2, dtype=F64), []
    sign = (-1.0, 1.0, 1.0, -1.0)
    plus = 0.0                                   # the same terms all added: its gradient is the magnitude of gsim
    for s in range(S):
        loss = 0.0
        for d, dim in enumerate((1, 0)):
            m, mm = sim[s].mean(dim), simm[s].mean(dim)
            tot, totm = sim[s].mean(), simm[s].mean()
            sm, sd = mm > totm, (m > tot).detach()
            margins[s, d, 0] = float((m - tot).detach().abs().min())
            margins[s, d, 1] = float((mm - totm).abs().min())
            for c, sel in enumerate((sm & ~sd, ~sm & sd, ~sm & ~sd, sm & sd)):
                counts[s, d, c] = int(sel.sum())
                if counts[s, d, c] > 0:
                    t = m[sel].mean()
                    terms[s, d, c] = float(t.detach())
                    loss = loss + sign[c] * t
                    plus = plus + t * inv_n
        losses.append(loss * inv_n)
    gsim, = torch.autograd.grad(sum(losses), sim, retain_graph=True)
    gsim_m, = torch.autograd.grad(plus, sim)
    return dict(slot_loss=torch.stack([l.detach() for l in losses]), terms=terms, counts=counts, gsim=gsim, gsim_m=gsim_m,
                margins=margins)


TERMS_K = [4, 100, 128, 256]
TERMS_S = [1, 5]


def terms_inputs(k, S):
    """sim = base + r_i + c_j with offsets from {-3,-1,1,3}/64 (+ noise 100 times smaller): every row and column mean is at least
    1/64 from the total mean up to the noise.  All four classes occur along both dimensions in slot 0; in slot 1 (S > 1) the mask's
    offsets equal the features', so FP and FN are empty (cnt == 0)."""
    gen = torch.Generator().manual_seed(case_seed(k, S, 5))
    i = torch.arange(k)
    size = (1.0 + 2.0 * ((i // 4) % 2)) / 64.0

    def offsets():
        """(feature offsets, mask offsets): signs by i % 2 and by (i // 2) % 2 - each group of four indices holds all four sign
        pairs - under one shared random permutation; both have mean zero (k is a multiple of 4)."""
        perm = torch.randperm(k, generator=gen)
        return ((2.0 * (i % 2) - 1.0) * size)[perm], ((2.0 * ((i // 2) % 2) - 1.0) * size)[perm]
    sim, simm = torch.zeros(S, k, k), torch.zeros(S, k, k)
    for s in range(S):
        (r, rm), (c, cm) = offsets(), offsets()
        if s == 1:
            rm, cm = r, c
        sim[s] = 0.5 + r[:, None] + c[None, :] + torch.randn(k, k, generator=gen) * 1e-4
        simm[s] = 0.25 + rm[:, None] + cm[None, :] + torch.randn(k, k, generator=gen) * 1e-4
    return sim.contiguous(), simm.contiguous()


# ---- FieldLoss stage 6: the gradient of the dense map -------------------------------------------------------------------------
def field_scatter(feat, gfeat, pts, mode, dense_shape, gup, H, W, dtype=F64):
    """d/d dense of gup * sum(gfeat * softmax(values at points)) with the softmax `feat` given: per point
    g = feat * (gfeat - sum(gfeat * feat)) * gup, spread with the point's weights (mode 0: its own NCHW pixel; mode 1: the bilinear
    corners of the low-resolution NHWC map).  Returns (gradient, sum |term| per element), term = weight x point gradient."""
    f, gf = feat.to(dtype), gfeat.to(dtype)
    g = f * (gf - (gf * f).sum(1, keepdim=True)) * gup
    gm = f * (gf.abs() + (gf.abs() * f).sum(1, keepdim=True)) * abs(gup)
    n, p = pts[:, 0].long(), pts[:, 1].long()
    y, x = p // W, p % W
    out, mag = torch.zeros(dense_shape, dtype=dtype), torch.zeros(dense_shape, dtype=dtype)
    if mode == 0:
        for q in range(pts.shape[0]):
            out[n[q], :, y[q], x[q]] += g[q]
            mag[n[q], :, y[q], x[q]] += gm[q]
        return out, mag
    Wy, Wx = bil_matrix(dense_shape[1], H, dtype)[y], bil_matrix(dense_shape[2], W, dtype)[x]
    for q in range(pts.shape[0]):
        w2 = Wy[q][:, None] * Wx[q][None, :]
        out[n[q]] += w2[:, :, None] * g[q]
        mag[n[q]] += w2[:, :, None] * gm[q]
    return out, mag


def scatter_point_share(feat, gfeat, pts, mode, dense_shape, gup, H, W):
    """For every point, the largest share any of its terms (corner weight x channel gradient) has in the sum |term| of the element
    it goes to; the smallest of these over the points: what dropping one whole point would at least change, relative to sum |term|."""
    f, gf = feat.double(), gfeat.double()
    g = (f * (gf - (gf * f).sum(1, keepdim=True)) * gup).abs()
    _, mag = field_scatter(feat, gfeat, pts, mode, dense_shape, gup, H, W)
    n, p = pts[:, 0].long(), pts[:, 1].long()
    y, x = p // W, p % W
    worst = float("inf")
    for q in range(pts.shape[0]):
        if mode == 0:
            share = (g[q] / mag[n[q], :, y[q], x[q]].clamp_min(1e-300)).max()
        else:
            w2 = bil_matrix(dense_shape[1], H)[y[q]][:, None] * bil_matrix(dense_shape[2], W)[x[q]][None, :]
            share = (w2[:, :, None] * g[q] / mag[n[q]].clamp_min(1e-300)).max()
        worst = min(worst, float(share))
    return worst


# (h, w) of the low-resolution map, (H, W) = 8 * (h, w) - 3; CH: 300 strides threads over channels, 320 is an 80 KB tile
SCATTER_HW = [(3, 3), (13, 9), (8, 8), (17, 16)]
SCATTER_CH = [4, 64, 200, 300, 320]


def scatter_inputs(h, w, CH, mode):
    """N = 3 with no point in sample 1; 40 points: the fixed ones of field_points_for, eight more on pixel 0 of sample 0, and (where
    the map has more than one 8 x 8 tile each way) one whose four bilinear corners lie in four tiles.
    The base gradient is of the size of the terms (0.01).  Returns (feat, gfeat, pts, base, N, H, W, dense shape)."""
    N, H, W = 3, 8 * h - 3, 8 * w - 3
    gen = torch.Generator().manual_seed(case_seed(h, w, CH, mode))
    pts = field_points_for(N, H, W, 40, gen, empty_sample=1)
    pts[8:16, 0], pts[8:16, 1] = 0, 0
    if h > 8 and w > 8:
        pts[16, 0], pts[16, 1] = 2, math.ceil(7.5 * (H - 1) / (h - 1)) * W + math.ceil(7.5 * (W - 1) / (w - 1))
    feat = torch.softmax(torch.randn(40, CH, generator=gen) * 2.0, 1)
    gfeat = torch.randn(40, CH, generator=gen)
    shape = (N, h, w, CH) if mode == 1 else (N, CH, H, W)
    return feat, gfeat, pts, torch.randn(shape, generator=gen) * 0.01, N, H, W, shape


def field_scatter_autograd(dense, gfeat, pts, mode, gup, H, W):
    """The same gradient by autograd of the float64 restatement of stage 3."""
    d = dense.double().clone().requires_grad_(True)
    v, _ = point_values(d, mode, pts, H, W)
    (gup * (gfeat.double() * torch.softmax(v, 1)).sum()).backward()
    return d.grad


def field_points_for(N, H, W, npts, gen, empty_sample=None):
    """[npts, 2] int32 rows {n, pixel}: the four corners, the last row and column, repeated points, the rest random; no point in
    `empty_sample`."""
    fixed = [0, W - 1, (H - 1) * W, H * W - 1, (H - 1) * W + W // 2, (H // 2) * W + W - 1, H * W - 1, 0]
    pix = torch.tensor((fixed + torch.randint(0, H * W, (max(npts - len(fixed), 0),), generator=gen).tolist())[:npts])
    ok = [i for i in range(N) if i != empty_sample]
    n = torch.tensor(ok)[torch.randint(0, len(ok), (npts,), generator=gen)]
    return torch.stack([n, pix], 1).int().contiguous()


# ---- head.hip support kernels -------------------------------------------------------------------------------------------------
def row_l2norm(x, eps, dtype=F64):
    """y = x / (||x|| + eps) per row, the norm; a zero row gives y = 0.  Returns (y, norm, |y|)."""
    x = x.to(dtype)
    n = torch.sqrt((x * x).sum(1))
    y = x / (n + eps)[:, None]
    return y, n, y.abs()


def row_l2norm_bwd(x, nrm, gy, eps, dtype=F64):
    """The kernel's stated formula gx = gy/(n+eps) - (x/n) * (gy.x)/(n+eps)^2, the second term switched off for a zero row.
    Returns (gx, magnitude with |gy|, |x| and sum |gy x|)."""
    x, n, gy = x.to(dtype), nrm.to(dtype), gy.to(dtype)
    inv = 1.0 / (n + eps)
    safe = torch.where(n > 0, n, torch.ones_like(n))
    on = (n > 0).to(dtype)
    k = (gy * x).sum(1) * inv * inv / safe * on
    km = (gy * x).abs().sum(1) * inv * inv / safe * on
    return gy * inv[:, None] - x * k[:, None], gy.abs() * inv[:, None] + x.abs() * km[:, None]


def pcm_norm(T, K, eps, dtype=F64):
    """T [rows, L]: rv[:, k] = T[:, k] / (T[:, K] + eps) for k < K, zero in the columns from K on."""
    T = T.to(dtype)
    out = torch.zeros_like(T)
    out[:, :K] = T[:, :K] / (T[:, K] + eps)[:, None]
    return out, out.abs()


def pcm_norm_bwd(T, grv, K, eps, dtype=F64):
    """gT[:, k] = grv[:, k] * r (k < K); gT[:, K] = -sum_k grv[:, k] T[:, k] r^2; zero beyond; r = 1 / (T[:, K] + eps)."""
    T, g = T.to(dtype), grv.to(dtype)
    r = 1.0 / (T[:, K] + eps)
    out, mag = torch.zeros_like(T), torch.zeros_like(T)
    out[:, :K] = g[:, :K] * r[:, None]
    mag[:, :K] = out[:, :K].abs()
    out[:, K] = -(g[:, :K] * T[:, :K]).sum(1) * r * r
    mag[:, K] = (g[:, :K] * T[:, :K]).abs().sum(1) * r * r
    return out, mag


def sym_relu_grad(gaff, aff, n):
    """out[b,i,j] = (gaff[b,i,j] + gaff[b,j,i]) * (aff[b,i,j] > 0) for j < n; the padding columns j >= n are written as zero."""
    g = gaff.double()
    out = torch.zeros_like(g)
    out[:, :, :n] = (g[:, :, :n] + g[:, :, :n].transpose(1, 2)) * (aff[:, :, :n] > 0)
    return out


def ew(op, a, b=None, y=None, alpha=1.0, dtype=F64):
    """op 0: alpha*a; op 1: a + alpha*b; op 2: (y > 0) ? a (+ b) : 0.  Returns (value, magnitude)."""
    a, b = a.to(dtype), _c(b, dtype)
    if op == 0:
        return alpha * a, (alpha * a).abs()
    if op == 1:
        return a + alpha * b, a.abs() + (alpha * b).abs()
    v = a + b if b is not None else a
    m = a.abs() + b.abs() if b is not None else a.abs()
    return torch.where(y > 0, v, torch.zeros_like(v)), m


def bcast_add(X, v, alpha, rps, dtype=F64):
    """X[r, :] + alpha * v[r // rps, :]."""
    X, v = X.to(dtype), v.to(dtype)
    n = torch.arange(X.shape[0]) // rps
    return X + alpha * v[n], X.abs() + (alpha * v[n]).abs()


# ---- measured errors of the fp32 restatements, and the rules the GPU tests and tests/test_cpu_dec_ref.py share -----------------
def units(x32, ref, mag):
    """The largest error of an fp32 restatement against float64, in units of U * magnitude.  Elements whose magnitude is below
    the smallest normal fp32 number are left out: there the restatement's error is the spacing of subnormals (or a flush to
    zero), not a property of the expression (the GPU checks grant such elements one subnormal absolutely instead)."""
    err, m = (x32.double() - ref.double()).abs(), mag.double()
    keep = m >= 2.0 ** -126
    return float((err[keep] / (U * m[keep])).max()) if bool(keep.any()) else 0.0


CE_CALIB = (2, 21, 8192)
CE_GUP = float(torch.tensor(0.37, dtype=F32))


@functools.lru_cache(maxsize=None)
def ce_bwd_units(kind):
    """The fp32 restatement of the cross-entropy gradient on the fixed draw CE_CALIB of the kind's distribution."""
    seg, mask = ce_inputs(CE_CALIB, kind)
    ref, mag = ce_argmax_bwd(seg, mask, CE_GUP)
    return units(ce_argmax_bwd(seg, mask, CE_GUP, F32)[0], ref, mag)


def ce_fwd_rule(seg, mask):
    """(reference mean, its magnitude, e_ref, allowance) of the sum rule for the cross-entropy loss."""
    ref, mag, _ = ce_argmax(seg, mask)
    e_ref = abs(float(ce_argmax(seg, mask, F32)[0]) - float(ref)) / float(mag)
    return ref, mag, e_ref, 4.0 * e_ref + 2.0 * U


def ce_exact_inputs(shape):
    """The exact regime of the loss: the label's logit is an integer b in -3..3, the next class (cyclically) holds b + d with an
    integer d in 20..27, every other class -100.  In fp32 exp(-d) vanishes beside 1, so log sum exp = b + d and every term is the
    integer d: every partial sum is exact and the loss is float32(sum d / (N*HW)).  One pixel dropped or doubled moves the sum by
    at least 20 of about 23.5 per pixel: at 2^21 pixels that is 7 units in the last place of the result.
    Returns (seg, mask, the expected loss as a float32 tensor [1])."""
    N, K, HW = shape
    _, mask = ce_inputs(shape, "spread")
    t = torch.from_numpy(np.argmax(mask.numpy(), axis=1))[:, None]
    gen = torch.Generator().manual_seed(case_seed(N, K, HW, 99))
    b = torch.randint(-3, 4, (N, 1, HW), generator=gen).float()
    d = torch.randint(20, 28, (N, 1, HW), generator=gen).float()
    seg = torch.full((N, K, HW), -100.0).scatter_(1, (t + 1) % K, b + d).scatter_(1, t, b)
    mean = np.float64(float(d.double().sum())) * (np.float64(1.0) / (np.float64(N) * np.float64(HW)))
    return seg.contiguous(), mask, torch.tensor([np.float32(mean)])


CLIP_SCENARIOS = ["zero", "below", "above", "equal", "nonorm"]


def clip_inputs(n, scenario):
    """(x, max_norm as an fp32 number)."""
    gen = torch.Generator().manual_seed(case_seed(n, 3))
    x = torch.zeros(n) if scenario == "zero" else torch.randn(n, generator=gen)
    norm64 = float(clip_grad_norm(x, 1.0)[0])
    mx = {"zero": 9.0, "below": 2.0 * norm64, "above": norm64 / 7.0, "nonorm": norm64 / 7.0, "equal": norm64 + 1e-6}[scenario]
    return x, float(np.float32(mx))


def clip_rule(x, mx):
    """(reference norm, reference vector, e_ref, allowance) of the sum rule for the norm (all terms positive)."""
    ref_n, ref_v, _ = clip_grad_norm(x, mx)
    e_ref = abs(float(clip_grad_norm(x, mx, F32)[0]) - float(ref_n)) / max(float(ref_n), 1e-300)
    return ref_n, ref_v, e_ref, 4.0 * e_ref + 2.0 * U


def clip_exact_inputs(n):
    """The exact regime of the norm: every element is +-4, the square sum 16 n is exact in the kernel's fp64 partials and the norm
    is float32(sqrt(16 n)).  One element dropped or doubled moves the norm by 1/(2n): at least 4 units in the last place at 2^20."""
    gen = torch.Generator().manual_seed(case_seed(n, 4))
    x = (torch.randint(0, 2, (n,), generator=gen) * 8 - 4).float()
    return x, torch.tensor([np.float32(np.sqrt(np.float64(16.0 * n)))])


def edge_units(seg, lab, beta):
    """((prob, mag, edge_fg) errors of the fp32 restatement in units of U * magnitude, its angle error), the float64 reference."""
    ref, r32 = field_edges(seg, lab, beta), field_edges(seg, lab, beta, F32)
    return (units(r32["prob"], ref["prob"], ref["prob"]), units(r32["mag"], ref["mag"], ref["mag_m"]),
            units(r32["edge_fg"], ref["edge_fg"], ref["mag_m"].sum(1)), angle_error(seg, lab, beta, ref)), ref


@functools.lru_cache(maxsize=None)
def edge_calib(beta):
    """edge_units on the fixed draw EDGE_CALIB: the figures every field_edges case is judged by."""
    return edge_units(*edge_inputs(EDGE_CALIB, beta), beta)[0]


GATHER_GEO = [(0, 0, 0, 24, 24), (1, 3, 3, 24, 24), (1, 5, 4, 33, 27), (1, 1, 1, 8, 8)]      # (mode, h, w, H, W)
GATHER_CH = [4, 64, 65, 200, 1024]
GATHER_KML = [(2, 24), (21, 24), (24, 24)]
GATHER_NPTS = [1, 5, 400]


def gather_inputs(geo, CH, K, npts):
    """(dense, mask, pts) of a field_gather case, N = 2: points at the corners, on the last row and column, repeated."""
    mode, h, w, H, W = geo
    N = 2
    gen = torch.Generator().manual_seed(case_seed(mode, h, w, H, W, CH, K, npts))
    dense = torch.randn((N, CH, H, W) if mode == 0 else (N, h, w, CH), generator=gen) * 2.0
    return dense, torch.randn(N, K, H, W, generator=gen), field_points_for(N, H, W, npts, gen)


@functools.lru_cache(maxsize=None)
def gather_calib(mode):
    """(feat, mfeat) errors of the fp32 restatement on a fixed draw of 1024 points at CH = 256, K = 21 for the mode."""
    geo = GATHER_GEO[0] if mode == 0 else GATHER_GEO[2]
    dense, mask, pts = gather_inputs(geo, 256, 21, 1024)
    f, m = field_gather(dense, mode, mask, pts, 21, 24, geo[3], geo[4])
    f32, m32 = field_gather(dense, mode, mask, pts, 21, 24, geo[3], geo[4], F32)
    return units(f32, f, f), units(m32[:, :21], m[:, :21], m[:, :21])


def scatter_rule(h, w, CH, mode, gup):
    """Everything test_field_scatter_* compare with: inputs, reference, sum |term|, e_ref, allowance, the smallest share of a
    point, and `atomics` (mode 0: each of up to 40 atomic additions rounds at the running value, at most |base| + sum |term|)."""
    feat, gfeat, pts, base, N, H, W, shape = scatter_inputs(h, w, CH, mode)
    g32 = float(torch.tensor(gup if gup is not None else 1.0, dtype=F32))
    ref, mag = field_scatter(feat, gfeat, pts, mode, shape, g32, H, W)
    e_ref, rel = sum_rule(field_scatter(feat, gfeat, pts, mode, shape, g32, H, W, F32)[0], ref, mag)
    return dict(feat=feat, gfeat=gfeat, pts=pts, base=base, N=N, H=H, W=W, shape=shape, ref=ref, mag=mag, e_ref=e_ref, rel=rel,
                share=scatter_point_share(feat, gfeat, pts, mode, shape, g32, H, W), atomics=40.0 * U if mode == 0 else 0.0)


def scatter_gup(hw, ch, mode):
    """gup NULL and 0.37 alternate over the cases."""
    return None if (hw + ch) % 2 else 0.37


ROW_R = [1, 3, 5, 32768 + 5]          # the last: 8192 workgroups x 4 waves cover 32 768 rows in a sweep
ROW_C = [1, 21, 64, 65, 200]
ROW_EPS = 1e-5


def row_inputs(Rn, C):
    """(x with every third row zero from three rows on, gy)."""
    gen = torch.Generator().manual_seed(case_seed(Rn, C))
    x = torch.randn(Rn, C, generator=gen)
    if Rn >= 3:
        x[1::3] = 0.0
    return x, torch.randn(Rn, C, generator=gen)


def row_norm_rule(x):
    """(e_ref, allowance) of the sum rule for the row norms."""
    rn = row_l2norm(x, ROW_EPS)[1]
    e_ref = float(((row_l2norm(x, ROW_EPS, F32)[1].double() - rn).abs() / rn.clamp_min(1e-300)).max())
    return e_ref, 4.0 * e_ref + 2.0 * U


def row_dot_rule(x, gy):
    """(e_ref, allowance) of the sum rule for the row dot products gy.x, relative to sum |gy x|."""
    dot, dmag = (gy.double() * x.double()).sum(1), (gy.double() * x.double()).abs().sum(1)
    e_ref = float((((gy * x).sum(1).double() - dot).abs() / dmag.clamp_min(1e-300)).max())
    return e_ref, 4.0 * e_ref + 2.0 * U
