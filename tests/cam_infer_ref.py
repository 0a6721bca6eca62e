"""Plain restatements of the CAM inference kernels at the bottom of muscle_amd/csrc/head.hip (infer_accum_kernel,
cam_infer_kernel, infer_norm_kernel behind mx_infer_accum, mx_cam_infer, mx_infer_norm), in torch and numpy on the CPU, with
the case tables of tests/test_gpu_cam_infer_kernels.py; tests/test_cpu_cam_infer_ref.py checks the restatements against
independent statements of the same operations and the input conditions the GPU cases rely on.

As in tests/dec_ref.py: a function that takes `dtype` gives the reference at float64 and the plain fp32 restatement at float32
(the same expressions, every operation rounded to fp32), and returns (value, magnitude): the magnitude is the same expression
with absolute values, and one rounding error is at most U = 2^-24 of it.

The bound of one pass (two bilinear blends, the model's align_corners one to Hs x Ws and the script's half-pixel one to H x W):
  2 * BLEND_OPS * U * magnitude        the roundings of the two blends (a blend of the first stage's errors is at most their
                                       largest, a blend of |tap| is the magnitude),
  + U * ac_slope_units                 the first stage's coordinate: dec_ref.bil_slope_units of the low-resolution channel,
  + U * hp_slope_units                 the second stage's coordinate (d+0.5)*(in/out) - 0.5: three roundings of a number of at
                                       most `in`, so at most 3U*in source pixels, times the largest neighbour difference of the
                                       float64 intermediate Hs x Ws map along that axis (the value is piecewise linear and
                                       continuous, across the clamps too).
Over passes the bounds add, and the sequential fp32 sum of the per-pass values (table order, from 0.f) is allowed by the sum
rule of dec_ref.sum_rule, its e_ref measured on that summation alone (the float64 per-pass values rounded to fp32 and added in
fp32); a single pass adds to 0.f exactly and gets no such allowance.  Nothing here is taken from a kernel's output.
"""
import functools

import numpy as np
import torch

from dec_ref import BLEND_OPS, F32, F64, GRID_CAP, U, bil_slope_units, case_seed, sum_rule

NAN = float("nan")


# ---- the two coordinate rules ---------------------------------------------------------------------------------------------------
def _taps(s, n_in, dtype):
    i0 = s.floor().long().clamp(max=n_in - 1)
    i1 = (i0 + 1).clamp(max=n_in - 1)
    return i0, i1, s - i0.to(dtype)


def ac_scale(n_out, n_in, dtype=F64):
    return (torch.tensor(float(n_in - 1), dtype=dtype) / torch.tensor(float(n_out - 1), dtype=dtype)) if n_out > 1 \
        else torch.tensor(0.0, dtype=dtype)


def ac_coords(n_out, n_in, dtype=F64):
    """align_corners=True (bil_coord): s = d * (in-1)/(out-1), 0 when out == 1.  Returns (i0, i1, weight of i1)."""
    return _taps(ac_scale(n_out, n_in, dtype) * torch.arange(n_out, dtype=dtype), n_in, dtype)


def hp_source(n_out, n_in, dtype=F64):
    """The half-pixel source coordinate before its clamp at 0: (d + 0.5) * (in/out) - 0.5."""
    ratio = torch.tensor(float(n_in), dtype=dtype) / torch.tensor(float(n_out), dtype=dtype)
    return (torch.arange(n_out, dtype=dtype) + 0.5) * ratio - 0.5


def hp_coords(n_out, n_in, dtype=F64):
    """Half-pixel centres (hp_coord; cv2.resize INTER_LINEAR, torch align_corners=False): s = max((d+0.5)*in/out - 0.5, 0)."""
    return _taps(hp_source(n_out, n_in, dtype).clamp_min(0.0), n_in, dtype)


def _flip(v, W):
    return v.flip(-1)


RULES = dict(ac=ac_coords, hp=hp_coords, flip=_flip)


def _blend(a, cy, cx):
    """a [C,h,w] at the taps cy, cx: along x inside a row first, then the rows (the order of bil_lr and of the kernels' blend)."""
    (y0, y1, fy), (x0, x1, fx) = cy, cx
    r = (1.0 - fx) * a[:, :, x0] + fx * a[:, :, x1]
    return (1.0 - fy)[:, None] * r[:, y0] + fy[:, None] * r[:, y1]


def pass_term(src, K, Hs, Ws, H, W, flip, dtype=F64, rules=RULES):
    """One pass: src [h,w,lds] -> (value [K-1,H,W] of channels 1..K-1, the same blend of |src|, the intermediate [K-1,Hs,Ws])."""
    a = src[..., 1:K].permute(2, 0, 1).to(dtype)
    h, w = a.shape[1:]
    cy, cx = rules["ac"](Hs, h, dtype), rules["ac"](Ws, w, dtype)
    inter, inter_m = _blend(a, cy, cx), _blend(a.abs(), cy, cx)
    hy, hx = rules["hp"](H, Hs, dtype), rules["hp"](W, Ws, dtype)
    v, m = _blend(inter, hy, hx), _blend(inter_m, hy, hx)
    if flip:
        v, m = rules["flip"](v, W), rules["flip"](m, W)
    return v, m, inter


def accum(passes, K, H, W, dtype=F64, rules=RULES):
    """passes: [(src [h,w,lds], Hs, Ws, flip)].  The sum over passes in table order and its magnitude, [K-1,H,W]."""
    s, m = 0, 0
    for src, Hs, Ws, flip in passes:
        v, vm, _ = pass_term(src, K, Hs, Ws, H, W, flip, dtype, rules)
        s, m = s + v, m + vm
    return s, m


def ac_slope_units(src, K, Hs, Ws):
    """[K-1]: dec_ref.bil_slope_units of each low-resolution channel 1..K-1 of src [h,w,lds] as it stands."""
    return torch.tensor([bil_slope_units(src[None, :, :, k:k + 1], Hs, Ws) for k in range(1, K)], dtype=F64)


def hp_slope_units(inter, H, W):
    """[C]: the coordinate term of the half-pixel stage per channel of the float64 intermediate [C,Hs,Ws], per unit U."""
    inter = inter.double()
    C, Hs, Ws = inter.shape
    dy = (inter[:, 1:] - inter[:, :-1]).abs().amax((1, 2)) if Hs > 1 else torch.zeros(C, dtype=F64)
    dx = (inter[:, :, 1:] - inter[:, :, :-1]).abs().amax((1, 2)) if Ws > 1 else torch.zeros(C, dtype=F64)
    return 3.0 * Hs * dy + 3.0 * Ws * dx


def accum_rule(passes, K, H, W):
    """Everything a comparison with accum needs, over all K-1 channels: ref, mag [K-1,H,W]; allowed (units of U * mag: the blends
    and the sum over passes); extra [K-1,1,1] (absolute, per unit U: the slope terms of every pass); e_sum (the fp32 summation's
    own error, relative to mag)."""
    ref, mag, extra, seq = 0, 0, torch.zeros(K - 1, dtype=F64), None
    for src, Hs, Ws, flip in passes:
        v, vm, inter = pass_term(src, K, Hs, Ws, H, W, flip)
        ref, mag = ref + v, mag + vm
        extra += ac_slope_units(src, K, Hs, Ws) + hp_slope_units(inter, H, W)
        seq = v.float() if seq is None else seq + v.float()
    e_sum, rel = sum_rule(seq, ref, mag) if len(passes) > 1 else (0.0, 0.0)
    return dict(ref=ref, mag=mag, allowed=2.0 * BLEND_OPS + rel / U, extra=extra[:, None, None], e_sum=e_sum)


def tolerance(rule, sel=None):
    """The absolute tolerance tensor of accum_rule's figures (for the channels `sel`)."""
    mag, extra = (rule["mag"], rule["extra"]) if sel is None else (rule["mag"][sel], rule["extra"][sel])
    return rule["allowed"] * U * mag + extra * U


def worst_units(x, ref, tol, allowed):
    """The largest share an error has of its tolerance, times `allowed`: the figure dec_gpu_util.check_elementwise records."""
    err = (x.double() - ref.double()).abs()
    return float((err / tol.clamp_min(1e-300)).max()) * allowed if err.numel() else 0.0


# ---- the normalisation ------------------------------------------------------------------------------------------------------------
EPS32 = np.float32(1e-6)          # the kernel's 1e-6f
NORM_OPS = 5                      # v - mn, - 1e-6; mx - mn, + 1e-6 (relative to a sum of positives, so to the quotient); the division


def norm(acc32, cont=None, eps=float(EPS32)):
    """acc32 [C, ...] fp32.  Per channel v = max(a, 0), mn / mx of v, zero what is < mn + 1e-6, (v - mn - 1e-6)/(mx - mn + 1e-6).
    The discrete step is exact: the inputs are fp32, so are mn and mx, and lo = mn + 1e-6f is ONE fp32 addition - it is made in
    numpy float32 arithmetic here; everything after it is float64 (with the value of float32(1e-6) for the constant).
    cont (float64, same shape): the continuous values come from it instead (the decisions still from acc32); eps: the constant of
    the float64 part (the script's own 1e-6 for a comparison with its float64 statement).
    Returns (value, magnitude (|v| + |mn| + 1e-6)/den, zeroed mask, (mn, mx)) with the shape of acc32."""
    a = np.asarray(acc32)
    assert a.dtype == np.float32
    shape = a.shape
    a = a.reshape(shape[0], -1)
    v32 = np.maximum(a, np.float32(0.0))
    lo = v32.min(1) + EPS32                                   # float32 + float32: one rounded addition
    assert lo.dtype == np.float32
    zeroed = v32 < lo[:, None]
    c = v32.astype(np.float64) if cont is None else np.maximum(np.asarray(cont, dtype=np.float64).reshape(a.shape), 0.0)
    mn, mx = c.min(1)[:, None], c.max(1)[:, None]
    v = np.where(zeroed, 0.0, c)
    den = mx - mn + eps
    return ((v - mn - eps) / den).reshape(shape), ((np.abs(v) + np.abs(mn) + eps) / den).reshape(shape), zeroed.reshape(shape), \
        (mn[:, 0], mx[:, 0])


def norm32(acc32):
    """The kernel's own fp32 evaluation, operation for operation in numpy float32 (no product in it, so nothing to contract)."""
    a = np.asarray(acc32)
    shape = a.shape
    v = np.maximum(a.reshape(shape[0], -1), np.float32(0.0))
    mn, mx = v.min(1)[:, None], v.max(1)[:, None]
    lo, den = mn + EPS32, mx - mn + EPS32
    v = np.where(v < lo, np.float32(0.0), v)
    out = (v - mn - EPS32) / den
    assert out.dtype == np.float32
    return out.reshape(shape)


# ---- case tables ------------------------------------------------------------------------------------------------------------------
# (h, w, Hs, Ws, H, W) and what each is there for (checked by tests/test_cpu_cam_infer_ref.py on the fp32 coordinates)
GEOMS = [(1, 1, 16, 16, 9, 7), (1, 5, 1, 80, 3, 33), (4, 1, 64, 1, 31, 1), (6, 6, 96, 96, 1, 1), (5, 7, 75, 100, 75, 100),
         (3, 4, 38, 50, 75, 100), (10, 13, 150, 200, 75, 100), (7, 5, 100, 75, 53, 91), (7, 5, 100, 75, 53, 90)]
GEOM_CLAIMS = {
    (1, 1, 16, 16, 9, 7): {"one_pixel_map"},
    (1, 5, 1, 80, 3, 33): {"ac_out1"},
    (4, 1, 64, 1, 31, 1): {"one_column"},
    (6, 6, 96, 96, 1, 1): {"single_output"},
    (5, 7, 75, 100, 75, 100): {"hp_identity"},
    (3, 4, 38, 50, 75, 100): {"hp_lo_clamp", "hp_hi_clamp"},
    (10, 13, 150, 200, 75, 100): {"hp_down2"},
    (7, 5, 100, 75, 53, 91): {"w_odd"},
    (7, 5, 100, 75, 53, 90): {"w_even"},
}
# (K, lds, keep): five full chunks of four; one channel; three; unsorted with a repeat and a tail chunk of one; K == lds with a
# tail chunk of three; the small paddings
CHANNELS = [(21, 24, tuple(range(20))), (21, 24, (11,)), (21, 24, (2, 7, 14)), (21, 24, (19, 0, 7, 7, 3)),
            (24, 24, tuple(range(23))), (5, 8, (3, 1)), (2, 4, (0,))]
CAM_CH = 4                                                   # channels per thread of cam_infer_kernel (head.hip)
TAIL_CHUNKS = [c for c in CHANNELS if len(c[2]) > CAM_CH and len(c[2]) % CAM_CH]
KLDS = sorted({c[:2] for c in CHANNELS})                     # every (K, lds) of the table: what mx_infer_accum runs
# (h, w, Hs, Ws, flip) rows for a 75 x 100 image, K = 21, lds = 24: infer_mcl.py's scales 0.5, 1, 1.5, 2, each plain then flipped;
# h, w = the 1/16 map of efficientnet-b0 without the last pooling (what cam="cam_lr" returns) for that Hs x Ws
SCRIPT_HW = (75, 100)
SCRIPT_SIZES = [(2, 3, 38, 50), (4, 6, 75, 100), (7, 9, 112, 150), (9, 12, 150, 200)]
SCRIPT_TABLE = [s + (f,) for s in SCRIPT_SIZES for f in (0, 1)]
# two passes that differ in every field, to a 29 x 41 image
TWO_PASS_HW = (29, 41)
TWO_PASS_TABLE = [(3, 5, 40, 30, 0), (6, 2, 17, 90, 1)]
MULTI = {"script": (SCRIPT_TABLE, SCRIPT_HW), "two_pass": (TWO_PASS_TABLE, TWO_PASS_HW)}
MULTI_KEEPS = [tuple(range(20)), (19, 0, 7, 7, 3), (11,)]   # K = 21, lds = 24
# one channel of 1449 x 1449 = 2 099 601 pixels: above the 8192 x 256 threads of one sweep in both kernels
ABOVE_CAP = dict(K=2, lds=4, keep=(0,), geom=(3, 4, 40, 40, 1449, 1449), flip=1)


def lr_maps(h, w, K, lds, *seed):
    """(CAM, SGC) low-resolution maps [h,w,lds]: unit-variance noise, NOT smoothed (a rough map is what shows a coordinate
    error); channel 0 and the padding columns K..lds-1 hold NaN: a kernel that reads them poisons its output."""
    gen = torch.Generator().manual_seed(case_seed(h, w, K, lds, *seed))
    out = []
    for _ in range(2):
        m = torch.randn(h, w, lds, generator=gen)
        m[..., 0] = NAN
        m[..., K:] = NAN
        out.append(m.contiguous())
    return tuple(out)


def base_for(K, H, W, *seed):
    """The non-zero starting content of an accumulator [K-1,H,W]."""
    gen = torch.Generator().manual_seed(case_seed(K, H, W, 77, *seed))
    return torch.randn(K - 1, H, W, generator=gen)


@functools.lru_cache(maxsize=16)
def table_case(rows, HW, K, lds):
    """rows: a tuple of (h, w, Hs, Ws, flip).  Returns dict(cam, sgc: the passes' maps; rule_cam, rule_sgc: accum_rule over all
    K-1 channels; w_cam, w_sgc: the fp32 restatement's sums).  Cached: the GPU tests and the CPU checks share one evaluation,
    which nobody modifies."""
    H, W = HW
    maps = [lr_maps(h, w, K, lds, Hs, Ws, flip, n) for n, (h, w, Hs, Ws, flip) in enumerate(rows)]
    out = dict(rows=rows, H=H, W=W, K=K, lds=lds, cam=[m[0] for m in maps], sgc=[m[1] for m in maps])
    for which in ("cam", "sgc"):
        passes = [(m, r[2], r[3], r[4]) for m, r in zip(out[which], rows)]
        out["rule_" + which] = accum_rule(passes, K, H, W)
        out["w_" + which] = accum(passes, K, H, W, F32)[0]
    return out


def single_case(geom, flip, K, lds):
    h, w, Hs, Ws, H, W = geom
    return table_case(((h, w, Hs, Ws, flip),), (H, W), K, lds)


def witness_units(case, which, sel=None):
    """The fp32 restatement against float64 in the figure the GPU tests record for the kernel (share of the tolerance x allowed)."""
    rule = case["rule_" + which]
    idx = slice(None) if sel is None else list(sel)
    return worst_units(case["w_" + which][idx], rule["ref"][idx], tolerance(rule, idx), rule["allowed"])


# ---- the normalisation's inputs ---------------------------------------------------------------------------------------------------
NORM_HW = [1, 63, 64, 255, 256, 257, 1000, 75 * 100]
NORM_KINDS = ["spread", "positive", "edge", "negative", "constant", "ext_last", "ext_wave4"]
EDGE_MN = np.float32(0.75)


def wave4_index(HW):
    """The largest index that a thread of the fourth wave (threadIdx 192..255 of 256) serves, short of the last element; None if
    there is none."""
    for i in range(HW - 2, -1, -1):
        if i % 256 >= 192:
            return i
    return None


def edge_values(mn):
    """(lo, [one fp32 step below lo, lo itself, one step above, two steps above]) for lo = mn + 1e-6f in fp32."""
    lo = np.float32(mn) + EPS32
    inf = np.float32(np.inf)
    up1 = np.nextafter(lo, inf)
    return lo, [np.nextafter(lo, -inf), lo, up1, np.nextafter(up1, inf)]


def norm_channel(kind, HW):
    """One channel [HW] fp32 of the kind.  Below 8 elements the kinds keep what fits (HW = 1: a single value)."""
    gen = torch.Generator().manual_seed(case_seed(HW, NORM_KINDS.index(kind), 5))
    r = torch.rand(HW, generator=gen).numpy().astype(np.float32)
    g = torch.randn(HW, generator=gen).numpy().astype(np.float32)
    w4 = wave4_index(HW)
    if kind == "spread":                          # negatives to clamp: mn = 0, lo = 1e-6f; values at the edge of that lo too
        a = g * np.float32(2.0)
        a[0] = np.float32(-1.5)
        a[1:5] = edge_values(0.0)[1][:max(min(4, HW - 1), 0)]
        a[HW - 1] = np.float32(7.0) if HW > 1 else a[0]
    elif kind == "positive":                      # all positive, a unique minimum
        a = r * np.float32(3.0) + np.float32(1.0)
        a[HW // 2] = np.float32(0.5)
    elif kind == "edge":                          # the minimum three times, the edge values of lo = mn + 1e-6f by construction
        a = r * np.float32(2.0) + EDGE_MN + np.float32(0.01)
        a[[0, HW // 3, HW - 1]] = EDGE_MN
        for i, v in zip(range(1, HW - 1), edge_values(EDGE_MN)[1]):
            a[i] = v
    elif kind == "negative":
        a = -r - np.float32(0.1)
    elif kind == "constant":
        a = np.full(HW, 2.5, np.float32)
    else:                                         # unique extremes in the last element and at the fourth wave's index
        a = r + np.float32(1.0)
        i_mx, i_mn = (HW - 1, w4) if kind == "ext_last" else (w4, HW - 1)
        if i_mn is not None:
            a[i_mn] = np.float32(0.25)
        if i_mx is not None:
            a[i_mx] = np.float32(9.0)
    return np.ascontiguousarray(a, dtype=np.float32)


@functools.lru_cache(maxsize=None)
def norm_case(HW):
    """All kinds in one launch: [len(NORM_KINDS), HW] fp32 and norm() of it."""
    a = np.stack([norm_channel(k, HW) for k in NORM_KINDS])
    a.setflags(write=False)
    return a, norm(a)
