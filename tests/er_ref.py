"""CPU references for the equivariant-regularisation (ER) top-k loss kernels of muscle_amd/csrc/losses.hip.

select_oracle is the exact oracle of the three-pass radix select: it works on the bit patterns of the fp32 values the
kernels histogram, so threshold, remaining count, tie count and the 2^36 fixed-point sum above the threshold are integers
that a correct kernel reproduces exactly.  The value / gradient references restate the loss expression (train_mcl.py:175-188,
with the bilinear upsample of MuSCLe.py:256-257 for the low-resolution path) in torch on the CPU, fp64 by default; the same
functions evaluated in fp32 give the round-off a plain fp32 implementation has, which the GPU tests scale their gradient
bound by.  Nothing here touches a GPU.
"""
import numpy as np
import torch
import torch.nn.functional as F

from oracle import mcl_oracle as O

FIX_SCALE = 2.0 ** 36          # ER_FIX_SCALE of losses.hip


def select_oracle(d_row_f32, k):
    """The select of one row of non-negative fp32 values: tau_bits = uint32 pattern of the k-th largest value (exact zeros
    rank last, so tau_bits = 0 once k exceeds the non-zero count), krem = k - #(bits > tau_bits), cnt_eq = #(bits == tau_bits),
    sum_gt_fix = sum of uint64(trunc(v * 2^36)) over bits > tau_bits (v * 2^36 is exact in fp32)."""
    v = np.ascontiguousarray(d_row_f32, dtype=np.float32).reshape(-1)
    bits = v.view(np.uint32)
    assert not (bits >> np.uint32(31)).any(), "select_oracle: rows are |.| * mask, no sign bits"
    k = int(k)
    assert 1 <= k <= bits.size
    nz = bits[bits != 0]
    tau_bits = 0 if k > nz.size else int(np.partition(nz, nz.size - k)[nz.size - k])
    gt = bits > np.uint32(tau_bits)
    fix = (v[gt] * np.float32(FIX_SCALE)).astype(np.uint64)
    return {"tau_bits": tau_bits, "krem": k - int(gt.sum()), "cnt_eq": int((bits == np.uint32(tau_bits)).sum()),
            "sum_gt_fix": int(fix.sum(dtype=np.uint64))}


def tau_of(o):
    return float(np.array([o["tau_bits"]], dtype=np.uint32).view(np.float32)[0])


def row_topk_sum(o):
    """Top-k sum of one row from its oracle, in fp64: sum_gt_fix * 2^-36 + krem * tau (the header's formula)."""
    return float(o["sum_gt_fix"]) / FIX_SCALE + float(o["krem"]) * tau_of(o)


def select_loss(rows_f32, k):
    """(fp32 loss, per-row oracles) of rows [N, row_len]: sum_n(top-k sum of row n) / (N k) in fp64, rounded to fp32."""
    os_ = [select_oracle(r, k) for r in rows_f32]
    acc = 0.0
    for o in os_:
        acc += row_topk_sum(o)
    return np.float32(acc / (len(os_) * int(k))), os_


def select_weights(rows_f32, oracles):
    """The fixed weights of the gradient reference: 1 above tau, krem / cnt_eq at tau, 0 below; with tau == 0 every
    non-zero value has weight 1 (and the zeros, whose gradient vanishes, 0)."""
    rows = np.ascontiguousarray(rows_f32, dtype=np.float32)
    bits = rows.view(np.uint32)
    w = np.zeros(rows.shape, dtype=np.float64)
    for n, o in enumerate(oracles):
        t = np.uint32(o["tau_bits"])
        w[n][bits[n] > t] = 1.0
        if o["tau_bits"] != 0:
            w[n][bits[n] == t] = o["krem"] / o["cnt_eq"]
    return w


def _t(a, dtype):
    return (a if torch.is_tensor(a) else torch.from_numpy(np.asarray(a))).to(dtype)


def er_values_ref(cams, sgcs, lwb, dtype=torch.float64):
    """|softmaxnorm(cams) - softmaxnorm(sgcs)| * m on NCHW raw maps, [N, K, H, W]."""
    m = _t(lwb, dtype)
    return (O.cam_softmaxnorm(_t(cams, dtype)) - O.cam_softmaxnorm(_t(sgcs, dtype))).abs() * m[:, :, None, None]


def upsample_lr(x_lr, K, H, W, dtype=torch.float64):
    """MuSCLe.py:256-257 on the first K channels of an NHWC low-resolution map [N, h, w, L] -> NCHW [N, K, H, W]."""
    x = _t(x_lr, dtype)[..., :K].permute(0, 3, 1, 2)
    return F.interpolate(x, (H, W), mode="bilinear", align_corners=True)


def er_values_lr_ref(cam_lr, sgc_lr, lwb, K, H, W, dtype=torch.float64):
    return er_values_ref(upsample_lr(cam_lr, K, H, W, dtype), upsample_lr(sgc_lr, K, H, W, dtype), lwb, dtype)


def er_grad_ref(cams, sgcs, lwb, w, k, lr=None, dtype=torch.float64):
    """autograd of sum(w * values) / (N k) w.r.t. sgcs; lr = (K, H, W) takes cams / sgcs as low-resolution NHWC maps.
    w [N, K, H, W] are fixed weights (select_weights)."""
    s = _t(sgcs, dtype).clone().requires_grad_()
    v = er_values_lr_ref(cams, s, lwb, *lr, dtype=dtype) if lr is not None else er_values_ref(cams, s, lwb, dtype)
    ((v * _t(w, dtype).reshape(v.shape)).sum() / (v.shape[0] * int(k))).backward()
    return s.grad.detach()


def min_small_diff(cams, sgcs, lwb, lr=None):
    """Input condition of the GPU cases, from fp64 alone: the smallest non-zero active-class |a - b| (below 1e-6 an fp32 sign
    can differ from the fp64 one).  Returns inf when every active value is zero."""
    v = er_values_lr_ref(cams, sgcs, lwb, *lr) if lr is not None else er_values_ref(cams, sgcs, lwb)
    nz = v[v > 0]
    return float(nz.min()) if nz.numel() else float("inf")


def tie_k(row_f32, lo, odd=False):
    """The smallest k >= lo whose threshold sits on a tie that has to be shared: the k-th and (k+1)-th largest fp32 values of
    the row are equal and the (k-1)-th is larger, so 0 < krem = 1 < cnt_eq."""
    bits = np.ascontiguousarray(row_f32, dtype=np.float32).reshape(-1).view(np.uint32)
    s = np.sort(bits[bits != 0])[::-1]
    ks = np.nonzero((s[1:-1] == s[2:]) & (s[:-2] != s[1:-1]))[0] + 2
    ks = ks[(ks >= lo) & ((ks % 2 == 1) | (not odd))]
    assert ks.size, "no shared tie in this row"
    return int(ks[0])


def free_k(row_f32, lo):
    """The smallest k >= lo whose threshold value occurs once in the row (cnt_eq = 1), or None if there is none."""
    bits = np.ascontiguousarray(row_f32, dtype=np.float32).reshape(-1).view(np.uint32)
    s = np.sort(bits[bits != 0])[::-1]
    ks = np.nonzero((s[1:-1] != s[2:]) & (s[:-2] != s[1:-1]))[0] + 2
    ks = ks[ks >= lo]
    return int(ks[0]) if ks.size else None
