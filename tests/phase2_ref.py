"""Plain float64 restatements of the phase-2 operations (muscle_amd/csrc/phase2.hip) and of Adam (mx_adam), for the unit tests
of tests/test_gpu_phase2_kernels.py and tests/test_gpu_adam.py.  Everything runs on the CPU; gradients come from torch autograd.
tests/test_cpu_phase2_ref.py checks these restatements against the oracle's own get_dynamic_crops / emd_dynamic.

Conventions of the kernels that the references share:
  packed crops   [pixels, 24] rows, 21 (K) classes then zero columns; a crop of rh x rw pixels occupies rows off .. off + rh*rw
  resize table   {n, y0, x0, lh, lw, rh, rw, off} per crop;  pool table {in_off, h, w, out_off};  pair table {x_off, n1, y_off, n2, sample, rank}
"""
import math

import numpy as np
import torch
import torch.nn.functional as F

from oracle import mcl_oracle as O

FP = 24
EMD_ITERS = 10
EMD_REG = 0.1


def f64(t):
    return torch.as_tensor(t).detach().to("cpu", torch.float64)


# ---- cam_maxnorm ----------------------------------------------------------------------------------------------------------------
def maxnorm(x, g=None):
    """(y, dx): oracle.cam_maxnorm on float64 and its autograd against the upstream gradient g."""
    x = f64(x).clone().requires_grad_()
    y = O.cam_maxnorm(x)
    if g is None:
        return y.detach(), None
    y.backward(f64(g))
    return y.detach(), x.grad


# ---- PixPro ---------------------------------------------------------------------------------------------------------------------
def pixpro(f1, f2, c1, c2, mask=None):
    """(loss, d loss / d f1) of oracle.pixpro on float64, both maps multiplied by the [N,K] mask first.
    A sample with an empty window has no pixel to average: the reference project's mean of nothing is NaN there, the kernel
    defines the sample's term as 0 (pixpro_finish_kernel skips cnt == 0) and leaves its gradient zero.  The restatement follows
    the kernel: the oracle runs on the samples with pixels and the mean over the batch still divides by N."""
    f1 = f64(f1).clone().requires_grad_()
    f2 = f64(f2)
    a, b = f1, f2
    if mask is not None:
        m = f64(mask)[:, :, None, None]
        a, b = a * m, b * m
    c1, c2 = torch.as_tensor(c1).long(), torch.as_tensor(c2).long()
    live = [n for n in range(f1.shape[0]) if int(c1[n, 2]) * int(c1[n, 3]) > 0]
    loss = 1 - (1 - O.pixpro(a[live], b[live], c1[live], c2[live])) * len(live) / f1.shape[0]
    loss.backward()
    return loss.detach(), f1.grad


# ---- F.normalize(dim=1) ---------------------------------------------------------------------------------------------------------
def chan_norm(x, g=None):
    x = f64(x).clone().requires_grad_()
    y = F.normalize(x, dim=1)
    if g is None:
        return y.detach(), None
    y.backward(f64(g))
    return y.detach(), x.grad


# ---- crops ----------------------------------------------------------------------------------------------------------------------
def table_total(table):
    return max(t[7] + t[5] * t[6] for t in table)


def _crop(x, t):
    n, y0, x0, lh, lw, rh, rw, _ = t
    return F.interpolate(x[n:n + 1, :, y0:y0 + lh, x0:x0 + lw], (rh, rw), mode="bilinear", align_corners=True)


def pack(crop):
    """[1,K,h,w] -> [h*w, 24] with zero columns for k >= K."""
    K = crop.shape[1]
    return F.pad(crop.reshape(K, -1).t(), (0, FP - K))


def crop_resize(x, table, total=None):
    """Packed rows [total, 24] of every crop of the table; rows no crop names stay zero."""
    x = f64(x) if not x.requires_grad else x
    out = torch.zeros(total if total is not None else table_total(table), FP, dtype=torch.float64)
    parts = [(t[7], pack(_crop(x, t))) for t in table]
    for off, p in parts:
        out = torch.cat([out[:off], p, out[off + p.shape[0]:]])       # (no in-place write: autograd follows)
    return out


def crop_resize_adjoint(shape, table, gout):
    """d <crop_resize(x), gout> / dx accumulated over all rows of the table (overlapping crops add)."""
    x = torch.zeros(shape, dtype=torch.float64, requires_grad=True)
    tot = 0
    for t in table:
        tot = tot + (pack(_crop(x, t)) * f64(gout)[t[7]:t[7] + t[5] * t[6]]).sum()
    tot.backward()
    return x.grad


def unpack(rows, h, w):
    """[h*w, 24] -> [1, 24, h, w]."""
    return rows.t().reshape(1, FP, h, w)


def avgpool4(rows, h, w, g=None):
    """(pooled rows [(h//4)*(w//4), 24], gradient rows [h*w, 24] against g) of F.avg_pool2d(4, 4) on a packed crop."""
    x = unpack(f64(rows), h, w).clone().requires_grad_()
    y = F.avg_pool2d(x, 4, 4)
    out = y.detach().reshape(FP, -1).t()
    if g is None:
        return out, None
    y.backward(unpack(f64(g), h // 4, w // 4))
    return out, x.grad.reshape(FP, -1).t()


def packed_dynamic_crops(x1, coord1, x2, coord2, geometry):
    """get_dynamic_crops out of crop_resize / avgpool4 alone: ([crops of view 1 per sample], [crops of view 2], batch indices),
    every crop [1,K,h,w].  The enumeration is the oracle's (torchutils.py:217-291); the values come from the packed references."""
    K = x1.shape[1]
    c1s, c2s, bidx = [], [], []
    for b in range(x1.shape[0]):
        h, w = int(coord1[b, 2]), int(coord1[b, 3])
        g = geometry[b]
        if g is None:
            continue
        lh, lw, sh, sw = g
        rh, rw = round(h / (h / sh)), round(w / (w / sw))
        t1 = [[b, int(coord1[b, 0]) + i, int(coord1[b, 1]) + j, lh, lw, rh, rw, 0]
              for i in range(0, h, sh) for j in range(0, w, sw) if i + lh <= h and j + lw <= w and rh >= 7 and rw >= 7]
        t2 = [[b, int(coord2[b, 0]) + i, int(coord2[b, 1]) + j, min(h // 2, h - i), min(w // 2, w - j)] for i in range(0, h - 1, h // 2)
              for j in range(0, w - 1, w // 2)]
        t2 = [[*t, t[3], t[4], 0] for t in t2]
        if not t1:
            continue
        out = []
        for x, tab, pool_all in ((x1, t1, False), (x2, t2, True)):
            crops = []
            for t in tab:
                rows, (ph, pw) = crop_resize(x, [t]), (t[5], t[6])
                if pool_all or ph > 28 or pw > 28:
                    rows, (ph, pw) = avgpool4(rows, ph, pw)[0], (ph // 4, pw // 4)
                crops.append(unpack(rows, ph, pw)[:, :K])
            out.append(crops)
        c1s.append(out[0]); c2s.append(out[1]); bidx.append(b)
    return c1s, c2s, bidx


# ---- Sinkhorn EMD ---------------------------------------------------------------------------------------------------------------
def emd_features(n, seed, K=21):
    """[n, 24] float32: non-negative (rand), L2-normalised rows, zero columns for k >= K."""
    g = torch.Generator().manual_seed(seed)
    x = F.normalize(torch.rand(n, K, generator=g, dtype=torch.float64), dim=1)
    return F.pad(x, (0, FP - K)).float()


def emd_weights(x, y):
    x, y = f64(x), f64(y)
    return x @ y.mean(0), y @ x.mean(0)


def sinkhorn_states(cost, mu, nu, reg=EMD_REG, maxiter=EMD_ITERS):
    """The maxiter + 1 states (u_t, v_t) of oracle.sinkhorn_logsumexp, same expressions."""
    u, v = 0.0 * mu, 0.0 * nu
    states = [(u, v)]
    for _ in range(maxiter):
        m = (-cost + u.unsqueeze(1) + v.unsqueeze(0)) / reg
        u, v = (reg * (torch.log(mu + 1e-6) - torch.logsumexp(m, dim=1)) + u,
                reg * (torch.log(nu + 1e-6) - torch.logsumexp(m.t(), dim=1)) + v)
        states.append((u, v))
    return states


def emd_pair(x, y, grad=True):
    """(score, d score / dx [n1,24], trajectory [11, n1+n2]) of one pair: cost 1 - x y^T, detached weights, gradient through the
    cost and with respect to x only (oracle.emd_dynamic)."""
    x = f64(x).clone().requires_grad_(grad)
    y = f64(y)
    w1, w2 = emd_weights(x, y)
    assert float(w1.min()) > 0 and float(w2.min()) > 0, "weights must be positive: log(mu + 1e-6) is finite"
    cost = 1 - x @ y.t()
    score = O.sinkhorn_logsumexp(cost, w1.detach(), w2.detach())
    gx = None
    if grad:
        score.backward()
        gx = x.grad
    with torch.no_grad():
        traj = torch.stack([torch.cat(s) for s in sinkhorn_states(cost.detach(), w1.detach(), w2.detach())])
    return score.detach(), gx, traj


# Pair tables of the GPU test, (n1, n2) per pair.  tests/test_cpu_phase2_ref.py states which path of the kernels each one takes
# (slice counts, empty slices, unroll remainders, LDS or global x) and checks that against the kernels' own arithmetic.
EMD_SINGLE = [(1, 1), (1, 49), (49, 1), (3, 5), (5, 3), (49, 272), (63, 64), (64, 65), (65, 63), (512, 7), (513, 7), (1024, 16),
              (16, 1024)]
EMD_FWD_LDS_GRAD_XG = [(625, 784), (729, 729)]          # scores from LDS, gradient with x in global memory
EMD_MIXED_XG = [(700, 784), (3, 5), (49, 1)]            # one table: the long pair makes the short ones run the XG kernels too


def emd_table(sizes):
    """(pair rows {x_off, n1, y_off, n2, sample, rank}, total pixels): every pair its own sample, crops packed back to back."""
    rows, off = [], 0
    for s, (n1, n2) in enumerate(sizes):
        rows.append([off, n1, off + n1, n2, s, s])
        off += n1 + n2
    return rows, off


# ---- Adam -----------------------------------------------------------------------------------------------------------------------
U24 = 2.0 ** -24


def f32(x):
    """The float the kernel receives for a scalar argument, as a Python float."""
    return float(np.float32(x))


class AdamClosedForm:
    """mx_adam in float64 on the float32 arguments the kernel receives (every scalar rounded to float first), with the error
    allowances of one fp32 evaluation carried along:
      p   8 * 2^-23 * lr + 2^-24 * |p| per step (a few ulps on an update of size about lr, plus the rounding of p), accumulated;
      m   5U * (b1 |m| + (1 - b1)(|g| + wd |p|)) per step: gr two roundings, each product one, the sum one; earlier error decays by b1;
      v   8U * (b2 v + (1 - b2)(|g| + wd |p|)^2) per step, plus 2^-125 for a result in the denormal range (kept or flushed).
    """

    def __init__(self, p, lr, b1=0.9, b2=0.999, eps=1e-8, wd=0.0):
        self.p = f64(p).clone()
        self.m, self.v = torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.ep, self.em, self.ev = torch.zeros_like(self.p), torch.zeros_like(self.p), torch.zeros_like(self.p)
        self.lr, self.b1, self.b2, self.eps, self.wd = f32(lr), f32(b1), f32(b2), f32(eps), f32(wd)
        self.t = 0

    def scalars(self):
        """(bias_corr1, sqrt_bias_corr2) of the NEXT step as FusedAdam forms them: in double, from the betas the kernel receives."""
        t = self.t + 1
        return 1.0 - self.b1 ** t, math.sqrt(1.0 - self.b2 ** t)

    def step(self, g, bc1, bc2s):
        g = f64(g)
        bc1, bc2s = f32(bc1), f32(bc2s)
        self.t += 1
        mag = g.abs() + self.wd * self.p.abs()
        gr = g + self.wd * self.p
        self.em = self.b1 * self.em + 5 * U24 * (self.b1 * self.m.abs() + (1 - self.b1) * mag)
        self.ev = self.b2 * self.ev + 8 * U24 * (self.b2 * self.v + (1 - self.b2) * mag * mag) + 2.0 ** -125
        self.m = self.b1 * self.m + (1 - self.b1) * gr
        self.v = self.b2 * self.v + (1 - self.b2) * gr * gr
        self.p = self.p - (self.lr / bc1) * self.m / (self.v.sqrt() / bc2s + self.eps)
        self.ep = self.ep + 8 * 2.0 ** -23 * self.lr + U24 * self.p.abs()
