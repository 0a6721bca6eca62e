"""Plain restatements of every operation of muscle_amd/csrc/bn.hip, in torch, for tests/test_gpu_bn_kernels.py.

Each function follows the formula in the comment above its kernel and the reference semantics cited at the top of bn.hip
(nn.BatchNorm2d(momentum=0.01, eps=1e-3), MemoryEfficientSwish, the SE gate, drop_connect + skip).  Tensors are [rows, C]
activation matrices; per-sample operands are [N] or [N, C] with sample n = row // rows_per_sample.

Every function takes `dtype`: float64 gives the reference, float32 gives the "plain fp32 restatement" whose own error against
float64 calibrates the tolerances (the same expressions, every operation rounded to fp32, torch's own `.sum`).  Every function
returns (value, magnitude).  The magnitude of an elementwise result is the same expression with absolute values (the sigmoid is
positive and keeps its signed argument); the magnitude of a sum is sum |term| per output.  A rounding error of one operation is
at most 2^-24 of the magnitude of its result, so tolerances are stated in units of 2^-24 * magnitude.
"""
import torch
import torch.nn.functional as F

U = 2.0 ** -24          # unit round-off of fp32


def _c(t, dtype):
    return None if t is None else t.to(dtype)


def sample_of_row(rows, rps, device):
    return torch.arange(rows, device=device) // rps


def swish(z):
    return z * torch.sigmoid(z)


def swish_mag(z, m):
    """|z * sigmoid(z)| with |z| replaced by its magnitude m >= |z|."""
    return m * torch.sigmoid(z)


def swish_grad(z):
    s = torch.sigmoid(z)
    return s * (1.0 + z * (1.0 - s))


def swish_grad_mag(z, m):
    s = torch.sigmoid(z)
    return s * (1.0 + m * (1.0 - s))


def g_eff(G, X, rps, *, rs=None, gate=None, add=None, a=None, b=None, dtype=torch.float64):
    """Effective upstream gradient (struct GEff): g = G; g *= rs[n]; g = g*gate[n,c] + add[n,c]; g *= swish'(a*X + b)."""
    G, X, rs, gate, add, a, b = (_c(t, dtype) for t in (G, X, rs, gate, add, a, b))
    n = sample_of_row(X.shape[0], rps, X.device)
    g, m = G, G.abs()
    if rs is not None:
        g = g * rs[n][:, None]
        m = m * rs[n].abs()[:, None]
    if gate is not None:
        g = g * gate[n] + add[n]
        m = m * gate[n].abs() + add[n].abs()
    if a is not None:
        z = a * X + b
        g = g * swish_grad(z)
        m = m * swish_grad_mag(z, a.abs() * X.abs() + b.abs())
    return g, m


def bn_apply(P, sc, sh, rps, *, rs=None, R=None, gate=None, act=False, dtype=torch.float64):
    """out = (sc[c]*P + sh[c]) [swish] [* gate[n,c]] [* rs[n]] [+ R]   (bn_apply_kernel)."""
    P, sc, sh, rs, R, gate = (_c(t, dtype) for t in (P, sc, sh, rs, R, gate))
    n = sample_of_row(P.shape[0], rps, P.device)
    v = sc * P + sh
    m = sc.abs() * P.abs() + sh.abs()
    if act:
        v, m = swish(v), swish_mag(v, m)
    if gate is not None:
        v, m = v * gate[n], m * gate[n].abs()
    if rs is not None:
        v, m = v * rs[n][:, None], m * rs[n].abs()[:, None]
    if R is not None:
        v, m = v + R, m + R.abs()
    return v, m


def bn_bwd_apply(G, X, rps, c, *, dtype=torch.float64, **opts):
    """out = c1[c]*g_eff + c2[c]*X + c3[c]   (bn_bwd_apply_kernel); c is [3, C]."""
    g, m = g_eff(G, X, rps, dtype=dtype, **opts)
    c = _c(c, dtype)
    x = _c(X, dtype)
    return c[0] * g + c[1] * x + c[2], c[0].abs() * m + c[1].abs() * x.abs() + c[2].abs()


def colstats(X, *, dtype=torch.float64):
    """[2, C]: sum x, sum x^2 over the rows   (FStats)."""
    x = _c(X, dtype)
    return torch.stack([x.sum(0), (x * x).sum(0)]), torch.stack([x.abs().sum(0), (x * x).sum(0)])


def bn_bwd_reduce(G, X, rps, *, dtype=torch.float64, **opts):
    """[2, C]: sum g_eff, sum g_eff * x over the rows   (FBwdReduce)."""
    g, m = g_eff(G, X, rps, dtype=dtype, **opts)
    x = _c(X, dtype)
    return torch.stack([g.sum(0), (g * x).sum(0)]), torch.stack([m.sum(0), (m * x.abs()).sum(0)])


def pool_sum(X, rps, *, G=None, a=None, b=None, act=False, dtype=torch.float64):
    """[N, C]: sum over a sample's rows of f(X), f = [a*x + b] [swish] [* G]   (FPool)."""
    X, G, a, b = (_c(t, dtype) for t in (X, G, a, b))
    v, m = X, X.abs()
    if a is not None:
        v, m = a * X + b, a.abs() * X.abs() + b.abs()
    if act:
        v, m = swish(v), swish_mag(v, m)
    if G is not None:
        v, m = v * G, m * G.abs()
    C = X.shape[1]
    return v.view(-1, rps, C).sum(1), m.view(-1, rps, C).sum(1)


def se_bn1_pool(dA, X, a, b, rps, *, dtype=torch.float64):
    """[5, N, C] per (sample, channel), z = a*x + b, act = swish(z), s' = swish'(z)   (se_bn1_pool_kernel):
    sum dA*act, sum dA*s', sum s', sum dA*s'*x, sum s'*x."""
    dA, X, a, b = (_c(t, dtype) for t in (dA, X, a, b))
    C = X.shape[1]
    z = a * X + b
    sg = torch.sigmoid(z)
    act = z * sg
    sp = sg * (1.0 + z * (1.0 - sg))
    del z, sg
    out, mag = [], []
    for term in (lambda: dA * act, lambda: dA * sp, lambda: sp, lambda: dA * sp * X, lambda: sp * X):
        t = term()
        out.append(t.view(-1, rps, C).sum(1))
        mag.append(t.abs().view(-1, rps, C).sum(1))
    return torch.stack(out), torch.stack(mag)


def bn_bwd_coeffs(s0, s1, count, gamma, mean, rstd, training):
    """(dgamma, dbeta, c [3, C]) from the two backward sums   (bn_bwd_finalize_one); float64."""
    gm, m, r = gamma.double(), mean.double(), rstd.double()
    dg = r * (s1 - m * s0)
    c1 = gm * r
    if training:
        k = gm * r * r * (dg / count)
        c = torch.stack([c1, -k, -gm * r * (s0 / count) + k * m])
    else:
        c = torch.stack([c1, torch.zeros_like(c1), torch.zeros_like(c1)])
    return dg, s0, c


def bn_backward_autograd(G, X, gamma, beta, running_mean, running_var, eps, training, act=False):
    """Full BatchNorm backward from torch autograd of F.batch_norm on float64: y = BN(X) [swish], upstream gradient G.
    Returns ((dX, dgamma, dbeta), (their magnitudes)).  Magnitudes: with r the rstd in use, g' = G [* swish'(y)] and
    xh = (|x| + mean|x|) * r (the normalised input with the cancellation of x - mean unravelled; mean|x| >= |mean|),
      dbeta: sum |g'|      dgamma: sum |g'| * xh      dX (training): |gamma| r (|g'| + mean|g'| + xh * mean(|g'| * xh))
      dX (eval): |gamma| r |g'|."""
    x = X.double().requires_grad_(True)
    w = gamma.detach().double().requires_grad_(True)
    bb = beta.detach().double().requires_grad_(True)
    rm, rv = running_mean.double().clone(), running_var.double().clone()
    y = F.batch_norm(x, None if training else rm, None if training else rv, w, bb, training, 0.0, eps)
    out = swish(y) if act else y
    out.backward(G.double())
    with torch.no_grad():
        xd = x.detach()
        if training:
            r = 1.0 / torch.sqrt(xd.var(0, unbiased=False) + eps)
        else:
            r = 1.0 / torch.sqrt(rv + eps)
        gp = G.double().abs()
        if act:
            yd = y.detach()
            gp = gp * swish_grad_mag(yd, yd.abs())
        xh = (xd.abs() + xd.abs().mean(0)) * r
        m_dbeta = gp.sum(0)
        m_dgamma = (gp * xh).sum(0)
        if training:
            m_dx = w.detach().abs() * r * (gp + gp.mean(0) + xh * (gp * xh).mean(0))
        else:
            m_dx = w.detach().abs() * r * gp
    return (x.grad, w.grad, bb.grad), (m_dx, m_dgamma, m_dbeta)


def fold_block(We, bn0, bn1, Wp, bn2, *, dtype=torch.float64):
    """Eval-mode BatchNorm folded into one block's 1x1 convolutions (fold_block_kernel), s_k = gamma_k / sqrt(var_k + eps_k):
    We_f = We * s0[row], be = beta0 - s0*mean0, s1, t1 = beta1 - s1*mean1, Wp_f = Wp * s2[row], bp = beta2 - s2*mean2.
    bn_k = (gamma, beta, running_mean, running_var, eps).  Returns (values, magnitudes) as dicts; the magnitude of a bias is
    |beta| + |s*mean|."""
    def st(bn):
        g, b, m, v, eps = bn
        g, b, m, v = (_c(t.detach(), dtype) for t in (g, b, m, v))
        s = g * torch.rsqrt(v + eps)
        return s, b - s * m, b.abs() + (s * m).abs()
    out, mag = {}, {}
    if We is not None:
        s0, out["be"], mag["be"] = st(bn0)
        out["We"] = _c(We.detach(), dtype) * s0[:, None]
        mag["We"] = out["We"].abs()
    out["s1"], out["t1"], mag["t1"] = st(bn1)
    mag["s1"] = out["s1"].abs()
    s2, out["bp"], mag["bp"] = st(bn2)
    out["Wp"] = _c(Wp.detach(), dtype) * s2[:, None]
    mag["Wp"] = out["Wp"].abs()
    return out, mag
