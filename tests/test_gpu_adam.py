"""mx_adam (muscle_amd/csrc/losses.hip) against the float64 closed form, and FusedAdam against torch.optim.Adam on float64 copies.

The bound on a parameter after a step, accumulated over steps (tests/phase2_ref.py, AdamClosedForm):
    |err| <= 8 * 2^-23 * lr + 2^-24 * |p|
a few ulps on an update of size at most about lr, plus the rounding of p.  Measured on an MI355X: at most 0.89 of the bound for
the raw kernel and 0.81 for FusedAdam (the rounding of p itself takes up to the whole second term).  FusedAdam meets it because
its bias corrections use the betas as the kernel receives them, rounded to float; formed from the unrounded 0.999 the first
steps miss the bound seven times over (1 - float(0.999) is 1.3e-5 short of 1 - 0.999).  ADAM_FIGURES=<file> appends the maxima.
"""
import os

import pytest
import torch

import phase2_ref as R

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
CANARY = -777.25
TAIL = 8
BIG = 8192 * 1024 + 1029          # a second grid-stride sweep (8192 workgroups x 1024 elements) and a scalar tail


def fig(name, value, bound):
    path = os.environ.get("ADAM_FIGURES")
    if path:
        with open(path, "a") as f:
            f.write(f"{name}\t{value:.3e}\t{bound}\n")


def _grad(n, g):
    x = torch.randn(n, generator=g)
    x[::5] = 0.0
    x[1::11] = 1e-20
    return x


RAW = [(n, wd, dyn) for n in (1, 3, 4, 5, 1023, 1025) for wd in (0.0, 5e-5) for dyn in (False, True)] + [(BIG, 5e-5, False)]


@pytest.mark.parametrize("n,wd,dyn", RAW, ids=lambda v: str(v))
def test_mx_adam_closed_form(n, wd, dyn):
    """Three steps carrying m and v; gradients with exact zeros and 1e-20; sentinels behind element n - 1."""
    from muscle_amd._lib import call, ptr, stream
    g_ = torch.Generator().manual_seed(n % 9973 + int(dyn))
    lr, b1, b2, eps = 1e-3, 0.9, 0.999, 1e-8
    p0 = torch.randn(n, generator=g_) * 0.05
    p0[::7] = 0.0
    ref = R.AdamClosedForm(p0, lr, b1, b2, eps, wd)
    bufs = [torch.full((n + TAIL,), CANARY, device=DEV) for _ in range(3)]
    p, m, v = bufs
    p[:n] = p0.to(DEV)
    m[:n] = 0
    v[:n] = 0
    worst = 0.0
    for t in range(3):
        g = _grad(n, g_)
        bc1, bc2s = ref.scalars()
        d_g = g.to(DEV)
        if dyn:      # the kernel reads {lr, bc1, bc2s} from the device and must ignore the arguments
            d_dyn = torch.tensor([lr, bc1, bc2s], dtype=torch.float32, device=DEV)
            call("mx_adam", ptr(p), ptr(d_g), ptr(m), ptr(v), n, 123.0, b1, b2, eps, wd, 0.5, 0.5, ptr(d_dyn), stream())
        else:
            call("mx_adam", ptr(p), ptr(d_g), ptr(m), ptr(v), n, lr, b1, b2, eps, wd, bc1, bc2s, None, stream())
        ref.step(g, bc1, bc2s)
        for name, got, want, allow in (("p", p, ref.p, ref.ep), ("m", m, ref.m, ref.em), ("v", v, ref.v, ref.ev)):
            err = (got[:n].cpu().double() - want).abs()
            assert bool(torch.isfinite(err).all())
            ratio = float((err / allow.clamp_min(1e-300)).max())
            if name == "p":
                worst = max(worst, ratio)
            assert bool((err <= allow).all()), (name, t, ratio)
            assert bool((got[n:] == CANARY).all()), f"{name}: written past element {n - 1}"
    fig(f"mx_adam n={n} wd={wd} dyn={dyn}", worst, "share of the bound")


# ---- FusedAdam against torch.optim.Adam -----------------------------------------------------------------------------------------
SHAPES = [(1,), (3,), (4,), (5,), (7, 3), (1030,), (6,)]      # the last one never has a gradient
NEVER, SOMETIMES, ODD = 6, 2, 3                               # SOMETIMES: gradient at steps 1 and 3 only; ODD: a view at element offset 1
STEPS, LR, LR3, WD = 4, 1e-3, 4e-4, 5e-5


def _run_fused(layout, pad=0.0):
    """layout 'separate': every gradient its own tensor, parameter ODD's a contiguous view at element offset 1 of a larger one.
    layout 'flat': views of one buffer, each parameter at the next multiple of 4, the padding filled with `pad`."""
    import muscle_amd
    g_ = torch.Generator().manual_seed(17)
    init = [torch.randn(s, generator=g_) * (0.05 if i % 2 else 1.0) for i, s in enumerate(SHAPES)]
    init[4][0] = 0.0
    ps = [torch.nn.Parameter(w.clone().to(DEV)) for w in init]
    rs = [torch.nn.Parameter(w.clone().double()) for w in init]
    opt = muscle_amd.FusedAdam(ps, lr=LR, weight_decay=WD)
    ropt = torch.optim.Adam(rs, lr=LR, weight_decay=WD)
    allow = [torch.zeros_like(r) for r in rs]
    gmax = [0.0] * len(ps)                                    # the largest |g| + wd |p| a parameter has met: the size of the moments' terms
    worst = 0.0
    for step in range(1, STEPS + 1):
        lr = LR if step < 3 else LR3
        for o in (opt, ropt):
            o.param_groups[0]["lr"] = lr
        live = [i for i in range(len(ps)) if i != NEVER and (i != SOMETIMES or step in (1, 3))]
        grads = [torch.randn(s, generator=g_) for s in SHAPES]
        grads[5][::5] = 0.0
        sizes = [(p.numel() + 3) // 4 * 4 for p in ps]
        flat = torch.full((sum(sizes),), pad, device=DEV)
        off = 0
        for i, (p, r) in enumerate(zip(ps, rs)):
            p.grad, r.grad = None, None
            if i in live:
                if layout == "flat":
                    p.grad = flat[off:off + p.numel()].view(p.shape)
                elif i == ODD:
                    p.grad = torch.zeros(p.numel() + 3, device=DEV)[1:1 + p.numel()].view(p.shape)
                    assert p.grad.is_contiguous() and p.grad.data_ptr() % 16 == 4
                else:
                    p.grad = torch.empty(p.shape, device=DEV)
                p.grad.copy_(grads[i])
                r.grad = grads[i].double()
                gmax[i] = max(gmax[i], float(grads[i].abs().max()) + WD * float(r.detach().abs().max()))
            off += sizes[i]
        before = [p.detach().clone() for p in ps]
        opt.step()
        ropt.step()
        for i, (p, r) in enumerate(zip(ps, rs)):
            if i not in live:
                assert torch.equal(p.detach(), before[i]), "a parameter without a gradient moved"
                continue
            allow[i] = allow[i] + 8 * 2.0 ** -23 * lr + 2.0 ** -24 * r.detach().abs()
            err = (p.detach().cpu().double() - r.detach()).abs()
            worst = max(worst, float((err / allow[i]).max()))
            assert bool((err <= allow[i]).all()), (layout, step, i, float((err / allow[i]).max()))
    fig(f"FusedAdam {layout} pad={pad}", worst, "share of the bound")
    return ps, rs, opt, ropt, gmax


def _check_state(opt, ropt, rs, gmax):
    """Moments against torch's.  Per step one fp32 evaluation, 5 (m) and 8 (v) roundings of a term's size (AdamClosedForm); the
    kernel's betas are floats, off by at most 2^-25, which moves the weights (1 - b) b^k of at most STEPS terms by 10 * 2^-25 in sum."""
    sd = opt.state_dict()["state"]
    assert NEVER not in sd and len(ropt.state.get(rs[NEVER], {})) == 0
    for i, r in enumerate(rs):
        if i == NEVER:
            continue
        st = ropt.state[r]
        assert sd[i]["step"] == int(st["step"]) == (2 if i == SOMETIMES else STEPS)
        m, v = sd[i]["exp_avg"].cpu().double(), sd[i]["exp_avg_sq"].cpu().double()
        assert m.shape == r.shape and v.shape == r.shape
        assert float((m - st["exp_avg"]).abs().max()) <= (STEPS * 5 + 5) * 2.0 ** -24 * gmax[i]
        assert float((v - st["exp_avg_sq"]).abs().max()) <= (STEPS * 8 + 5) * 2.0 ** -24 * gmax[i] ** 2


def test_fused_adam_separate_gradients():
    ps, rs, opt, ropt, gmax = _run_fused("separate")
    _check_state(opt, ropt, rs, gmax)
    assert torch.equal(ps[NEVER].detach().cpu().double(), rs[NEVER].detach())


def test_fused_adam_flat_gradients_and_padding():
    a = _run_fused("flat", 0.0)
    b = _run_fused("flat", 1.0)
    _check_state(a[2], a[3], a[1], a[4])
    for pa, pb in zip(a[0], b[0]):
        assert torch.equal(pa.detach().view(torch.int32), pb.detach().view(torch.int32)), "the padding's gradient reached a parameter"
    sa, sb = a[2].state_dict()["state"], b[2].state_dict()["state"]
    for i in sa:
        assert torch.equal(sa[i]["exp_avg"], sb[i]["exp_avg"]) and torch.equal(sa[i]["exp_avg_sq"], sb[i]["exp_avg_sq"])
