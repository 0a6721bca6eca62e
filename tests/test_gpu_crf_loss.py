"""The dense-CRF energy loss on the GPU (muscle_amd.crf_loss / mx_crf_loss_fwd, mx_crf_loss_bwd) against the numpy restatement of
its model in crf_loss_ref.py: loss, the messages [M | Z] and the gradient, per case; batch isolation, the closed forms, autograd
with a non-contiguous seg_map, run-to-run bits, the stager's "window" and muscle_step with the term on and off.

Tolerance, the convention of tests/test_gpu_crf.py: per case e32 is the error of the float32 restatement against the float64 one
for the same input (what fp32 rounding alone does to the model, reference arithmetic on the CPU) - absolute for the loss, max-abs
relative to the tensor's max-abs for M and gseg - and the kernel must stay within F_TOL * e32 + 1e-7.
F_TOL = 6 is twice the worst ratio err / e32 measured once on an MI355X over all cases below, rounded up (profiles/crf_loss_bench.txt
lists them); the kernels are deterministic, so the margin is for other inputs, not for noise.  The ratios (loss / M / gseg):
    f1_5x7_allpairs    0.16 / 1.91 / 0.48        f2_32x64_K2    0.50 / 1.74 / 1.00
    f2_lowres9x17_R3   1.00 / 2.53 / 1.21        f4_32x64_K21   1.00 / 1.24 / 0.85
    f1_lowres33x10_R3  0.42 / 2.34 / 0.99        f8_32x64_K24   1.00 / 1.46 / 1.00
M is the one above 1: its exponent goes through three fp32 roundings and v_exp_f32, numpy's float32 exp is correctly rounded.
A ratio of 1.00 for the loss means the kernel and the float32 restatement round to the same float32."""
import random

import numpy as np
import pytest
import torch

import crf_loss_ref as R

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
F_TOL = 6.0
FLOOR = 1e-7
G_UP = 0.37


def _image(g, N, H, W):
    """Blocks of colour with mild noise, as the normalised batch image: neighbouring cells are close in colour inside a block
    and far across an edge, so the bilateral kernel takes every value between 0 and 1."""
    base = g.integers(30, 226, (N, (H + 5) // 6, (W + 8) // 9, 3)).repeat(6, 1).repeat(9, 2)[:, :H, :W]
    u8 = np.clip(base + g.normal(0, 6, (N, H, W, 3)), 0, 255).astype(np.uint8)
    return R.color_norm(u8)


# name: (N, K, H, W, f, sxy, srgb, trunc, windows)
CASES = {
    # one ragged tile, all pairs, a window that covers everything
    "f1_5x7_allpairs": (1, 5, 5, 7, 1, 3.0, 20.0, 0.0, [(0, 0, 5, 7)]),
    # low resolution 9 x 17, R = 3: ragged tiles on both axes; a rectangle that cuts cells (fractional r)
    "f2_lowres9x17_R3": (2, 21, 18, 34, 2, 3.0, 15.0, 2.0, [(3, 5, 18, 31), (0, 0, 15, 34)]),
    # low resolution 33 x 10, R = 3: five tile rows, a window walk that starts mid-tile; one empty rectangle of three
    "f1_lowres33x10_R3": (3, 24, 33, 10, 1, 1.5, 25.0, 2.0, [(2, 1, 33, 10), (7, 4, 7, 9), (0, 0, 30, 7)]),
    "f2_32x64_K2": (2, 2, 32, 64, 2, 4.0, 15.0, 2.0, None),
    "f4_32x64_K21": (2, 21, 32, 64, 4, 8.0, 15.0, 2.0, [(1, 3, 30, 61), (5, 0, 32, 50)]),
    "f8_32x64_K24": (2, 24, 32, 64, 8, 12.0, 30.0, 2.0, [(0, 9, 29, 64), (3, 3, 32, 64)]),
    "all_empty": (2, 5, 8, 16, 2, 4.0, 15.0, 2.0, [(3, 5, 3, 9), (8, 0, 8, 0)]),
}
_IN, _REF = {}, {}


def _inputs(name):
    if name not in _IN:
        N, K, H, W, f, sxy, srgb, trunc, win = CASES[name]
        g = np.random.default_rng(sorted(CASES).index(name))
        seg = (g.normal(0, 2.5, (N, K, H, W)) + 3.0 * (g.integers(0, K, (N, 1, (H + 3) // 4, (W + 4) // 5)) == np.arange(K)[None, :, None, None])
               .repeat(4, 2).repeat(5, 3)[:, :, :H, :W]).astype(np.float32)
        window = None if win is None else np.array(win, np.int32)
        _IN[name] = (seg, _image(g, N, H, W), window, dict(f=f, sxy=sxy, srgb=srgb, trunc=trunc))
    return _IN[name]


def _refs(name):
    """(the float64 restatement, e32 per quantity) of a case, computed once."""
    if name not in _REF:
        seg, img, window, kw = _inputs(name)
        r64 = R.energy(seg, img, window, dtype=np.float64, g=G_UP, **kw)
        r32 = R.energy(seg, img, window, dtype=np.float32, g=G_UP, **kw)
        assert r32["M"].dtype == np.float32 and r32["gseg"].dtype == np.float32
        m64, m32 = (np.concatenate([r["M"], r["Z"][..., None]], -1) for r in (r64, r32))
        e32 = {"loss": abs(float(r32["loss"]) - float(r64["loss"])), "M": _rel(m32, m64), "gseg": _rel(r32["gseg"], r64["gseg"])}
        _REF[name] = (r64, m64, e32)
    return _REF[name]


def _rel(a, ref):
    scale = float(np.abs(ref).max())
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / scale if scale > 0 else float(np.abs(a).max())


def _gpu(seg, img, window, kw, g=G_UP):
    from muscle_amd import crf_loss as CL
    t = lambda a: None if a is None else torch.from_numpy(np.ascontiguousarray(a)).to(DEV)  # noqa: E731
    dseg, dwin = t(seg), t(window)
    loss, sums, M = CL.energy_forward(dseg, t(img), dwin, sxy=kw["sxy"], srgb=kw["srgb"], scale=kw["f"], trunc=kw["trunc"])
    gseg = CL.energy_backward(dseg, dwin, M, sums, torch.tensor([g], device=DEV), kw["f"])
    torch.cuda.synchronize()
    return loss.cpu().numpy(), sums.cpu().numpy(), M.cpu().numpy(), gseg.cpu().numpy()


@pytest.mark.parametrize("name", list(CASES))
def test_loss_messages_and_gradient_against_the_restatement(name):
    seg, img, window, kw = _inputs(name)
    r64, m64, e32 = _refs(name)
    K = seg.shape[1]
    loss, sums, M, gseg = _gpu(seg, img, window, kw)
    assert np.isfinite(loss).all() and np.isfinite(M).all() and np.isfinite(gseg).all()
    assert not M[..., K + 1:].any()                                         # the columns above r / Z stay zero
    err = {"loss": abs(float(loss[0]) - float(r64["loss"])), "M": _rel(M[..., :K + 1], m64), "gseg": _rel(gseg, r64["gseg"])}
    for k in err:
        print(f"crf_loss {name} {k}: err {err[k]:.3e} e32 {e32[k]:.3e} ratio {err[k] / e32[k] if e32[k] > 0 else float('nan'):.2f}")
    print(f"crf_loss {name} D: gpu {sums[0]:.9e} ref {float(r64['D']):.9e}")
    for k in err:
        assert err[k] <= F_TOL * e32[k] + FLOOR, (name, k, err[k], e32[k])
    if name == "all_empty":
        assert float(loss[0]) == 0.0 and sums[0] == 0.0 and not gseg.any()
    else:
        assert 0.0 < float(loss[0]) < 1.0
        outside = R.inside(window, *seg.shape[:1], *seg.shape[2:], np.float32) == 0
        assert not gseg[np.broadcast_to(outside[:, None], gseg.shape)].any()


def test_batch_items_do_not_see_each_other():
    """N = 3 with different windows, images and logits: each item's [M | Z] is that of the item run alone, bit for bit."""
    seg, img, window, kw = _inputs("f1_lowres33x10_R3")
    _, _, M, _ = _gpu(seg, img, window, kw)
    for n in range(3):
        _, _, m1, _ = _gpu(seg[n:n + 1], img[n:n + 1], window[n:n + 1], kw)
        assert np.array_equal(M[n], m1[0]), n
    assert not M[1].any() and M[0].any() and M[2].any()                     # the empty window sends nothing


@pytest.mark.parametrize("K,f", [(2, 1), (21, 4), (24, 8)])
def test_closed_forms(K, f):
    """A flat image and uniform logits: 1 - 1/K.  A confident constant one-hot map: 0 (its column is r's column, bit for bit)."""
    N, H, W = 2, 16, 48
    img = R.color_norm(np.full((N, H, W, 3), 120, np.uint8))
    window = np.array([(1, 2, 16, 45), (0, 0, 13, 48)], np.int32)
    kw = dict(f=f, sxy=2.0 * f, srgb=15.0, trunc=2.0)
    loss, _, _, _ = _gpu(np.full((N, K, H, W), 0.5, np.float32), img, window, kw)
    print("crf_loss uniform", K, f, float(loss[0]) - (1 - 1 / K))
    assert abs(float(loss[0]) - (1 - 1 / K)) <= 1e-6
    hot = np.zeros((N, K, H, W), np.float32)
    hot[:, 1] = 30.0
    img2 = _image(np.random.default_rng(7), N, H, W)
    loss, _, _, gseg = _gpu(hot, img2, window, kw)
    print("crf_loss one-hot", K, f, float(loss[0]))
    assert abs(float(loss[0])) < 1e-6 and np.abs(gseg).max() < 1e-6


def test_autograd_with_a_non_contiguous_seg_map():
    """DenseEnergyLoss through torch.autograd on a permuted view, upstream 0.37: the gradient of the restatement, and the bits of
    the direct backward call on the contiguous copy."""
    import muscle_amd
    name = "f4_32x64_K21"
    seg, img, window, kw = _inputs(name)
    r64, _, e32 = _refs(name)
    base = torch.from_numpy(np.ascontiguousarray(seg.transpose(0, 2, 3, 1))).to(DEV).requires_grad_(True)      # [N,H,W,K]
    view = base.permute(0, 3, 1, 2)
    assert not view.is_contiguous()
    crit = muscle_amd.DenseEnergyLoss(sxy=kw["sxy"], srgb=kw["srgb"], scale=kw["f"], trunc=kw["trunc"])
    loss = crit(view, torch.from_numpy(img).to(DEV), torch.from_numpy(window).to(DEV))
    assert loss.dim() == 0 and loss.is_cuda
    (G_UP * loss).backward()
    torch.cuda.synchronize()
    got = base.grad.permute(0, 3, 1, 2).cpu().numpy()
    l0, _, _, g0 = _gpu(seg, img, window, kw)
    assert float(loss.detach()) == float(l0[0]) and np.array_equal(got, g0)
    assert _rel(got, r64["gseg"]) <= F_TOL * e32["gseg"] + FLOOR


def test_two_runs_give_the_same_bits():
    for name in ("f2_lowres9x17_R3", "f4_32x64_K21"):
        a, b = _gpu(*_inputs(name)), _gpu(*_inputs(name))
        for x, y in zip(a, b):
            assert np.array_equal(x, y), name


STAGER_CASES = [(75, 101, 0.6, 0), (96, 73, 1.0, 1), (31, 23, 1.75, 1), (150, 131, 0.5, 0)]


def test_stager_adds_the_windows_and_changes_nothing_else():
    import label_ref as LR
    import segdata_ref as SR
    from muscle_amd import segdata as D
    S, dev = 96, torch.device(DEV)
    random.seed(23)
    torch.manual_seed(23)
    plans = []
    for i, (H, W, s, flip) in enumerate(STAGER_CASES):
        p = D.plan_label_item(SR.synth_image(H, W, 10 + i), LR.synth_label_map(H, W, 30 + i), s, s, S)
        p.flip = bool(flip)
        plans.append(p)
    labels = torch.zeros(4, 20)
    a = D.SegStager(dev, 4, S)(plans, labels=labels)
    b = D.SegStager(dev, 4, S, windows=True)(plans, labels=labels)
    torch.cuda.synchronize()
    assert set(a) == {"img", "mask", "label"} and set(b) == set(a) | {"window"}
    for k in a:
        assert torch.equal(a[k], b[k]), k
    win = b["window"]
    assert win.dtype == torch.int32 and win.shape == (4, 4) and win.is_cuda
    assert win.cpu().tolist() == [list(D.plan_window(p, S)) for p in plans]
    mask = b["mask"].cpu().numpy()
    for i, (y0, x0, y1, x1) in enumerate(win.cpu().tolist()):              # padding is 255 everywhere outside the window
        out = np.ones((S, S), bool)
        out[y0:y1, x0:x1] = False
        assert (mask[i][out] == 255).all()


# ---- step level: the smallest label batch of tests/test_gpu_label_path.py (B0 decoder, crop 64, batch 2) -------------------------
def _label_batch(n, S, soft=False):
    gen = torch.Generator().manual_seed(1000 * n + S)
    lab = torch.zeros(n, 20)
    mask = torch.zeros(n, S, S, dtype=torch.uint8)
    yy, xx = torch.meshgrid(torch.arange(S), torch.arange(S), indexing="ij")
    for i in range(n):
        c = 3 + 4 * i
        lab[i, c - 1] = 1
        mask[i][(yy - S // 2 + 5 * i) ** 2 + (xx - S // 3) ** 2 < (S // 4) ** 2] = c
        mask[i, :, S - 9:] = 255                                      # padding on the right, as a placed window leaves it
    window = torch.tensor([[0, 0, S, S - 9]] * n, dtype=torch.int32)
    if soft:
        m = torch.nn.functional.one_hot(mask.clamp(max=20).long(), 21).permute(0, 3, 1, 2).float() * (mask != 255)[:, None]
        mask = m.contiguous()
    return {"img": torch.randn(n, 3, S, S, generator=gen).to(DEV), "label": lab.to(DEV), "mask": mask.to(DEV), "window": window.to(DEV)}


def _step(batch, **kw):
    import muscle_amd
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(DEV)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-4, weight_decay=1e-5)
    torch.manual_seed(1)                                               # the drop_connect draws
    random.seed(5)
    out = muscle_amd.muscle_step(model, opt, batch, lamb=0.0, step=7, k=8, **kw)
    torch.cuda.synchronize()
    return out, torch.cat([p.detach().reshape(-1) for p in model.parameters()]).cpu()


@pytest.mark.both_arith
def test_muscle_step_with_the_energy_term_off_and_on():
    import muscle_amd
    batch = _label_batch(2, 64)
    crit = muscle_amd.DenseEnergyLoss(sxy=16.0, srgb=60.0, scale=4, trunc=2.0)
    (plain, p0), (off, p1), (on, p2) = _step(batch), _step(batch, energy=crit, energy_weight=0.0), _step(batch, energy=crit, energy_weight=1.0)
    assert set(plain) == set(off) == {"loss_seg", "loss_beacon", "grad_norm"}
    assert torch.equal(p0, p1) and float(plain["loss_seg"]) == float(off["loss_seg"])
    assert set(on) == set(plain) | {"loss_energy"}
    e, gn = float(on["loss_energy"].detach()), float(on["grad_norm"])
    print("crf_loss muscle_step loss_energy", e, "grad_norm", gn, "without", float(off["grad_norm"]))
    assert np.isfinite(e) and 0.0 < e < 1.0 and np.isfinite(gn) and gn > 0
    assert float(on["loss_seg"]) == float(off["loss_seg"])                 # the forward is the same; the gradient is not
    assert not torch.equal(p1, p2) and bool(torch.isfinite(p2).all())


def test_muscle_step_with_the_energy_term_on_a_soft_mask():
    import muscle_amd
    batch = _label_batch(2, 64, soft=True)
    del batch["window"]                                                    # no window: the whole container counts
    out, p = _step(batch, energy=muscle_amd.DenseEnergyLoss(sxy=16.0, srgb=60.0, scale=2), energy_weight=0.5)
    e = float(out["loss_energy"].detach())
    assert 0.0 < e < 1.0 and np.isfinite(float(out["grad_norm"])) and bool(torch.isfinite(p).all())
