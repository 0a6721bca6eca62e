"""Host side of the dense-CRF energy loss (muscle_amd/crf_loss.py): the numpy restatement tests/crf_loss_ref.py against central
differences and its closed forms in float64, E >= 0, `segdata.plan_window` against the footprint of a staged label map, and the
ABI declared in include/muscle_hip.h.  Nothing here needs a GPU."""
import random

import numpy as np
import pytest
import torch

import crf_loss_ref as R
import label_ref as LR
import segdata_ref as SR


def _case(seed, N, K, H, W, spread=2.0):
    g = np.random.default_rng(seed)
    seg = g.normal(0, spread, (N, K, H, W))
    u8 = g.integers(0, 256, (N, H, W, 3)).astype(np.uint8)
    return seg, R.color_norm(u8)


def test_gradient_against_central_differences():
    """N=2, K=3, 4 x 6, f=2, a window that cuts cells (fractional r) and one that leaves a whole item row out."""
    seg, img = _case(0, 2, 3, 4, 6)
    window = np.array([[1, 1, 4, 5], [0, 0, 3, 6]], np.int32)
    kw = dict(window=window, f=2, sxy=3.0, srgb=60.0, trunc=2.0)
    ref = R.energy(seg, img, g=0.37, **kw)
    assert 0 < ref["loss"] < 1 and np.abs(ref["gseg"]).max() > 1e-4
    eps, worst = 1e-5, 0.0
    for idx in np.ndindex(*seg.shape):
        a, b = seg.copy(), seg.copy()
        a[idx] += eps
        b[idx] -= eps
        num = 0.37 * (R.energy(a, img, **kw)["loss"] - R.energy(b, img, **kw)["loss"]) / (2 * eps)
        worst = max(worst, abs(num - ref["gseg"][idx]))
    assert worst < 1e-9, worst                                              # O(eps^2) truncation + 1e-16 / eps cancellation
    outside = R.inside(window, 2, 4, 6, np.float64) == 0
    assert (ref["gseg"][np.broadcast_to(outside[:, None], seg.shape)] == 0).all()


@pytest.mark.parametrize("K", [2, 5, 21])
@pytest.mark.parametrize("f", [1, 2])
def test_closed_forms(K, f):
    """Uniform logits: every S_c = r / K, so the loss is exactly 1 - 1/K whatever image and window.  A constant, confident
    one-hot map: S_1 = r up to exp(-60), loss 0."""
    _, img = _case(K, 2, K, 8, 12)
    window = np.array([[0, 1, 7, 12], [2, 0, 8, 9]], np.int32)
    kw = dict(window=window, f=f, sxy=4.0, srgb=40.0, trunc=1.5)
    flat = R.energy(np.full((2, K, 8, 12), 0.25), img, **kw)
    assert abs(flat["loss"] - (1 - 1 / K)) < 1e-12
    hot = np.zeros((2, K, 8, 12))
    hot[:, 1] = 60.0
    conf = R.energy(hot, img, **kw)
    assert abs(conf["loss"]) < 1e-12 and np.abs(conf["gseg"]).max() < 1e-12


def test_energy_is_not_negative_and_below_one():
    for seed in range(6):
        N, K, f = 1 + seed % 3, 2 + 3 * seed, (1, 2, 4)[seed % 3]
        seg, img = _case(10 + seed, N, K, 8, 16, spread=4.0)
        window = None if seed % 2 else np.array([[1, 2, 7, 15]] * N, np.int32)
        out = R.energy(seg, img, window=window, f=f, sxy=6.0, srgb=30.0, trunc=0.0 if seed == 3 else 2.0)
        assert out["D"] > 0 and -1e-15 <= out["loss"] <= 1.0
        assert (out["Z"][..., None] * out["r"][..., None] + 1e-15 >= np.moveaxis(out["S"], 1, -1) * out["M"]).all()


def test_all_windows_empty():
    seg, img = _case(3, 2, 4, 4, 8)
    out = R.energy(seg, img, window=np.array([[2, 3, 2, 8], [4, 0, 4, 0]], np.int32), f=2)
    assert out["loss"] == 0 and out["D"] == 0 and not out["gseg"].any()


STAGER_CASES = [(75, 101, 0.6, 0), (96, 73, 1.0, 1), (31, 23, 1.75, 1), (150, 131, 0.5, 0), (40, 200, 1.0, 1)]


@pytest.mark.parametrize("kind", ["label", "soft"])
def test_plan_window_is_the_footprint_of_the_staged_label(kind):
    """An all-zero label map staged by the numpy restatement of mx_label_stage differs from 255 exactly inside plan_window, for
    flipped and unflipped plans, windows smaller than the container in either axis and larger than it; a soft plan of the same
    draws has the same window."""
    from muscle_amd import segdata as D
    S, partial = 96, 0
    for i, (H, W, s, flip) in enumerate(STAGER_CASES):
        random.seed(40 + i)
        torch.manual_seed(40 + i)
        im = SR.synth_image(H, W, 10 + i)
        p = D.plan_label_item(im, np.zeros((H, W), np.uint8), s, s, S)
        p.flip = bool(flip)
        staged = LR.plan_label_cpu(p, S)
        y0, x0, y1, x1 = D.plan_window(p, S)
        foot = np.zeros((S, S), bool)
        foot[y0:y1, x0:x1] = True
        assert np.array_equal(staged != 255, foot), (i, (y0, x0, y1, x1))
        assert 0 <= y0 < y1 <= S and 0 <= x0 < x1 <= S
        assert np.array_equal(foot, SR.window(SR.plan_as_draws(p), S))
        partial += int(not foot.all())
        if kind == "soft":
            random.seed(40 + i)
            torch.manual_seed(40 + i)
            q = D.plan_seg_item(im, SR.synth_label(H, W, 50 + i), s, s, S)
            q.flip = bool(flip)
            assert D.plan_window(q, S) == (y0, x0, y1, x1)
    assert partial >= 3


def test_abi_and_exports():
    from muscle_amd import _lib
    import muscle_amd
    sigs = _lib.parse_header()
    assert sigs["mx_crf_loss_ws"] == "iiiii" and "mx_crf_loss_ws" in _lib.LONG_RETURNS
    assert sigs["mx_crf_loss_fwd"] == "pppiiiiifffppppp"
    assert sigs["mx_crf_loss_bwd"] == "pppppiiiiipp"
    assert muscle_amd.DenseEnergyLoss is muscle_amd.crf_loss.DenseEnergyLoss
    with pytest.raises(ValueError):
        muscle_amd.DenseEnergyLoss(scale=3)
    loss = muscle_amd.DenseEnergyLoss()
    assert (loss.sxy, loss.srgb, loss.scale, loss.trunc) == (80.0, 15.0, 4, 2.0)
    for seg, img, win in ((torch.zeros(1, 1, 8, 8), torch.zeros(1, 3, 8, 8), None),           # K = 1
                          (torch.zeros(1, 25, 8, 8), torch.zeros(1, 3, 8, 8), None),          # K = 25
                          (torch.zeros(1, 3, 8, 6), torch.zeros(1, 3, 8, 6), None),           # W % 4
                          (torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 4), None),           # img of another size
                          (torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8), torch.zeros(1, 4))):   # a float window
        with pytest.raises(ValueError):
            loss(seg, img, win)
    with pytest.raises(_lib.MuscleHipError):                                # host tensors: no CPU path
        loss(torch.zeros(1, 3, 8, 8), torch.zeros(1, 3, 8, 8))


def test_train_muscle_arguments():
    from muscle_amd.train_muscle import parse_args
    a = parse_args(["--mask_root", "x"])
    assert (a.energy_weight, a.energy_sxy, a.energy_srgb, a.energy_scale, a.energy_trunc) == (0.0, 80.0, 15.0, 4, 2.0)
    a = parse_args(["--mask_root", "x", "--energy_weight", "0.5", "--energy_scale", "8", "--energy_trunc", "0"])
    assert (a.energy_weight, a.energy_scale, a.energy_trunc) == (0.5, 8, 0.0)
    with pytest.raises(SystemExit):
        parse_args(["--mask_root", "x", "--energy_weight", "1", "--crop_size", "450"])
