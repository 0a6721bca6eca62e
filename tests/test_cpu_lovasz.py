"""The Lovasz-softmax model without a GPU: the numpy restatement (lovasz_ref.py) against torch autograd of Berman's published
function (written out below from the paper), its closed forms, the numpy mirror of the sort key, and train_muscle's flags."""
import numpy as np
import pytest
import torch

import lovasz_ref as R

# (N, K, H, W, classes, per_image, absent classes): the shapes the kernels are tested on
CASES = {
    "1x3x5x7": (1, 3, 5, 7, "present", False, ()),
    "2x21x24x40_present": (2, 21, 24, 40, "present", False, (4, 17)),
    "2x21x24x40_all": (2, 21, 24, 40, "all", False, (4, 17)),
    "3x24x33x10_per_image": (3, 24, 33, 10, "present", True, ()),
}


# ---- Berman, Triki & Blaschko (CVPR 2018), Algorithm 1 and the published lovasz_softmax_flat, in float64 torch -------------------------
def _berman_grad(gt_sorted):
    gts = gt_sorted.sum()
    intersection = gts - gt_sorted.cumsum(0)
    union = gts + (1 - gt_sorted).cumsum(0)
    jaccard = 1.0 - intersection / union
    if len(gt_sorted) > 1:
        jaccard[1:] = jaccard[1:] - jaccard[:-1]
    return jaccard


def _berman_flat(probas, labels, classes):
    losses = []
    for c in range(probas.shape[1]):
        fg = (labels == c).double()
        if classes == "present" and fg.sum() == 0:
            continue
        errors = (fg - probas[:, c]).abs()
        errors_sorted, perm = torch.sort(errors, 0, descending=True)
        losses.append(torch.dot(errors_sorted, _berman_grad(fg[perm])))
    return sum(losses) / len(losses) if losses else probas.sum() * 0.0


def _berman(seg, label, classes, per_image):
    K = seg.shape[1]
    probas = torch.softmax(seg, 1)

    def flat(p, l):
        p, l = p.permute(0, 2, 3, 1).reshape(-1, K), l.reshape(-1)
        keep = (l != 255) & (l < K)
        if not bool(keep.any()):
            return p.sum() * 0.0
        return _berman_flat(p[keep], l[keep], classes)
    if per_image:
        return sum(flat(probas[n:n + 1], label[n:n + 1]) for n in range(seg.shape[0])) / seg.shape[0]
    return flat(probas, label)


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_matches_autograd_of_bermans_function(name):
    N, K, H, W, classes, per_image, absent = CASES[name]
    seg, lab = R.make_case(N, K, H, W, seed=sorted(CASES).index(name), absent=absent)
    r = R.lovasz(seg, lab, classes, per_image, np.float64, gup=0.37)
    t = torch.from_numpy(seg).double().requires_grad_(True)
    loss = _berman(t, torch.from_numpy(lab.astype(np.int64)), classes, per_image)
    (0.37 * loss).backward()
    assert abs(float(loss.detach()) - float(r["loss"])) <= 1e-12
    assert np.abs(t.grad.numpy() - r["gseg"]).max() <= 1e-12
    assert float(r["loss"]) > 0 and np.abs(r["gseg"]).max() > 0
    for c in absent:
        assert r["counts"][c, 0] == 0


def test_closed_form_equals_the_jaccard_differences():
    g = np.random.default_rng(3)
    for G in (0, 1, 5, 40):
        P = 40
        fg = np.zeros(P, bool)
        fg[g.permutation(P)[:G]] = True
        e = g.random(P)
        _, inc, _, _, _ = R.segment(e, fg, np.ones(P, bool), np.float64)
        order = np.argsort(-e, kind="stable")
        want = _berman_grad(torch.from_numpy(fg[order].astype(np.float64))).numpy()
        assert np.abs(inc[order] - want).max() <= 1e-12


def test_one_valid_pixel_gives_its_error():
    seg, lab = R.make_case(1, 3, 5, 7, seed=1)
    lab[:] = 255
    lab[0, 2, 3] = 1
    r = R.lovasz(seg, lab, "present")
    assert r["counts"][1].tolist() == [1, 1] and abs(float(r["loss"]) - float(r["err"][1, 2 * 7 + 3])) <= 1e-15


def test_no_foreground_under_all_gives_the_largest_error():
    seg, lab = R.make_case(2, 4, 6, 10, seed=2, absent=(3,))
    r = R.lovasz(seg, lab, "all")
    assert r["counts"][3, 0] == 0 and abs(float(r["seg_loss"][3]) - float(r["err"][3].max())) <= 1e-15


def test_a_perfect_prediction_has_no_loss():
    _, lab = R.make_case(2, 5, 8, 12, seed=4, ignored=0.1)
    seg = 40.0 * (np.minimum(lab, 4)[:, None] == np.arange(5)[None, :, None, None]).astype(np.float32)
    for classes in ("present", "all"):
        assert 0.0 <= float(R.lovasz(seg, lab, classes)["loss"]) < 1e-6


def test_the_loss_does_not_depend_on_the_pixel_order():
    seg, lab = R.make_case(1, 6, 9, 11, seed=5)
    perm = np.random.default_rng(6).permutation(99)
    a = R.lovasz(seg, lab, "present")
    b = R.lovasz(seg.reshape(1, 6, 99)[:, :, perm].reshape(1, 6, 9, 11), lab.reshape(1, 99)[:, perm].reshape(1, 9, 11), "present")
    assert abs(float(a["loss"]) - float(b["loss"])) <= 1e-14


@pytest.mark.parametrize("per_image", [False, True])
def test_all_ignored_gives_zero_loss_and_gradient(per_image):
    seg, lab = R.make_case(2, 5, 4, 6, seed=7)
    lab[:] = 255
    lab[1, 0, 0] = 9                                                   # a value >= K is ignored too, never an index
    for dtype in (np.float64, np.float32):
        r = R.lovasz(seg, lab, "all", per_image, dtype)
        assert float(r["loss"]) == 0.0 and not r["gseg"].any() and (r["rank"] == -1).all()


def test_float32_mode_stays_in_float32_and_order_from_is_taken():
    seg, lab = R.make_case(2, 5, 8, 12, seed=8)
    r64 = R.lovasz(seg, lab, "present", dtype=np.float64)
    r32 = R.lovasz(seg, lab, "present", dtype=np.float32)
    for k in ("loss", "gseg", "err", "g", "seg_loss"):
        assert np.asarray(r32[k]).dtype == np.float32, k
    assert abs(float(r32["loss"]) - float(r64["loss"])) < 1e-5
    o = R.lovasz(seg, lab, "present", dtype=np.float64, order_from=r32["err"])
    assert np.array_equal(o["rank"], r32["rank"])


def test_key_of_orders_as_a_stable_descending_sort():
    from muscle_amd.lovasz import KEY_INVALID, KEY_ONE, key_of
    g = np.random.default_rng(11)
    bits = g.integers(0, 0x3F800000, 100000, dtype=np.int64, endpoint=True).astype(np.uint32)
    special = np.array([0.0, 1.0, 1e-45, 1e-39, 1.1754942e-38, np.nan, 0.0, 1.0, np.nan], np.float32)
    e = np.concatenate([bits.view(np.float32), special, bits[:500].view(np.float32)])        # exact repeats: ties
    e = e[g.permutation(e.size)]
    key = key_of(e)
    assert key.dtype == np.uint32 and int(key.max()) <= KEY_ONE < KEY_INVALID
    as_one = np.where(np.isnan(e), np.float32(1.0), e)                 # NaN sorts with e = 1
    assert np.array_equal(np.argsort(key, kind="stable"), np.argsort(-as_one, kind="stable"))
    assert key_of(np.float32(1.0)) == 0 and key_of(np.float32(0.0)) == KEY_ONE and key_of(np.float32(np.nan)) == 0
    assert key_of(np.float32(2.0)) == 0 and key_of(np.float32(-0.5)) == 0 and key_of(np.float32(np.inf)) == 0


def test_train_muscle_flags():
    from muscle_amd.train_muscle import parse_args
    a = parse_args(["--mask_root", "m"])
    assert a.lovasz_weight == 0.0 and a.lovasz_classes == "present" and a.lovasz_per_image == 0
    a = parse_args(["--mask_root", "m", "--mask_type", "label", "--lovasz_weight", "0.5", "--lovasz_classes", "all", "--lovasz_per_image", "1"])
    assert a.lovasz_weight == 0.5 and a.lovasz_classes == "all" and a.lovasz_per_image == 1
    for bad in (["--mask_type", "label", "--lovasz_weight", "-1"],
                ["--lovasz_weight", "0.5"],
                ["--mask_type", "label", "--lovasz_weight", "0.5", "--beacon_sampler", "device", "--graph", "1"]):
        with pytest.raises(SystemExit):
            parse_args(["--mask_root", "m"] + bad)


def test_bad_arguments_raise_before_any_launch():
    from muscle_amd import LovaszSoftmaxLoss, lovasz_softmax
    from muscle_amd._lib import MuscleHipError
    seg, lab = torch.zeros(2, 5, 4, 6), torch.zeros(2, 4, 6, dtype=torch.uint8)
    with pytest.raises(ValueError):
        LovaszSoftmaxLoss(classes="some")
    with pytest.raises(ValueError):
        lovasz_softmax(seg, lab, classes="some")
    with pytest.raises(ValueError):
        lovasz_softmax(seg, lab.long())
    with pytest.raises(ValueError):
        lovasz_softmax(seg, lab[:, :3])
    with pytest.raises(ValueError):
        lovasz_softmax(torch.zeros(2, 25, 4, 6), lab)
    with pytest.raises(ValueError):
        lovasz_softmax(seg[0], lab)
    with pytest.raises(MuscleHipError):
        lovasz_softmax(seg, lab)
