"""The boundary-evaluation kernels (csrc/boundary_eval.hip) and `evaluation.BoundaryEval` against the numpy restatement
tests/boundary_ref.py.  Everything is an integer table or a float64 value formed from one: every comparison is exact equality.
The shapes are the smallest at which the kernels can go wrong: one pixel, one row, one column, images smaller than the
radius (dmax 64 on 20 x 30), sizes that are no multiple of the 16 x 64 tile and span several tiles, void rows."""
import functools

import numpy as np
import pytest
import torch

import boundary_ref as R
from muscle_amd import ops
from muscle_amd.evaluation import BoundaryEval, SegEval

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _checker(H, W):
    yy, xx = np.mgrid[0:H, 0:W]
    return (((yy // 2) + (xx // 2)) % 2).astype(np.uint8)


def _blobs_with_a_block():
    """The main case: 14 cells over three tiles by three, void rows, and one 37 x 45 block of a single class in the lower left
    corner whose inside reaches the distances dmax and dmax + 1 with and without the image edge."""
    a = R.blobs(67, 130, 14, 21, seed=11, void_rows=(20, 21))
    a[30:, :45] = 3
    return a


# name -> (gt label map, K, dmax)
CASES = {
    "1x1": (lambda: np.array([[1]], np.uint8), 2, 16),
    "1x7": (lambda: np.array([[0, 0, 1, 1, 1, 255, 0]], np.uint8), 2, 16),
    "7x1": (lambda: np.array([[1, 1, 0, 255, 0, 0, 0]], np.uint8).T.copy(), 2, 16),
    "5x5const": (lambda: np.full((5, 5), 1, np.uint8), 2, 16),
    "checker9x13": (lambda: _checker(9, 13), 2, 16),
    "blobs67x130": (lambda: _blobs_with_a_block(), 21, 16),
    "blobs130x67": (lambda: R.blobs(130, 67, 14, 21, seed=12, void_rows=(33, 100)), 21, 16),
    "blobs67x130_K2": (lambda: R.blobs(67, 130, 9, 2, seed=13, void_rows=(7,)), 2, 16),
    "20x30_dmax1": (lambda: R.blobs(20, 30, 5, 21, seed=14, void_rows=(9,)), 21, 1),
    "20x30_dmax64": (lambda: R.blobs(20, 30, 3, 21, seed=15, void_rows=(9,)), 21, 64),
}
MAIN = "blobs67x130"


@functools.lru_cache(maxsize=None)
def _gt(name):
    a = CASES[name][0]()
    a.setflags(write=False)
    return a


@functools.lru_cache(maxsize=None)
def _pred(name, kind):
    """same: the ground truth itself (void pixels become class 0); shift: the ground truth moved by (2, 3) pixels; big: the shifted map
    with a stripe of values >= K."""
    gt, K = _gt(name), CASES[name][1]
    p = gt.copy()
    if kind != "same":
        p = np.roll(np.roll(p, 2 if gt.shape[0] > 2 else 0, axis=0), 3 if gt.shape[1] > 3 else 0, axis=1)
    p[p == 255] = 0
    if kind == "big":
        stripe = p[:, ::5]
        p[:, ::5] = np.array([K, K + 100, 255], np.uint8)[np.arange(stripe.size).reshape(stripe.shape) % 3]
    p.setflags(write=False)
    return p


@functools.lru_cache(maxsize=None)
def _ref_dist(name, edge):
    return R.edge_dist(_gt(name), CASES[name][2], edge)


@functools.lru_cache(maxsize=None)
def _ref_tables(name, kind):
    _, K, dmax = CASES[name]
    return R.tables(_pred(name, kind), _gt(name), K, dmax)


def _dev(a):
    return torch.from_numpy(np.array(a)).to(DEV)                          # a copy: the cached inputs are read-only


def _run(name, kind, adds=1):
    _, K, dmax = CASES[name]
    ev = BoundaryEval(DEV, K, dmax)
    for _ in range(adds):
        ev.add(_dev(_pred(name, kind)), _dev(_gt(name)))
    return ev


def test_the_main_case_is_not_degenerate():
    """Checked on the restatement alone, so that a kernel that returns constants cannot pass the table tests."""
    hist, rat = _ref_tables(MAIN, "shift")
    c = R.within(hist, 2)
    assert (c[3] > 0).sum() >= 3                                         # classes with T_b > 0 at d = 2
    assert ((c[5] > 0) & (c[5] < c[3])).any()                            # a class with 0 < TP_b < T_b
    assert (_ref_dist(MAIN, 0) != _ref_dist(MAIN, 1)).any()              # the image edge matters somewhere
    for edge in (0, 1):                                                  # pixels at exactly dmax (a scan one short would miss them) and beyond
        assert (_ref_dist(MAIN, edge) == CASES[MAIN][2]).any() and (_ref_dist(MAIN, edge) == CASES[MAIN][2] + 1).any()
    assert (hist[5] != hist[2]).any() and rat.sum() > 0
    big = _pred(MAIN, "big")
    assert (big >= CASES[MAIN][1]).any() and (_gt(MAIN) == 255).any()


@pytest.mark.parametrize("edge", [0, 1])
@pytest.mark.parametrize("name", sorted(CASES))
def test_distance_map_equals_the_window_scan(name, edge):
    dmax = CASES[name][2]
    got = ops.label_edge_dist(_dev(_gt(name)), dmax, edge).cpu().numpy()
    ref = _ref_dist(name, edge)
    assert got.dtype == np.uint8 and got.shape == ref.shape
    assert np.array_equal(got, ref), f"{name} edge={edge}: {(got != ref).sum()} of {ref.size} pixels differ"
    assert got.min() >= 1 and got.max() <= dmax + 1


def test_distance_map_of_the_prediction_and_into_a_given_buffer():
    p = _pred(MAIN, "big")
    out = torch.zeros(p.shape, dtype=torch.uint8, device=DEV)
    assert ops.label_edge_dist(_dev(p), 16, 1, out=out) is out
    assert np.array_equal(out.cpu().numpy(), R.edge_dist(p, 16, 1))


@pytest.mark.parametrize("name", sorted(CASES))
def test_pred_equal_gt_gives_tp_equal_t_equal_p(name):
    hist, rat = _run(name, "same").tables()
    void = _gt(name) == 255
    if not void.any():                                                   # with void pixels pred holds class 0 there: P and dp differ
        assert np.array_equal(hist[0], hist[1]) and np.array_equal(hist[3], hist[4]) and np.array_equal(rat[0], rat[1])
    assert np.array_equal(hist[0], hist[2])
    rh, rr = _ref_tables(name, "same")
    assert np.array_equal(hist, rh) and np.array_equal(rat, rr)
    if not void.any():
        assert np.array_equal(hist[3], hist[5]) and np.array_equal(rat[0], rat[2])


@pytest.mark.parametrize("kind", ["shift", "big"])
@pytest.mark.parametrize("name", sorted(CASES))
def test_tables_equal_the_restatement(name, kind):
    hist, rat = _run(name, kind).tables()
    rh, rr = _ref_tables(name, kind)
    assert hist.dtype == np.int64 and hist.shape == rh.shape and rat.shape == rr.shape
    assert np.array_equal(hist, rh), f"rows that differ: {sorted(set(np.argwhere(hist != rh)[:, 0].tolist()))}"
    assert np.array_equal(rat, rr)
    assert hist[:, :, 0].sum() == 0


@pytest.mark.parametrize("name", ["1x7", MAIN])
def test_gt_all_void_counts_nothing(name):
    _, K, dmax = CASES[name]
    ev = BoundaryEval(DEV, K, dmax)
    ev.add(_dev(_pred(name, "shift")), _dev(np.full(_gt(name).shape, 255, np.uint8)))
    hist, rat = ev.tables()
    assert hist.sum() == 0 and rat.sum() == 0


def test_two_adds_equal_the_sum_and_two_runs_give_the_same_bits():
    a, b = _run(MAIN, "shift"), _run("blobs130x67", "big")
    _, K, dmax = CASES[MAIN]
    both = BoundaryEval(DEV, K, dmax)
    both.add(_dev(_pred(MAIN, "shift")), _dev(_gt(MAIN)))
    both.add(_dev(_pred("blobs130x67", "big")), _dev(_gt("blobs130x67")))
    (ha, ra), (hb, rb), (h2, r2) = a.tables(), b.tables(), both.tables()
    assert np.array_equal(h2, ha + hb) and np.array_equal(r2, ra + rb)
    again = _run(MAIN, "shift")
    assert torch.equal(again.hist, a.hist) and torch.equal(again.ratio_counts, a.ratio_counts)
    twice = _run(MAIN, "shift", adds=2).tables()
    assert np.array_equal(twice[0], 2 * ha) and np.array_equal(twice[1], 2 * ra)
    both.reset()
    assert int(both.hist.sum()) == 0 and int(both.ratio_counts.sum()) == 0


@pytest.mark.parametrize("name", [MAIN, "blobs67x130_K2", "20x30_dmax64"])
def test_all_bins_sum_to_seg_evals_table(name):
    """Values < K or 255 only (the shifted prediction): rows 2 / 1 / 0 summed over every bin are mx_seg_confusion's (TP, P, T)."""
    _, K, dmax = CASES[name]
    p, g = _dev(_pred(name, "shift")), _dev(_gt(name))
    se = SegEval(DEV, K)
    se.add(p, g)
    conf = se.counts.cpu().numpy()
    hist, _ = _run(name, "shift").tables()
    assert conf[:, 2].sum() > 0
    assert np.array_equal(hist[2].sum(axis=1), conf[:, 0]) and np.array_equal(hist[5].sum(axis=1), conf[:, 0])
    assert np.array_equal(hist[1].sum(axis=1), conf[:, 1]) and np.array_equal(hist[4].sum(axis=1), conf[:, 1])
    assert np.array_equal(hist[0].sum(axis=1), conf[:, 2]) and np.array_equal(hist[3].sum(axis=1), conf[:, 2])


def test_validation_feeds_the_evaluator_the_predictions_it_counts(tmp_path):
    """SegValidation(boundary=) / validate_seg(boundary=): the evaluator's tables are those of `add` on the returned predictions, per
    image and batched, and the mIoU table is what it is without the evaluator."""
    import PIL.Image
    import muscle_amd
    from muscle_amd.evaluation import SegValidation, validate_seg
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    rng = np.random.default_rng(5)
    names, imgs, gts = ["a", "b", "c"], [], []
    for i, (nm, (h, w)) in enumerate(zip(names, ((40, 56), (33, 47), (40, 56)))):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([127 + 100 * np.sin(xx / (4.0 + c) + i) * np.cos(yy / (6.0 - c)) for c in range(3)], -1) + rng.normal(0, 12, (h, w, 3))
        PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        PIL.Image.fromarray(R.blobs(h, w, 5, 21, seed=20 + i, void_rows=(3,))).save(root / "SegmentationClass" / f"{nm}.png")
        imgs.append(PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB"))
        gts.append(np.array(PIL.Image.open(root / "SegmentationClass" / f"{nm}.png")))
    torch.manual_seed(1)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(DEV).eval()
    dev = torch.device(DEV)
    plain = SegValidation(dev, 21)
    val = SegValidation(dev, 21, boundary=BoundaryEval(dev, 21, 8))
    want = BoundaryEval(dev, 21, 8)
    with torch.no_grad():
        for im, gt, nm in zip(imgs, gts, names):
            pred = val.add(model, im, gt, nm)
            assert torch.equal(pred, plain.add(model, im, gt, nm))
            want.add(pred, _dev(gt))
    assert int(want.hist.sum()) > 0 and torch.equal(val.table.counts, plain.table.counts)
    assert torch.equal(val.boundary.hist, want.hist) and torch.equal(val.boundary.ratio_counts, want.ratio_counts)
    batched = SegValidation(dev, 21, boundary=BoundaryEval(dev, 21, 8))
    with torch.no_grad():
        batched.add_batch(model, [imgs[0], imgs[2]], [gts[0], gts[2]], ["a", "c"])
        batched.add_batch(model, [imgs[1]], [gts[1]], ["b"])
    assert torch.equal(batched.boundary.hist, want.hist) and torch.equal(batched.boundary.ratio_counts, want.ratio_counts)
    for batch in (1, 2):
        bev = BoundaryEval(dev, 21, 8)
        assert validate_seg(model, names, str(root), dev, 21, batch=batch, boundary=bev) == plain.miou()
        assert torch.equal(bev.hist, want.hist) and torch.equal(bev.ratio_counts, want.ratio_counts)
    val.reset()
    assert int(val.boundary.hist.sum()) == 0 and int(val.table.counts.sum()) == 0


@pytest.mark.parametrize("name", [MAIN, "checker9x13", "20x30_dmax1"])
def test_metrics_equal_the_restatement(name):
    _, K, dmax = CASES[name]
    ev = _run(name, "shift")
    rh, rr = _ref_tables(name, "shift")
    curve = ev.trimap_curve()
    assert len(curve) == dmax
    for d in range(1, dmax + 1):
        assert ev.trimap_miou(d) == curve[d - 1] == R.trimap_miou(rh, d)
        assert ev.boundary_miou(d) == R.boundary_miou(rh, d)
    mean, per_class = R.ratio_miou(rr)
    assert ev.boundary_miou() == mean
    log = ev.loglist()
    assert log["mIoU"] == mean and len(log) == K + 1
    assert [log[k] for k in list(log)[:K]] == per_class
    if name == MAIN:
        assert 0.0 < mean < 100.0 and curve[0] != curve[-1]
    lines = ev.lines()
    assert len(lines) == 1 + (K + 1) // 2 + 1 + dmax and lines[-1].startswith("trimap d=%2d" % dmax)
