"""Host side of the boundary evaluation ("Boundary evaluation"): the numpy restatement tests/boundary_ref.py against
scipy's erosions and against a plain confusion count, the per-image radius rule, the scripts' new flags, the declared entry
points and their argument errors (reported before any launch, so no GPU is needed)."""
import ctypes
import os

import numpy as np
import pytest

import boundary_ref as R
from muscle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _maps():
    yield np.zeros((1, 1), np.uint8)
    yield np.array([[0, 0, 1, 1, 1, 255, 0]], np.uint8)
    yield np.array([[3, 3, 1, 1, 1, 255, 0]], np.uint8).T.copy()
    yield np.full((5, 5), 7, np.uint8)
    yield R.blobs(17, 23, 6, 4, seed=0, void_rows=(5,))
    yield R.blobs(12, 9, 5, 3, seed=1)


@pytest.mark.parametrize("dmax", [1, 2, 5, 16])
def test_band_is_mask_minus_erosion(dmax):
    """(L == c) & (dist_edge1 <= d) == mask_c & ~binary_erosion(mask_c, 3x3 ones, iterations=d, border_value=0) for every value c
    of the map (255 included: it is an ordinary value) and every d <= dmax."""
    from scipy.ndimage import binary_erosion
    for L in _maps():
        dist = R.edge_dist(L, dmax, 1)
        assert dist.min() >= 1 and dist.max() <= dmax + 1
        for c in np.unique(L):
            mask = L == c
            for d in range(1, dmax + 1):
                band = mask & ~binary_erosion(mask, np.ones((3, 3), bool), iterations=d, border_value=0)
                assert np.array_equal(mask & (dist <= d), band), (L.shape, int(c), d)


@pytest.mark.parametrize("edge", [0, 1])
def test_window_scan_equals_the_erosion_form(edge):
    for L in _maps():
        for dmax in (1, 3, 16):
            assert np.array_equal(R.edge_dist(L, dmax, edge), R.edge_dist_erosion(L, dmax, edge)), (L.shape, dmax)


def test_edge0_ignores_the_image_border_and_edge1_does_not():
    L = np.zeros((6, 8), np.uint8)
    assert (R.edge_dist(L, 3, 0) == 4).all()
    e1 = R.edge_dist(L, 3, 1)
    assert e1[0].tolist() == [1] * 8 and e1[2].tolist() == [1, 2, 3, 3, 3, 3, 2, 1] and e1[3, 3] == 3
    L[:, 4:] = 255                                                     # a pixel next to a void pixel is at distance 1
    assert R.edge_dist(L, 3, 0)[0].tolist() == [4, 3, 2, 1, 1, 2, 3, 4]


def test_all_bins_sum_to_the_plain_confusion_count():
    gt = R.blobs(19, 27, 7, 4, seed=3, void_rows=(4, 11))
    pred = np.roll(gt, 2, axis=1)
    pred[pred == 255] = 9                                              # a value >= K in the prediction
    for K, dmax in ((4, 3), (3, 8)):                                   # K = 3: class 3 of gt belongs to no class
        hist, rat = R.tables(pred, gt, K, dmax)
        conf = R.confusion(pred, gt, K)
        assert hist[:, :, 0].sum() == 0
        assert np.array_equal(hist[2].sum(axis=1), conf[:, 0])
        assert np.array_equal(hist[1].sum(axis=1), conf[:, 1]) and np.array_equal(hist[4].sum(axis=1), conf[:, 1])
        assert np.array_equal(hist[0].sum(axis=1), conf[:, 2]) and np.array_equal(hist[3].sum(axis=1), conf[:, 2])
        assert np.array_equal(hist[5].sum(axis=1), conf[:, 0])
        assert conf[:, 0].sum() > 0 and (conf[:, 0] < conf[:, 2]).any()
        d_img = R.image_radius(19, 27, 0.02, dmax)
        assert np.array_equal(rat, R.within(hist, d_img)[3:6])
        h2, r2 = R.tables_erosion(pred, gt, K, dmax)
        assert np.array_equal(h2, hist) and np.array_equal(r2, rat)


def test_image_radius_rule():
    from muscle_amd.evaluation import boundary_radius
    for H, W, dmax, want in ((1, 1, 16, 1), (375, 500, 16, 12), (375, 500, 8, 8), (2000, 2000, 16, 16), (100, 100, 16, 3)):
        assert R.image_radius(H, W, 0.02, dmax) == want == boundary_radius(H, W, 0.02, dmax), (H, W, dmax)
    assert boundary_radius(375, 500, 0.02, 16) == 12                   # 0.02 * 625 = 12.5: Python's round goes to the even value
    assert boundary_radius(300, 400, 0.05, 64) == 25


def test_metric_arithmetic_on_a_hand_table():
    hist = np.zeros((6, 2, 4), np.int64)
    hist[0, 0, 1:] = [4, 2, 10]
    hist[1, 0, 1:] = [3, 3, 9]
    hist[2, 0, 1:] = [2, 1, 8]
    assert R.trimap_miou(hist, 1) == (2 / (4 + 3 - 2 + 1e-10) + 0.0) / 2 * 100
    assert R.trimap_miou(hist, 2) == (3 / (6 + 6 - 3 + 1e-10) + 0.0) / 2 * 100
    assert R.boundary_miou(hist, 2) == 0.0


def test_script_arguments():
    from muscle_amd import evaluation, infer_seg, train_muscle
    a = evaluation.parse_args(["--comment", "c", "--type", "png"])
    assert a.boundary == 0 and a.boundary_dmax == 16 and a.boundary_ratio == 0.02
    a = evaluation.parse_args(["--comment", "c", "--type", "png", "--boundary", "1", "--boundary_dmax", "8", "--boundary_ratio", "0.01"])
    assert a.boundary == 1 and a.boundary_dmax == 8 and a.boundary_ratio == 0.01
    with pytest.raises(SystemExit):
        evaluation.parse_args(["--comment", "c", "--type", "npy", "--t", "0.3", "--boundary", "1"])
    with pytest.raises(SystemExit):
        evaluation.parse_args(["--comment", "c", "--type", "png", "--boundary", "1", "--boundary_dmax", "65"])
    assert infer_seg.parse_args(["--weights", "w"]).boundary == 0
    assert infer_seg.parse_args(["--weights", "w", "--gt_dir", "g", "--boundary", "1"]).boundary == 1
    with pytest.raises(SystemExit):
        infer_seg.parse_args(["--weights", "w", "--boundary", "1"])      # nothing to compare against without --gt_dir
    assert train_muscle.parse_args(["--mask_root", "m"]).val_boundary == 0
    assert train_muscle.parse_args(["--mask_root", "m", "--val_boundary", "1"]).val_boundary == 1


def test_entry_points_are_declared_and_refuse_bad_arguments_before_any_launch():
    sigs = _lib.parse_header()
    assert sigs["mx_label_edge_dist"] == "piiiipp" and sigs["mx_boundary_counts"] == "pppppiiiiippp"
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)                               # never dereferenced: every call returns before a launch
    p = ctypes.addressof(buf)
    for kw in (dict(H=0), dict(W=0), dict(H=-3), dict(dmax=0), dict(dmax=65), dict(edge=2), dict(edge=-1), dict(H=1 << 16, W=1 << 15)):
        a = {**dict(H=4, W=4, dmax=2, edge=1), **kw}
        assert L.mx_label_edge_dist(p, a["H"], a["W"], a["dmax"], a["edge"], p, None) < 0, kw
        assert b"label_edge_dist" in L.mx_last_error(), kw
    assert L.mx_label_edge_dist(None, 4, 4, 2, 1, p, None) < 0 and L.mx_label_edge_dist(p, 4, 4, 2, 1, None, None) < 0
    for kw in (dict(K=1), dict(K=33), dict(H=0), dict(W=-1), dict(dmax=0), dict(dmax=65), dict(d_img=0), dict(d_img=3),
               dict(H=1 << 16, W=1 << 15)):
        a = {**dict(K=3, H=4, W=4, dmax=2, d_img=1), **kw}
        assert L.mx_boundary_counts(p, p, p, p, p, a["K"], a["H"], a["W"], a["dmax"], a["d_img"], p, p, None) < 0, kw
        assert b"boundary_counts" in L.mx_last_error(), kw
    for i in (0, 1, 2, 3, 4, 10, 11):
        args = [p, p, p, p, p, 3, 4, 4, 2, 1, p, p]
        args[i] = None
        assert L.mx_boundary_counts(*args, None) < 0 and b"boundary_counts" in L.mx_last_error(), i


def test_host_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    from muscle_amd import ops
    from muscle_amd.evaluation import BoundaryEval, SegValidation, validate_seg
    import inspect
    g = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(_lib.MuscleHipError):
        BoundaryEval("cpu").add(g, g)
    with pytest.raises(_lib.MuscleHipError):
        ops.label_edge_dist(g, 2, 1)
    with pytest.raises(ValueError):
        ops.label_edge_dist(g.float(), 2, 1)
    for kw in (dict(num_cls=1), dict(num_cls=33), dict(dmax=0), dict(dmax=65), dict(ratio=0.0)):
        with pytest.raises(ValueError):
            BoundaryEval("cpu", **kw)
    ev = BoundaryEval("cpu", 3, 4)
    hist, rat = ev.tables()
    assert hist.shape == (6, 3, 6) and rat.shape == (3, 3) and hist.dtype == rat.dtype == np.int64
    assert ev.trimap_curve() == [0.0] * 4 and ev.boundary_miou() == 0.0 and ev.loglist()["mIoU"] == 0.0
    with pytest.raises(ValueError):
        ev.trimap_miou(5)
    assert inspect.signature(validate_seg).parameters["boundary"].default is None
    assert inspect.signature(SegValidation.__init__).parameters["boundary"].default is None


def test_documents_state_the_contract_and_the_unpinned_parity():
    read = lambda f: open(os.path.join(ROOT, f)).read()  # noqa: E731
    design, integ, readme = read("DESIGN.md"), read("INTEGRATION.md"), read("README.md")
    assert "### Boundary evaluation" in design and "unpinned" in design and "Boundary IoU" in design
    for text in (integ, readme):
        assert "--boundary 1" in text and "--val_boundary 1" in text
    assert "boundary_eval_bench.txt" in read("profiles/README.md")
    assert os.path.exists(os.path.join(ROOT, "tools", "bench_boundary_eval.py"))
