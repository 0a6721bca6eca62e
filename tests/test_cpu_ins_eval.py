"""Host side of the instance evaluation (muscle_amd/ins_eval.py): the VOC AP on hand-worked cases with known values, the
ground-truth builder, the product's AP against the numpy restatement tests/ins_eval_ref.py on seeded random tables, and the
argument errors of the two entry points (reported before any launch, so no GPU is needed)."""
import ctypes
import math

import numpy as np
import pytest

import ins_eval_ref as R
from muscle_amd import _lib
from muscle_amd.ins_eval import InsSegEval, average_precision, mask_iou, voc_instances

T4 = (0.25, 0.5, 0.7, 0.75)


def _eval(images, num_cls=3, thresholds=(0.5,)):
    ev = InsSegEval("cpu", num_cls, thresholds)
    for iou, score, cls, gt_cls in images:
        ev.add_iou(np.asarray(iou, np.float64).reshape(len(score), len(gt_cls)), score, cls, gt_cls)
    return ev.result()


# ---- AP on hand-worked cases ------------------------------------------------------------------------------------------------
def test_perfect_predictions_give_one():
    r = _eval([([[1.0, 0.0], [0.0, 1.0]], [0.9, 0.8], [0, 1], [0, 1])], num_cls=2)
    assert r["ap"].tolist() == [[1.0, 1.0]] and r["map"].tolist() == [1.0]


def test_tp_fp_tp_over_two_objects_gives_five_sixths():
    iou = [[0.9, 0.0], [0.1, 0.1], [0.0, 0.9]]
    r = _eval([(iou, [0.9, 0.8, 0.7], [0, 0, 0], [0, 0])], num_cls=1)
    assert abs(r["ap"][0, 0] - 5.0 / 6.0) <= 1e-15
    assert abs(r["ap"][0, 0] - R.evaluate([(np.array(iou), [0.9, 0.8, 0.7], [0, 0, 0], [0, 0])], 1, (0.5,))["ap"][0, 0]) <= 1e-15


def test_a_second_hit_on_a_taken_object_is_a_false_positive():
    # both predictions overlap object 0 best; the second finds it taken although its IoU passes: TP, FP, and object 1 is never found
    iou = [[0.9, 0.0], [0.8, 0.6]]
    r = _eval([(iou, [0.9, 0.8], [0, 0], [0, 0])], num_cls=1)
    assert r["ap"][0, 0] == 0.5                                # recall stops at 1/2 with precision 1
    # the arg-max is taken before the "taken" test: the second prediction does NOT fall back to object 1 (IoU 0.6 >= 0.5)


def test_objects_without_predictions_give_zero_and_predictions_without_objects_give_nan():
    # class 0: one object, no prediction -> 0; class 1: a prediction, no object -> nan, out of map; class 2: nothing -> nan
    r = _eval([([[0.9]], [0.5], [1], [0])], num_cls=3)
    assert r["ap"][0, 0] == 0.0 and math.isnan(r["ap"][0, 1]) and math.isnan(r["ap"][0, 2])
    assert r["map"][0] == 0.0


def test_all_classes_nan_gives_nan():
    r = _eval([(np.zeros((1, 0)), [0.5], [1], [])], num_cls=3)
    assert np.isnan(r["ap"]).all() and math.isnan(r["map"][0])
    assert np.isnan(InsSegEval("cpu", 2).result()["map"]).all()               # nothing added at all


def test_an_image_without_objects_of_the_class_counts_its_predictions_as_false_positives():
    a = ([[0.9]], [0.4], [0], [0])                              # image 1: a TP at score 0.4
    b = (np.zeros((1, 1)), [0.8], [0], [1])                     # image 2: a class-0 prediction, the only object is class 1 -> FP at 0.8
    r = _eval([a, b], num_cls=2)
    assert r["ap"][0, 0] == 0.5 and r["ap"][0, 1] == 0.0         # FP first, then TP: precision 1/2 at recall 1


def test_thresholds_share_one_iou_matrix():
    r = _eval([([[0.6]], [0.5], [0], [0])], num_cls=1, thresholds=T4)
    assert r["ap"][:, 0].tolist() == [1.0, 1.0, 0.0, 0.0]
    r = _eval([([[0.5]], [0.5], [0], [0])], num_cls=1, thresholds=(0.5,))
    assert r["ap"][0, 0] == 1.0                                 # IoU >= t, not >


def test_score_zero_takes_part():
    r = _eval([([[0.9]], [0.0], [0], [0])], num_cls=1)
    assert r["ap"][0, 0] == 1.0


# ---- tie order --------------------------------------------------------------------------------------------------------------
def test_score_ties_within_an_image_resolve_by_ascending_index():
    first_tp = _eval([([[0.9], [0.1]], [0.5, 0.5], [0, 0], [0])], num_cls=1)["ap"][0, 0]
    first_fp = _eval([([[0.1], [0.9]], [0.5, 0.5], [0, 0], [0])], num_cls=1)["ap"][0, 0]
    assert first_tp == 1.0 and first_fp == 0.5                  # the reverse tie order would swap the two values


def test_score_ties_across_images_resolve_by_order_of_add():
    tp = ([[0.9]], [0.5], [0], [0])
    fp = (np.zeros((1, 0)), [0.5], [0], [])
    assert _eval([tp, fp], num_cls=1)["ap"][0, 0] == 1.0
    assert _eval([fp, tp], num_cls=1)["ap"][0, 0] == 0.5
    for images in ([tp, fp], [fp, tp]):
        ref = R.evaluate([(np.asarray(i, np.float64).reshape(len(s), len(g)), s, c, g) for i, s, c, g in images], 1, (0.5,))
        assert ref["ap"][0, 0] == _eval(images, num_cls=1)["ap"][0, 0]


def test_average_precision_edges():
    assert math.isnan(average_precision(np.zeros(0), np.zeros(0, bool), 0))
    assert average_precision(np.zeros(0), np.zeros(0, bool), 3) == 0.0
    assert average_precision(np.array([0.3, 0.9]), np.array([False, True]), 1) == 1.0


# ---- voc_instances ----------------------------------------------------------------------------------------------------------
def test_voc_instances_hand_case():
    obj = np.array([[0, 3, 3, 3, 255],
                    [7, 7, 9, 9, 255],
                    [7, 7, 9, 200, 200]], np.uint8)
    cls = np.array([[0, 5, 5, 2, 255],
                    [4, 2, 0, 255, 255],
                    [2, 4, 0, 21, 0]], np.uint8)
    G, gt = voc_instances(cls, obj, 20)
    # object 3: class 5 twice, 2 once -> 5; object 7: classes 4 and 2 twice each -> the smaller, 2; object 9: only background and
    # void -> dropped; object 200: class 21 > num_cls and background -> dropped; void (255) -> 0
    assert gt.tolist() == [4, 1] and gt.dtype == np.int64
    assert G.dtype == np.uint8 and G.tolist() == [[0, 1, 1, 1, 0], [2, 2, 0, 0, 0], [2, 2, 0, 0, 0]]
    G21, gt21 = voc_instances(cls, obj, 21)
    assert gt21.tolist() == [4, 1, 20] and G21[2].tolist() == [2, 2, 0, 3, 3]


def test_voc_instances_empty_image_and_bad_input():
    G, gt = voc_instances(np.zeros((3, 4), np.uint8), np.full((3, 4), 255, np.uint8))
    assert gt.shape == (0,) and not G.any()
    with pytest.raises(ValueError):
        voc_instances(np.zeros((3, 4), np.uint8), np.zeros((4, 3), np.uint8))
    with pytest.raises(ValueError):
        voc_instances(np.zeros((3, 4), np.int32), np.zeros((3, 4), np.int32))


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_voc_instances_equals_the_restatement(seed):
    rng = np.random.RandomState(seed)
    obj = R.blobs(24, 31, 9, seed).astype(np.uint8) * 20               # ids 20, 40, ..: compacted in ascending order
    obj[rng.rand(24, 31) < 0.05] = 255
    cls = rng.randint(0, 23, (24, 31)).astype(np.uint8)
    cls[rng.rand(24, 31) < 0.05] = 255
    cls[obj == 40] = 0                                                 # an object with no class pixel
    G, gt = voc_instances(cls, obj, 20)
    Gr, gtr = R.gt_instances(cls, obj, 20)
    assert np.array_equal(G, Gr) and np.array_equal(gt, gtr) and gt.size >= 2
    assert sorted(set(G.reshape(-1).tolist())) == list(range(gt.size + 1))


# ---- product against the restatement ----------------------------------------------------------------------------------------
def _random_images(seed, overlapping):
    rng = np.random.RandomState(seed)
    images = []
    for _ in range(5):
        n, m = rng.randint(0, 13), rng.randint(0, 7)
        t = rng.randint(0, 40, (n + 1, m + 1))
        for k in range(1, min(n, m) + 1):
            if rng.rand() < 0.7:
                t[k, k] += rng.randint(50, 400)                        # IoUs on both sides of every threshold
        if overlapping:
            t[0] = np.maximum(t[0], t[1:].max(0) if n else 0)           # row 0 counts every pixel: no mask row can exceed it
        gt_cls = rng.randint(0, 20, m)
        cls = np.array([gt_cls[k] if k < m and rng.rand() < 0.8 else rng.randint(0, 20) for k in range(n)], np.int64)
        score = np.round(rng.rand(n), 1)                                # ties occur
        images.append((t.astype(np.int32), score, cls, gt_cls))
    return images


@pytest.mark.parametrize("overlapping", [False, True])
@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_ap_equals_the_restatement_on_random_tables(seed, overlapping):
    """Both sides are float64 on identical integers; only the summation order of <= 10^4 terms <= 1 can differ: |d| <= 1e-12."""
    images = _random_images(seed, overlapping)
    ev = InsSegEval("cpu", 20, T4)
    ref_in = []
    for t, score, cls, gt_cls in images:
        iou = mask_iou(t, overlapping)
        ref_iou = R.iou_from_table(t, overlapping)
        assert iou.shape == ref_iou.shape and iou.dtype == np.float64
        assert np.array_equal(iou, ref_iou)                             # one division of the same two integers
        ev.add_iou(iou, score, cls, gt_cls)
        ref_in.append((ref_iou, score, cls, gt_cls))
    got, ref = ev.result(), R.evaluate(ref_in, 20, T4)
    assert got["ap"].shape == (4, 20) and got["map"].shape == (4,)
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(ref["ap"]))
    d = np.nanmax(np.abs(got["ap"] - ref["ap"]))
    dm = np.abs(got["map"] - ref["map"]).max()
    print(f"[ins_eval] seed {seed} overlapping={overlapping}: max |dAP| = {d:.3g}, max |dmAP| = {dm:.3g}, mAP = {got['map']}")
    assert d <= 1e-12 and dm <= 1e-12
    assert np.nanmax(got["ap"]) > 0 and (~np.isnan(got["ap"])).sum() >= 8      # the case is not degenerate


def test_mask_iou_forms():
    # label-map form: A_g is the column sum (row 0 holds the object's pixels outside every segment)
    t = np.array([[10, 4], [2, 6]])
    assert mask_iou(t, False)[0, 0] == 6 / (8 + 10 - 6)
    # mask form: row 0 counts every pixel, A_g = row 0
    assert mask_iou(t, True)[0, 0] == 6 / (8 + 4 - 6)
    assert mask_iou(np.zeros((1, 3)), True).shape == (0, 2) and mask_iou(np.zeros((3, 1)), False).shape == (2, 0)
    assert mask_iou(np.zeros((2, 2)), False)[0, 0] == 0.0               # empty union


# ---- argument errors of the entry points ------------------------------------------------------------------------------------
def test_entry_points_refuse_bad_arguments_before_any_launch():
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)                               # never dereferenced: every call returns before a launch
    p = ctypes.addressof(buf)
    ok = dict(n_pix=16, A=1, B=1)
    bad = [dict(n_pix=0), dict(n_pix=-5), dict(n_pix=1 << 31), dict(A=-1), dict(B=-1), dict(B=256), dict(A=1 << 26, B=0),
           dict(A=(1 << 18), B=255)]
    for kw in bad:
        a = {**ok, **kw}
        rc = L.mx_label_pair_counts(p, p, a["n_pix"], a["A"], a["B"], p, p, None)
        assert rc < 0 and b"label_pair_counts" in L.mx_last_error(), kw
        rc = L.mx_mask_pair_counts(p, p, a["n_pix"], a["A"], a["B"], p, p, None)
        assert rc < 0 and b"mask_pair_counts" in L.mx_last_error(), kw
    for args in ((None, p, 16, 1, 1, p, p), (p, None, 16, 1, 1, p, p), (p, p, 16, 1, 1, None, p), (p, p, 16, 1, 1, p, None)):
        assert L.mx_label_pair_counts(*args, None) < 0 and b"label_pair_counts" in L.mx_last_error()
        assert L.mx_mask_pair_counts(*args, None) < 0 and b"mask_pair_counts" in L.mx_last_error()
    assert L.mx_mask_pair_counts(None, p, 16, 0, 1, None, p, None) < 0    # masks may be NULL with n = 0, the table may not


def test_host_wrappers_refuse_host_tensors_and_bad_shapes():
    import torch
    from muscle_amd import label_pair_counts, mask_pair_counts, pair_table
    from muscle_amd.ins_seg import InstanceLabels
    G = torch.zeros(4, 5, dtype=torch.uint8)
    with pytest.raises(_lib.MuscleHipError):
        pair_table(np.zeros((2, 4, 5), bool), G, 0)
    with pytest.raises(_lib.MuscleHipError):
        label_pair_counts(torch.zeros(4, 5, dtype=torch.int32), G, 1, 1)
    with pytest.raises(_lib.MuscleHipError):
        mask_pair_counts(torch.zeros(1, 4, 5, dtype=torch.bool), G, 1)
    with pytest.raises(ValueError):
        label_pair_counts(torch.zeros(4, 5, dtype=torch.float32), G, 1, 1)
    with pytest.raises(ValueError):
        pair_table(InstanceLabels(torch.zeros(4, 5, dtype=torch.int32), np.zeros(0, np.float32), np.zeros(0, np.int64),
                                  np.zeros(0, np.int32)), G.to(torch.int32), 0)
    with pytest.raises(ValueError):
        InsSegEval("cpu").add(np.zeros((1, 4, 5), bool), G.numpy(), G.numpy())   # a bare mask stack has no scores


# ---- scripts and documents --------------------------------------------------------------------------------------------------
def test_script_arguments():
    from muscle_amd import infer_irn, ins_eval
    a = ins_eval.parse_args(["--list", "l", "--ins_seg_dir", "d"])
    assert a.iou == [0.25, 0.5, 0.7, 0.75] and a.num_classes == 20 and a.voc12_root == "data/VOC2012"
    a = ins_eval.parse_args(["--list", "l", "--ins_seg_dir", "d", "--iou", "0.5", "--num_classes", "3", "--voc12_root", "v"])
    assert a.iou == [0.5] and a.num_classes == 3 and a.voc12_root == "v"
    base = ["--irn_weights_name", "w", "--cam_dir", "c"]
    assert infer_irn.parse_args(base).ins_eval == 0                                   # off by default
    assert infer_irn.parse_args(base + ["--ins_seg_out_dir", "i", "--ins_eval", "1"]).ins_eval == 1
    with pytest.raises(SystemExit):
        infer_irn.parse_args(base + ["--ins_eval", "1"])                              # nothing to evaluate without the instance path


def test_a_list_without_object_pngs_is_an_error_naming_the_first_missing_file(tmp_path):
    from muscle_amd import ins_eval
    for d in ("SegmentationClass", "SegmentationObject"):
        (tmp_path / d).mkdir()
    (tmp_path / "SegmentationClass" / "a.png").write_bytes(b"")
    (tmp_path / "SegmentationObject" / "a.png").write_bytes(b"")
    (tmp_path / "SegmentationClass" / "b.png").write_bytes(b"")
    ins_eval.check_gt_files(str(tmp_path), ["a"])
    with pytest.raises(FileNotFoundError, match="SegmentationObject/b.png"):
        ins_eval.check_gt_files(str(tmp_path), ["a", "b", "c"])


def test_lines_format():
    ev = InsSegEval("cpu", 2, (0.5, 0.75))
    ev.add_iou(np.array([[0.6]]), [0.5], [0], [0])
    lines = ev.lines()
    assert lines == ["0.5iou: {'ap': array([ 1., nan]), 'map': 1.0}", "0.75iou: {'ap': array([ 0., nan]), 'map': 0.0}"]


def test_documents_state_the_contract_and_the_unpinned_parity():
    import os
    from muscle_amd import ins_eval
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    read = lambda f: open(os.path.join(root, f)).read()  # noqa: E731
    design, integ, header = read("DESIGN.md"), read("INTEGRATION.md"), read("include/muscle_hip.h")
    for text in (ins_eval.__doc__, design, integ):
        assert "eval_instance_segmentation_voc" in text and "unpinned" in text
    assert "### Instance evaluation" in design and "python -m muscle_amd.ins_eval" in integ and "--ins_eval 1" in integ
    assert "python -m muscle_amd.ins_eval" in read("README.md") and "ins_eval_bench.txt" in read("profiles/README.md")
    assert "mx_label_pair_counts" in header and "mx_mask_pair_counts" in header and "2^26" in header
