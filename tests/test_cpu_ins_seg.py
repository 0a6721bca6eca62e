"""Instance pseudo-labels without a GPU.

Two kinds of test live here.  The ones that pin the YARDSTICK exercise only tests/ins_seg_ref.py, which by design imports nothing
from muscle_amd, so they pass with or without the feature: the restatement's labelling against scipy, the hand-worked 3x4 cases
of steps 2 and 6, the patterns, the properties of the shared test fields that keep the GPU cases discriminating, the finish
restatement and the seed of the 300-channel case.  The ones that pin the FEATURE fail without muscle_amd/ins_seg.py:
test_argument_refusals, test_instance_labels_container, test_script_arguments and test_header_and_documents."""
import os

import numpy as np
import pytest
import torch
from scipy import ndimage

import ins_seg_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- the restatement's component labelling ----------------------------------------------------------------------------------
@pytest.mark.parametrize("name", R.PATTERNS)
@pytest.mark.parametrize("shape", [(1, 1), (1, 70), (70, 1), (33, 65)], ids=str)
def test_components_equal_scipy(shape, name):
    lab = R.pattern(name, *shape, seed=5)
    root = R.label_components(lab)
    assert ((root < 0) == (lab == 0)).all()
    sc = np.zeros(shape, np.int64)                              # scipy labels one value at a time; stack the values' components
    for v in np.unique(lab[lab != 0]):
        part, k = ndimage.label(lab == v)                       # default structure: 4-connectivity
        sc = np.where(part > 0, part + sc.max(), sc)
    assert np.array_equal(R.renumber_by_first_pixel(root + 1), R.renumber_by_first_pixel(sc))
    idx = np.arange(lab.size).reshape(shape)
    for r in np.unique(root[root >= 0]):                        # the id is the first raster pixel
        assert idx[root == r].min() == r


def test_patterns_are_what_they_claim():
    sp = R.pattern("spiral", 33, 65)
    root = R.label_components(sp)
    assert len(np.unique(root[root >= 0])) == 1 and sp.sum() > 33 * 65 // 3
    noise = R.pattern("noise", 33, 65, seed=5)
    sizes = np.bincount(R.renumber_by_first_pixel(R.label_components(noise) + 1).ravel())[1:]
    assert sizes.max() > 200 and len(sizes) > 20                # a winding giant component and many small ones
    assert set(np.unique(R.pattern("three", 33, 65, seed=5))) == {0, 1, 2, 3}


# ---- hand-worked 3x4 cases --------------------------------------------------------------------------------------------------
def test_step2_by_hand():
    weak = np.array([[1, 1, 0, 1],
                     [0, 0, 0, 1],
                     [1, 0, 0, 0]], bool)
    dp = np.zeros((2, 3, 4), np.float32)
    dp[0][~weak] = 3.0                                          # |dp| = 3 >= 2.5: not weak
    dp[1][0, 0] = 2.4                                           # |dp| = 2.4 < 2.5: weak
    assert np.array_equal(R.weak_map(dp), weak)
    assert np.array_equal(R.label_components(weak.astype(np.int32)), [[0, 0, -1, 3], [-1, -1, -1, 3], [8, -1, -1, -1]])
    cy = np.array([[0, 0, 0, 1], [2, 1, 1, 1], [2, 2, 1, 0]], np.int32)
    cx = np.array([[0, 1, 3, 3], [0, 1, 3, 3], [0, 0, 2, 0]], np.int32)
    # ids at the centroids: 0 0 3 3 / 8 -1 3 3 / 8 8 -1 0 -> background first, then ascending
    cluster, I = R.cluster_centroids(np.stack([cy, cx]), dp)
    assert I == 4 and np.array_equal(cluster, [[1, 1, 2, 2], [3, 0, 2, 2], [3, 3, 0, 1]])
    cy[1, 1], cx[1, 1], cy[2, 2], cx[2, 2] = 0, 0, 2, 0         # no centroid on a non-weak pixel: no background id
    cluster, I = R.cluster_centroids(np.stack([cy, cx]), dp)
    assert I == 3 and np.array_equal(cluster, [[0, 0, 1, 1], [2, 0, 1, 1], [2, 2, 2, 0]])
    x = R.split_instances(np.arange(24, dtype=np.float32).reshape(2, 3, 4), cluster, I)
    assert x.shape == (6, 3, 4) and x[4, 0, 2] == 14 and x[4, 0, 0] == 0 and x[0, 2, 3] == 11 and x[3, 0, 0] == 12


def test_step6_by_hand():
    label = np.array([[2, 2, 0, 1],
                      [0, 2, 0, 1],
                      [3, 0, 2, 2]], np.int32)
    win = np.arange(12, dtype=np.float32).reshape(3, 4) / 16
    s = R.segments(label, win, (3, 11), 2)                      # K = 2 classes (3, 11), I = 2: labels 1, 2 -> class 3; 3, 4 -> class 11
    assert np.array_equal(s["seg_map"], [[2, 2, 0, 1], [0, 2, 0, 1], [4, 0, 3, 3]])      # (label, first pixel): (1,3) (2,0) (2,10) (3,8)
    assert s["cls"].tolist() == [3, 3, 3, 11] and s["area"].tolist() == [2, 3, 2, 1]
    assert s["score"].tolist() == [7 / 16, 5 / 16, 11 / 16, 8 / 16]                       # 12 pixels: no area is below 0.12
    assert s["cls"].dtype == np.int64 and s["area"].dtype == np.int32 and s["score"].dtype == np.float32
    big = np.zeros((10, 20), np.int32)                          # 200 pixels: an area of 1 is below 2.0, an area of 2 is not
    big[0, 0], big[5, 5:7], big[9, 19] = 1, 1, 4
    w = np.full((10, 20), 0.5, np.float32)
    s = R.segments(big, w, (0, 19), 2)
    assert s["area"].tolist() == [1, 2, 1] and s["score"].tolist() == [0.0, 0.5, 0.0] and s["cls"].tolist() == [0, 0, 19]
    none = R.segments(np.zeros((3, 4), np.int32), win, (3,), 1)
    assert none["score"].shape == (0,) and none["seg_map"].sum() == 0


# ---- the test fields --------------------------------------------------------------------------------------------------------
def test_swirl_field_properties():
    """What makes the GPU centroid and end-to-end cases discriminating: several clusters with a background, and an iteration
    that turns a last-bit difference of the products into other centroids."""
    dp = R.attractors(47, 63, 0, swirl=True)
    cent = R.find_centroids(dp, 100)
    root = R.label_components(R.weak_map(dp).astype(np.int32))
    ids = root[cent[0], cent[1]]
    cluster, I = R.cluster_centroids(cent, dp)
    moved = int((cent != R.find_centroids(dp, 100, products64=True)).any(0).sum())
    print(f"[ins_seg] swirl 47x63: I={I}, background pixels {(ids < 0).sum()}, fp64 products move {moved} centroids")
    assert I >= 4 and (ids < 0).any() and (cluster == 0).sum() == (ids < 0).sum()
    assert moved >= 1
    out = R.find_centroids(R.attractors(24, 31, 1, outward=True), 1)
    assert out.min() == 0 and out[0].max() == 23 and out[1].max() == 30          # the clip holds the pushed border pixels


def test_finish_restatement():
    rw = np.zeros((2, 2, 2), np.float32)
    rw[1, 0, 0] = 2.0
    label, win, vmax, margin = R.finish(rw, 8, 8, 0.25)
    assert vmax == 2.0 and label[0, 0] == 2 and win[0, 0] == 1.0 and label[7, 7] == 0 and win[7, 7] == np.float32(0.25)
    label, win, vmax, _ = R.finish(np.zeros((3, 2, 2), np.float32), 5, 7, 0.25)
    assert vmax == 0 and not label.any()
    c = R.CASE4                                                 # the seed of the 300-channel GPU case meets its own cap
    _, _, _, margin = R.finish(R.walk_maps(c["C"], c["h"], c["w"], c["seed"]), c["H"], c["W"], c["bg"])
    assert (margin <= 1e-6).mean() <= 0.01


# ---- the interface ----------------------------------------------------------------------------------------------------------
def test_argument_refusals():
    import muscle_amd
    from muscle_amd import ins_seg
    from muscle_amd._lib import MuscleHipError
    dp = torch.zeros(2, 3, 4)
    cent = torch.zeros(2, 3, 4, dtype=torch.int32)
    for bad in (dp.double(), torch.zeros(3, 3, 4), torch.zeros(3, 4), np.zeros((2, 3, 4), np.float32)):
        with pytest.raises(ValueError, match="dp must be"):
            muscle_amd.find_centroids(bad)
    for it in (-1, 2.5, True):
        with pytest.raises(ValueError, match="iterations"):
            muscle_amd.find_centroids(dp, it)
    for bad in (cent.long(), torch.zeros(2, 3, 5, dtype=torch.int32)):
        with pytest.raises(ValueError, match="centroids must be"):
            muscle_amd.cluster_centroids(bad, dp)
    for th in (0, -1.0, float("nan"), "2.5", None):
        with pytest.raises(ValueError, match="thres"):
            muscle_amd.cluster_centroids(cent, dp, th)
    for bad in (torch.zeros(3, 4), torch.zeros(1, 3, 4, dtype=torch.int32), torch.zeros(0, 4, dtype=torch.int32)):
        with pytest.raises(ValueError, match="label must be"):
            muscle_amd.connected_components(bad)
    edge, cam = torch.zeros(1, 3, 4), {5: np.zeros((12, 16), np.float32)}
    f = ins_seg.instances_from_field
    with pytest.raises(ValueError, match="method"):
        f(edge, dp, cam, 12, 16, method="sparse")
    with pytest.raises(ValueError, match="no class"):
        f(edge, dp, {}, 12, 16)
    for bg in (-0.1, "0.25", None):
        with pytest.raises(ValueError, match="bg_thres"):
            f(edge, dp, cam, 12, 16, bg_thres=bg)
    with pytest.raises(ValueError, match="iterations"):
        f(edge, dp, cam, 12, 16, iterations="3")
    with pytest.raises(ValueError, match="down must be"):
        f(edge, dp, cam, 12, 16, down=torch.zeros(2, 3, 4))
    with pytest.raises(ValueError, match="iterations"):
        f(edge, dp, cam, 12, 16, iterations=-3)
    with pytest.raises(ValueError, match="dp_thres"):
        f(edge, dp, cam, 12, 16, dp_thres=0)
    with pytest.raises(ValueError, match="CAM of class 5"):
        f(edge, dp, cam, 12, 15)

    class Training:
        training = True
    with pytest.raises(ValueError, match="eval"):
        muscle_amd.infer_irn_instances(Training(), torch.zeros(2, 3, 12, 16), cam)
    # well-formed arguments on the host: there is no CPU path
    with pytest.raises(MuscleHipError):
        muscle_amd.find_centroids(dp)
    with pytest.raises(MuscleHipError):
        muscle_amd.connected_components(torch.zeros(3, 4, dtype=torch.int32))


def test_instance_labels_container():
    from muscle_amd import InstanceLabels
    sm = torch.tensor([[0, 1, 1], [2, 0, 1]], dtype=torch.int32)
    ins = InstanceLabels(sm, np.array([0.5, 0.0], np.float32), np.array([3, 11]), np.array([3, 1], np.int32))
    d = ins.to_irn_dict()
    assert len(ins) == 2 and sorted(d) == ["class", "mask", "score"]
    assert d["mask"].dtype == bool and np.array_equal(d["mask"], [[[0, 1, 1], [0, 0, 1]], [[0, 0, 0], [1, 0, 0]]])
    empty = InstanceLabels(torch.zeros(2, 3, dtype=torch.int32), np.zeros(0, np.float32), np.zeros(0, np.int64), np.zeros(0, np.int32), 0.0)
    d = empty.to_irn_dict()
    assert d["score"].shape == (0,) and d["mask"].shape == (0, 2, 3) and d["class"].shape == (0,)


def test_script_arguments():
    from muscle_amd.infer_irn import parse_args
    base = ["--irn_weights_name", "w.pth", "--cam_dir", "c"]
    a = parse_args(base)
    assert a.ins_seg_out_dir is None and (a.ins_seg_bg_thres, a.ins_refine_iters, a.ins_dp_thres) == (0.25, 300, 2.5)
    a = parse_args(base + ["--ins_seg_out_dir", "d", "--ins_seg_bg_thres", "0.3", "--ins_refine_iters", "10", "--ins_dp_thres", "2"])
    assert (a.ins_seg_out_dir, a.ins_seg_bg_thres, a.ins_refine_iters, a.ins_dp_thres) == ("d", 0.3, 10, 2.0)


def test_header_and_documents():
    from muscle_amd import _lib
    sigs = _lib.parse_header()
    for name in ("mx_irn_centroids", "mx_irn_weak", "mx_ccl_ws", "mx_ccl", "mx_id_mark", "mx_id_rank", "mx_id_apply",
                 "mx_irn_ins_split", "mx_irn_up_max", "mx_irn_ins_finish", "mx_seg_stats", "mx_seg_map"):
        assert name in sigs, name
    assert sigs["mx_ccl"] == "piippp" and sigs["mx_irn_centroids"] == "piiipp" and "mx_ccl_ws" in _lib.LONG_RETURNS
    read = lambda f: open(os.path.join(ROOT, f)).read()
    integ = read("INTEGRATION.md")
    assert "ins_seg_out_dir" in integ and "unpinned" in integ and "skimage" in integ
    assert "ins_seg_out_dir" in read("README.md")
    assert "Instance pseudo-labels" in read("DESIGN.md")
    assert "ins_seg_bench.txt" in read(os.path.join("profiles", "README.md"))
    src = read(os.path.join("muscle_amd", "csrc", "irn_ins.hip"))
    for word in ("atomicAdd(&area", "atomicMax(&score_bits", "atomicMin(&par"):
        assert word in src
    assert "float" not in "".join(ln for ln in src.splitlines() if "atomic" in ln and "(" in ln and "__float_as_uint" not in ln and "//" not in ln)
