"""muscle_amd.irn_sweep on the host: the numpy restatement tests/irn_sweep_ref.py against a brute-force argmax, the grid
validation, the command line, best()'s tie order, the two entry points' header signatures and the side-effect-free import.
Every comparison is of integers or bits."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_sweep_ref as SR  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def brute_counts(v, keys, gt, thresholds, K):
    """np.argmax over the dense [t, v_1 .. v_{K-1}] stack (absent channels 0; the first maximum wins), counted with bincount."""
    out = np.zeros((len(thresholds), K, 3), np.int64)
    H, W = gt.shape
    for i, t in enumerate(thresholds):
        stack = np.zeros((K, H, W), np.float32)
        stack[0] = np.float32(t)
        for j, k in enumerate(keys):
            stack[k + 1] = v[j]
        pred = np.argmax(stack, axis=0)
        ok = gt < 255
        out[i, :, 1] = np.bincount(pred[ok], minlength=K)[:K]
        out[i, :, 2] = np.bincount(gt[ok & (gt < K)], minlength=K)[:K]
        out[i, :, 0] = np.bincount(gt[ok & (pred == gt)], minlength=K)[:K]
    return out


def test_restatement_vs_brute_force_on_a_hand_built_case_with_ties():
    """2x3 pixels, classes 2 and 5 kept (K = 7).  Pixel (0,0): v == t exactly at t = 0.5 (background by the tie rule);
    (0,1): both channels 0 (background even at t = 0); (0,2): the two channels tie, the first wins; (1,0): value 1 (a tie at
    t = 1); (1,1): gt = 255, skipped; (1,2): gt = 6 has no prediction of its own class."""
    v = np.array([[[0.5, 0.0, 0.75], [1.0, 0.9, 0.25]],
                  [[0.25, 0.0, 0.75], [0.5, 0.1, 0.625]]], np.float32)
    keys = [2, 5]
    gt = np.array([[3, 0, 3], [3, 255, 6]], np.uint8)
    thr = [0.0, 0.25, 0.5, 0.625, 1.0]
    got = SR.counts_from_values(v, keys, gt, thr, 7)
    assert np.array_equal(got, brute_counts(v, keys, gt, thr, 7))
    lab = [SR.label_from_values(v, keys, t) for t in thr]
    assert lab[2][0, 0] == 0 and lab[1][0, 0] == 3                     # v == t is background, t below it is not
    assert all(l[0, 1] == 0 for l in lab)                             # v == 0 never beats t >= 0
    assert lab[0][0, 2] == 3 and lab[4][1, 0] == 0 and lab[3][1, 0] == 3 and lab[3][1, 2] == 0 and lab[2][1, 2] == 6
    assert got[0, :, 2].sum() == 5 and got[0, :, 1].sum() == 5          # five counted pixels, each predicted once
    nan = np.full_like(v, np.nan)                                       # an all-zero walk result: 0 / 0 everywhere
    assert all((SR.label_from_values(nan, keys, t) == 0).all() for t in thr)


def test_restatement_upsample_is_the_half_pixel_bilinear():
    """up4 against F.interpolate(scale 4, bilinear, align_corners=False) cropped: the same taps and weights (values within fp32
    round-off; the bits are the kernel's, which the GPU test compares), and exact on a constant map."""
    import torch.nn.functional as F
    rng = np.random.default_rng(3)
    for h, w, H, W in ((3, 4, 9, 14), (1, 2, 2, 3), (5, 5, 20, 20)):
        m = rng.random((h, w), dtype=np.float32)
        ref = F.interpolate(torch.from_numpy(m)[None, None], scale_factor=4, mode="bilinear", align_corners=False)[0, 0, :H, :W].numpy()
        assert float(np.abs(SR.up4(m, H, W) - ref).max()) <= 2e-7
        assert np.array_equal(SR.up4(np.full((h, w), 0.3, np.float32), H, W), np.full((H, W), 0.3, np.float32))
    x = np.array([3, 1.5, -2.25], np.float32)
    assert np.array_equal(SR._fma32(x, x, x), (x.astype(np.float64) * x + x).astype(np.float32))       # exact cases
    # (1 + 2^-12)^2 = 1 + 2^-11 + 2^-24 is an fp32 midpoint; + 2^-60 lies above it.  Rounding to fp64 first loses the 2^-60 and
    # the tie then goes to even, 1 + 2^-11: the fused result is the neighbour above.
    a, c = np.float32([1 + 2.0 ** -12]), np.float32([2.0 ** -60])
    assert (a.astype(np.float64) * a + c).astype(np.float32)[0] == np.float32(1 + 2.0 ** -11)
    assert SR._fma32(a, a, c)[0] == np.float32(1 + 2.0 ** -11 + 2.0 ** -23)


def test_grid_validation():
    from muscle_amd.irn_sweep import IrnSweep, check_grid
    from muscle_amd import indexing
    ok = dict(betas=(4, 10), exp_times=(0, 2, 4), thresholds=(0.0, 0.2, 1.0))
    assert check_grid(**ok) == ((4.0, 10.0), (0, 2, 4), (0.0, 0.2, 1.0))
    bad = [dict(exp_times=(2, 1)), dict(exp_times=(1, 1)), dict(exp_times=(13,)), dict(exp_times=(-1,)), dict(exp_times=(1.5,)),
           dict(exp_times=()), dict(thresholds=(-0.1, 0.2)), dict(thresholds=tuple(i / 100 for i in range(65))), dict(thresholds=()),
           dict(thresholds=(0.3, 0.2)), dict(betas=()), dict(betas=(0,)), dict(betas=(65,)), dict(betas=(8, 8)),
           dict(betas=(float("nan"),)), dict(num_cls=25), dict(num_cls=1)]
    for kw in bad:
        with pytest.raises(ValueError):
            check_grid(**dict(ok, **kw))
        with pytest.raises(ValueError):                                # the class refuses before it touches a device
            IrnSweep("cuda:0", **dict(ok, **kw))
    assert len(check_grid((8,), (0,), tuple(i / 100 for i in range(64)))[2]) == 64
    x, e = torch.zeros(1, 1, 4, 5), torch.zeros(1, 4, 5)
    for lst in ((2, 1), (3, 3), (13,), (), (0.5,)):
        with pytest.raises(ValueError):
            indexing.propagate_to_edge_multi(x, e, exp_times_list=lst)


def test_host_tensors_are_refused():
    from muscle_amd._lib import MuscleHipError
    from muscle_amd.irn_sweep import IrnSweep
    from muscle_amd import indexing
    with pytest.raises(MuscleHipError):
        indexing.propagate_to_edge_multi(torch.zeros(1, 1, 4, 5), torch.zeros(1, 4, 5), exp_times_list=(0, 1))
    sw = IrnSweep("cpu", (8,), (0,), (0.3,))
    with pytest.raises(MuscleHipError):
        sw.add_field(torch.zeros(1, 4, 5), {}, np.zeros((16, 20), np.uint8), 16, 20)
    with pytest.raises(MuscleHipError):
        sw.add_compact(None, np.zeros((16, 20), np.uint8))


def test_cli_parsing():
    from muscle_amd.irn_sweep import DEFAULT_BETAS, DEFAULT_EXP_TIMES, DEFAULT_THRESHOLDS, infer_irn_arguments, parse_args
    a = parse_args("--irn_weights_name W --cam_dir CAMS --voc12_root VOC --infer_list data/train.txt".split())
    assert (tuple(a.betas), tuple(a.exp_times), tuple(a.thresholds)) == (DEFAULT_BETAS, DEFAULT_EXP_TIMES, DEFAULT_THRESHOLDS)
    assert len(DEFAULT_THRESHOLDS) == 20 and a.gt_dir == os.path.join("VOC", "SegmentationClass") and a.out_table is None
    a = parse_args("--irn_weights_name W --cam_dir CAMS --voc12_root VOC --infer_list data/train.txt --betas 6 8 10 12 "
                   "--exp_times 4 5 6 7 8 --thresholds 0.15 0.25 0.35 --gt_dir GT --logfile F --out_table T.npy".split())
    assert a.betas == [6, 8, 10, 12] and a.exp_times == [4, 5, 6, 7, 8] and a.thresholds == [0.15, 0.25, 0.35]
    assert (a.gt_dir, a.logfile, a.out_table) == ("GT", "F", "T.npy")
    a = parse_args("--from_soft IRN_SOFT --voc12_root VOC --infer_list LIST --thresholds 0.2 0.3".split())
    assert a.from_soft == "IRN_SOFT" and a.thresholds == [0.2, 0.3]
    for bad in ("--cam_dir CAMS", "--from_soft S --cam_dir C", "--irn_weights_name W --cam_dir C --exp_times 8 4",
                "--irn_weights_name W --cam_dir C --exp_times 13", "--irn_weights_name W --cam_dir C --thresholds -0.1",
                "--from_soft S --thresholds 0.3 0.2"):
        with pytest.raises(SystemExit):
            parse_args(bad.split())
    assert infer_irn_arguments(10.0, 8, 0.35) == "--beta 10 --exp_times 8 --sem_seg_bg_thres 0.35 --walk stencil"
    from muscle_amd.infer_irn import parse_args as infer_args          # the string is a valid infer_irn command line
    b = infer_args(["--irn_weights_name", "W", "--cam_dir", "C"] + infer_irn_arguments(10.0, 8, 0.35).split())
    assert (b.beta, b.exp_times, b.sem_seg_bg_thres, b.walk) == (10, 8, 0.35, "stencil")


def test_script_names_a_missing_file_before_the_loop(tmp_path):
    import PIL.Image
    from muscle_amd.irn_sweep import main
    (tmp_path / "list.txt").write_text("a\nb\n")
    gt = tmp_path / "SegmentationClass"
    gt.mkdir()
    PIL.Image.fromarray(np.zeros((8, 8), np.uint8)).save(gt / "a.png")
    base = ["--voc12_root", str(tmp_path), "--infer_list", str(tmp_path / "list.txt")]
    with pytest.raises(FileNotFoundError, match="b.png"):               # ground truth, both modes; nothing was launched
        main(["--from_soft", str(tmp_path)] + base)
    PIL.Image.fromarray(np.zeros((8, 8), np.uint8)).save(gt / "b.png")
    with pytest.raises(FileNotFoundError, match="a.npy"):               # the CAM dict
        main(["--irn_weights_name", "W", "--cam_dir", str(tmp_path / "cams")] + base)


def test_best_breaks_ties_toward_the_lowest_grid_index():
    from muscle_amd.irn_sweep import IrnSweep, best_of
    m = np.zeros((2, 3, 4))
    m[0, 2, 1] = m[1, 0, 0] = m[0, 2, 3] = 5.0
    assert best_of(m) == (0, 2, 1)
    assert best_of(np.zeros((2, 3, 4))) == (0, 0, 0)
    sw = IrnSweep("cpu", (4, 10), (0, 2), (0.1, 0.2, 0.3), num_cls=3)
    assert sw.counts().shape == (2, 2, 3, 3, 3) and sw.counts().dtype == np.int64 and sw.mious().shape == (2, 2, 3)
    good = torch.tensor([[5, 5, 5], [5, 5, 5], [5, 5, 5]])               # IoU 1 in every class
    sw.table[1, 0, 1] = good
    sw.table[0, 1, 2] = good
    sw.table[1, 1, 0] = good
    miou, beta, et, t = sw.best()
    assert (beta, et, t) == (4.0, 2, 0.3) and abs(miou - 100.0) < 1e-6
    assert abs(sw.loglist(0, 1, 2)["mIoU"] - 100.0) < 1e-6 and sw.loglist(0, 0, 0)["mIoU"] == 0.0


def test_header_declares_the_two_entries_with_their_reference_lines():
    from muscle_amd._lib import HEADER_PATH, parse_header
    sigs = parse_header()
    assert sigs["mx_irn_walk_snap"] == "ppppiiipppiipipppp"
    assert sigs["mx_irn_sweep_confusion"] == "piipiipiipiippp"
    text = open(HEADER_PATH).read()
    assert "infer_irn.py:76-92" in text and "src/indexing.py:116-147" in text and "src/evaluation.py:36-50" in text


def test_entry_points_report_argument_errors():
    """Refused before any launch, with a message that names the entry (no GPU needed)."""
    import ctypes
    from muscle_amd import _lib
    L = _lib.lib()
    p = 4096                                                       # any non-null address: the checks come before the first use

    def snap(steps, **k):
        arr = (ctypes.c_int * len(steps))(*steps)
        return L.mx_irn_walk_snap(k.get("x", p), p, p, p, 4, 5, 5, p, p, p, 34, 1, arr, k.get("ns", len(steps)), p, p + 8, p, None)

    for steps, kw in (((1, 4, 2), {}), ((2, 2), {}), ((0, 1), {}), ((1, 4097), {}), (tuple(range(1, 15)), {}), ((1,), {"ns": 0}),
                      ((1, 2), {"x": None})):
        assert snap(steps, **kw) < 0 and b"irn_walk_snap" in L.mx_last_error(), (steps, kw)

    def sweep(**k):
        return L.mx_irn_sweep_confusion(k.get("rw", p), k.get("E", 2), k.get("Kp", 3), p, 4, 5, k.get("gt", p), k.get("H", 16), 20, p,
                                        k.get("nt", 5), k.get("K", 21), p, k.get("counts", p), None)

    for kw in ({"rw": None}, {"gt": None}, {"counts": None}, {"nt": 65}, {"nt": 0}, {"K": 25}, {"H": 17}, {"E": 14}, {"E": 0}, {"Kp": 21}):
        assert sweep(**kw) < 0 and b"irn_sweep_confusion" in L.mx_last_error(), kw


def test_module_imports_without_side_effects():
    code = ("import sys, muscle_amd.irn_sweep, torch\n"
            "bad = [m for m in ('cv2', 'pandas', 'tensorboardX') if m in sys.modules]\n"
            "assert not bad, bad\n"
            "assert not torch.cuda.is_initialized()\n"
            "import muscle_amd._lib as L\n"
            "assert L._lib is None\n"
            "import muscle_amd\n"
            "assert muscle_amd.IrnSweep is muscle_amd.irn_sweep.IrnSweep\n"
            "print('IMPORT-OK')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "IMPORT-OK" in r.stdout, r.stderr[-2000:]
    src = open(os.path.join(ROOT, "muscle_amd", "irn_sweep.py")).read()
    top = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
    assert not any(w in ln for ln in top for w in ("torch", "PIL", "_lib")), top
