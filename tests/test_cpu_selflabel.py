"""Host side of the class-balanced self-training labels (muscle_amd.selflabel): the confidence code's landmarks, the threshold
rule on hand-built histograms, the quality curve against a brute-force count, the statistics files, the script refusals, the
argument checks and the places that state the rule.  No kernel is launched here."""
import os

import numpy as np
import pytest
import torch

import selflabel_ref as R
from muscle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
F = np.float32


def _codes(vals):
    from muscle_amd import selflabel as SL
    a = np.array(vals, dtype=np.float32)
    got, ref = SL.code_of(a), R.code(a)
    assert got.dtype == np.uint8 and np.array_equal(got, ref) and np.array_equal(R.code_fast(a), ref)
    return got.tolist()


def test_code_landmarks():
    one = F(1.0)
    assert _codes([1.0]) == [0]
    assert _codes([one - F(2.0 ** -24)]) == [1]                        # the largest fp32 below 1: u = 2^-24
    assert _codes([0.5]) == [185]
    assert _codes([2.0 ** -24, 1e-3]) == [192, 192]                    # just above 0, where 1 - conf still rounds below 1
    assert _codes([1e-30, 1e-45]) == [193, 193]                        # 1 - conf rounds to 1
    assert _codes([0.0, -0.0]) == [193, 193]
    assert _codes([-1e-3, -5.0, -np.inf]) == [193, 193, 193]
    assert _codes([np.nan]) == [255]
    assert _codes([np.nextafter(one, F(2)), 1.5, 1e30, np.inf]) == [0, 0, 0, 0]
    for e in range(1, 25):                                             # conf = 1 - 2^-e: exponent 127 - e, mantissa 0
        assert _codes([one - F(2.0 ** -e)]) == [(127 - e) * 8 - 823]
    assert _codes([0.25, 0.125]) == [189, 191]                         # u = 0.75 (mantissa .100), 0.875 (.110)


def test_code_is_monotone_and_stays_in_range():
    from muscle_amd import selflabel as SL
    g = np.random.default_rng(0)
    conf = np.concatenate([1.0 - np.exp(g.uniform(np.log(2.0 ** -26), 0.0, 20000)), g.uniform(-0.5, 1.5, 2000),
                           1.0 - 2.0 ** -np.arange(0, 30.0, 0.125), [0.0, 1.0]]).astype(np.float32)
    conf = np.sort(conf)
    code = SL.code_of(conf)
    assert np.array_equal(code, R.code_fast(conf)) and np.array_equal(code[::37], R.code(conf[::37]))
    assert np.all(np.diff(code.astype(np.int64)) <= 0)                 # non-increasing in conf
    assert code.max() == 193 and code.min() == 0 and len(np.unique(code)) > 150      # nothing above 193; the scale is used
    # below 2^-21 fp32 confidences are too coarse for every code: 1 - conf is a multiple of 2^-24, so 2..8 never occur
    assert not np.isin(code, np.arange(2, 9)).any()
    assert SL.code_of(0.5).shape == () and int(SL.code_of(0.5)) == 185


def test_code_interval_brackets_its_code():
    from muscle_amd import selflabel as SL
    assert SL.code_interval(0) == (1.0, np.inf) and SL.code_interval(193) == (-np.inf, 0.0)
    assert all(np.isnan(SL.code_interval(c)).all() for c in (194, 254, 255))
    assert SL.code_interval(185) == (0.4375, 0.5) and SL.code_interval(1) == (1.0 - 1.125 * 2.0 ** -24, 1.0)
    for c in range(1, 193):
        lo, hi = SL.code_interval(c)
        assert lo < hi and (c == 192 or SL.code_interval(c + 1)[1] == lo)
        if c >= 25:                                                    # from u = 2^-21 on both edges are fp32 confidences
            assert int(SL.code_of(F(hi))) == c and int(SL.code_of(F(lo))) == c + 1        # hi belongs to the code, lo to the next


def _hist(K=3):
    return np.zeros((K, 256), dtype=np.int64)


def test_thresholds_on_hand_built_histograms():
    from muscle_amd import selflabel as SL
    h = _hist(4)
    h[1, [3, 10, 40, 192]] = [5, 5, 10, 20]                            # n = 40, cumulative 5, 10, 20, 40
    h[2, [0, 193]] = [1, 9]
    h[3, [7, 255]] = [2, 8]                                            # 8 NaN pixels: counted in n, never reachable
    t = SL.thresholds(h, 0.25)
    assert t.dtype == np.uint8 and t.shape == (4,)
    assert t.tolist() == [0, 10, 193, 193]                             # empty class 0; need = 10 lands exactly on code 10
    assert SL.thresholds(h, 0.26).tolist()[1] == 40                    # need = 11: the next code, all of its ties kept
    assert SL.thresholds(h, 0.125).tolist()[1] == 3 and SL.thresholds(h, 1e-9).tolist() == [0, 3, 0, 7]     # need >= 1
    assert SL.thresholds(h, 0.1).tolist()[2] == 0 and SL.thresholds(h, 0.11).tolist()[2] == 193
    assert SL.thresholds(h, 1.0).tolist() == [0, 192, 193, 193]        # portion 1.0: everything but the NaN pixels
    assert SL.thresholds(h, 0.2).tolist()[3] == 7 and SL.thresholds(h, 0.21).tolist()[3] == 193             # capped at 193
    # the min_conf cap: code_of(0.5) = 185, code_of(1 - 2^-10) = 113
    assert SL.thresholds(h, 1.0, min_conf=0.5).tolist() == [0, 185, 185, 185]
    assert SL.thresholds(h, 0.25, min_conf=0.5).tolist() == [0, 10, 185, 185]
    assert SL.thresholds(h, 1.0, min_conf=1.0 - 2.0 ** -10).tolist() == [0, 113, 113, 113]
    assert SL.thresholds(h, 1.0, min_conf=0.0).tolist() == SL.thresholds(h, 1.0).tolist()
    assert SL.thresholds(h, 1.0, min_conf=1.0).tolist() == [0, 0, 0, 0]
    # per-class portions
    assert SL.thresholds(h, [0.5, 0.125, 0.1, 1.0]).tolist() == [0, 3, 0, 193]
    # the ceil is taken of the float64 product: 0.07 * 100 = 7.000000000000001 -> need 8
    h2 = _hist(1)
    h2[0, :100] = 1
    assert 0.07 * 100 > 7 and SL.thresholds(h2, 0.07).tolist() == [7] and SL.thresholds(h2, 0.5).tolist() == [49]
    g = np.random.default_rng(5)
    for _ in range(20):
        hr = g.integers(0, 4, (5, 256)) * (g.random((5, 256)) < 0.1)
        hr[:, 194:255] = 0
        hr[g.integers(0, 5)] = 0
        for p in (0.01, 0.3, 0.5, 1.0, g.random(5) * 0.99 + 0.01):
            mc = None if g.random() < 0.5 else float(g.random())
            assert np.array_equal(SL.thresholds(hr, p, mc), R.thresholds(hr, p, mc))


def test_threshold_arguments():
    from muscle_amd import selflabel as SL
    h = _hist(3)
    for p in (0.0, -0.1, 1.0001, np.nan, [0.5, 0.5], [0.5, 0.0, 0.5]):
        with pytest.raises(ValueError, match="portion"):
            SL.thresholds(h, p)
    for bad in (np.zeros((3, 255), np.int64), np.zeros((25, 256), np.int64), np.zeros((3, 256), np.float32), np.zeros(256, np.int64),
                -np.ones((3, 256), np.int64)):
        with pytest.raises(ValueError):
            SL.thresholds(bad, 0.5)
    with pytest.raises(ValueError, match="min_conf"):
        SL.thresholds(h, 0.5, min_conf=1.5)
    with pytest.raises(ValueError):
        SL.quality_curve(h, _hist(4), h, [0.5])


def test_curve_against_a_brute_force_count():
    from muscle_amd import selflabel as SL
    g = np.random.default_rng(7)
    K, n = 5, 4000
    label = g.choice([0, 1, 2, 4], size=n).astype(np.uint8)            # class 3 is empty
    conf = (1.0 - np.exp(g.uniform(np.log(2.0 ** -20), 0.0, n))).astype(np.float32)
    conf[::97] = np.nan
    code = R.code_fast(conf)
    gt = np.where(g.random(n) < 0.7, label, g.choice([0, 1, 2, 3, 4, 9], size=n)).astype(np.uint8)
    gt[g.random(n) < 0.2] = 255
    gt[label == 4] = 255                                               # class 4 keeps no valid pixel
    hist, val, hit = R.tables(label, code, gt, K)
    portions = [0.1, 0.25, 0.5, 0.9, 1.0]
    cv = SL.quality_curve(hist, val, hit, portions)
    rows = R.curve_brute(label, code, gt, K, portions)
    for i, (kept, total, kv, kh) in enumerate(rows):
        assert np.array_equal(cv["tcode"][i], R.thresholds(hist, portions[i]))
        assert np.array_equal(cv["kept"][i], kept) and np.array_equal(cv["total"], total)
        assert np.array_equal(cv["val"][i], kv) and np.array_equal(cv["hit"][i], kh)
        assert np.all(kept >= np.minimum(hist[:, :194].sum(1), np.ceil(portions[i] * total)))   # at least the portion, NaN pixels apart
        for c in range(K):
            assert (np.isnan(cv["coverage"][i, c]) and total[c] == 0) or cv["coverage"][i, c] == kept[c] / total[c]
            assert (np.isnan(cv["precision"][i, c]) and kv[c] == 0) or cv["precision"][i, c] == kh[c] / kv[c]
        assert cv["coverage_all"][i] == kept.sum() / total.sum()
        on = kv > 0
        assert on.tolist() == [True, True, True, False, False]
        assert cv["mean_precision"][i] == np.mean(kh[on] / kv[on])
    assert cv["coverage"].dtype == np.float64 and cv["kept"].dtype == np.int64
    assert len(SL.curve_lines(cv)) == 1 + len(portions)
    empty = SL.quality_curve(_hist(2), _hist(2), _hist(2), [0.5])      # nothing counted: nan, not a division error
    assert np.isnan(empty["coverage_all"]).all() and np.isnan(empty["mean_precision"]).all()


def test_stats_files_sum(tmp_path):
    from muscle_amd import selflabel as SL
    g = np.random.default_rng(9)
    parts = []
    for i in range(3):
        st = SL.ConfStats("cpu", 7)                                    # on the host the tables and the files work; the kernels do not
        t = g.integers(0, 2 ** 40, (3, 7, 256))
        st._t.copy_(torch.from_numpy(t))
        st.save(str(tmp_path / f"s{i}.npz"))
        parts.append(t)
        with np.load(tmp_path / f"s{i}.npz", allow_pickle=False) as z:
            assert sorted(z.files) == ["hist", "hit", "val", "version"] and z["hist"].dtype == np.int64
    one = SL.ConfStats.load(str(tmp_path / "s1.npz"))
    assert one.num_cls == 7 and all(np.array_equal(a, b) for a, b in zip(one.tables(), parts[1]))
    tot = SL.ConfStats.load(*(str(tmp_path / f"s{i}.npz") for i in range(3)))
    for a, b in zip(tot.tables(), sum(parts)):
        assert a.dtype == np.int64 and a.shape == (7, 256) and np.array_equal(a, b)
    SL.ConfStats("cpu", 5).save(str(tmp_path / "k5.npz"))
    with pytest.raises(ValueError, match="classes"):
        SL.ConfStats.load(str(tmp_path / "s0.npz"), str(tmp_path / "k5.npz"))
    np.savez(tmp_path / "other.npz", hist=parts[0][0])
    with pytest.raises(ValueError, match="statistics"):
        SL.ConfStats.load(str(tmp_path / "other.npz"))
    with pytest.raises(ValueError):
        SL.ConfStats.load()
    with pytest.raises(ValueError):
        SL.ConfStats("cpu", 25)


def test_device_calls_check_their_arguments():
    """Shape, dtype and K raise ValueError before any launch; host tensors raise MuscleHipError."""
    from muscle_amd import selflabel as SL
    prob = torch.rand(3, 4, 5)
    u8 = torch.zeros(4, 5, dtype=torch.uint8)
    for bad in (prob.double(), prob[0], torch.rand(25, 4, 5), torch.rand(0, 4, 5), prob.numpy()):
        with pytest.raises(ValueError):
            SL.conf_code(bad)
    with pytest.raises(ValueError, match="gt"):
        SL.conf_code(prob, gt=torch.zeros(5, 4, dtype=torch.uint8))
    with pytest.raises(ValueError, match="gt"):
        SL.conf_code(prob, gt=u8.int())
    with pytest.raises(ValueError, match="classes"):
        SL.conf_code(prob, stats=SL.ConfStats("cpu", 4))
    with pytest.raises(ValueError):
        SL.ConfStats("cpu", 3).add_coded(u8, u8[:3])
    with pytest.raises(ValueError):
        SL.ConfStats("cpu", 3).add_coded(u8.float(), u8)
    for tc in (np.zeros(3, np.int64), np.zeros((3, 1), np.uint8), np.zeros(25, np.uint8), np.zeros(0, np.uint8), torch.zeros(3)):
        with pytest.raises(ValueError):
            SL.select(u8, u8, tc)
    with pytest.raises(ValueError):
        SL.select(u8, u8[:2], np.zeros(3, np.uint8))
    with pytest.raises(_lib.MuscleHipError):
        SL.conf_code(prob)
    with pytest.raises(_lib.MuscleHipError):
        SL.ConfStats("cpu", 3).add(prob, u8)
    with pytest.raises(_lib.MuscleHipError):
        SL.ConfStats("cpu", 3).add_coded(u8, u8)
    with pytest.raises(_lib.MuscleHipError):
        SL.select(u8, u8, np.zeros(3, np.uint8))


def test_script_arguments_and_refusals(tmp_path, capsys):
    from muscle_amd import infer_seg, selflabel as SL
    base = ["--weights", "w.pth"]
    assert infer_seg.parse_args(base).out_conf is None
    a = infer_seg.parse_args(base + ["--out_seg", "S", "--out_conf", "C"])
    assert (a.out_seg, a.out_conf, a.crf) == ("S", "C", 0)
    assert infer_seg.parse_args(base + ["--out_seg", "S", "--out_conf", "C", "--crf", "2", "--cls_dir", "L"]).out_conf == "C"
    for bad, word in ((["--out_conf", "C"], "--out_seg"), (["--out_seg", "S", "--out_conf", "C", "--cls_dir", "L"], "--crf 2")):
        with pytest.raises(SystemExit):
            infer_seg.parse_args(base + bad)
        assert word in capsys.readouterr().err
    sel = ["select", "--seg_dir", "S", "--conf_dir", "C", "--out_dir", "O"]
    a = SL.parse_args(sel + ["--portion", "0.5"])
    assert (a.cmd, a.seg_dir, a.conf_dir, a.out_dir, a.portion, a.stats, a.min_conf, a.list, a.gt_dir) == \
        ("select", "S", "C", "O", 0.5, None, 0.0, None, None)
    a = SL.parse_args(sel + ["--portion", "1.0", "--stats", "a.npz", "b.npz", "--min_conf", "0.9", "--list", "l.txt", "--gt_dir", "G"])
    assert (a.portion, a.stats, a.min_conf, a.list, a.gt_dir) == (1.0, ["a.npz", "b.npz"], 0.9, "l.txt", "G")
    for bad in (sel, sel + ["--portion", "0"], sel + ["--portion", "1.5"], sel + ["--portion", "0.5", "--min_conf", "2"],
                sel + ["--portion", "0.5", "--num_classes", "25"], ["--portion", "0.5"]):
        with pytest.raises(SystemExit):
            SL.parse_args(bad)
    capsys.readouterr()
    # a missing file is an error that names it, raised before the loop (and before anything touches the device)
    import PIL.Image
    for d in ("S", "C"):
        (tmp_path / d).mkdir()
    for nm in ("a", "b"):
        PIL.Image.fromarray(np.zeros((3, 4), np.uint8), "L").save(tmp_path / "S" / f"{nm}.png")
    PIL.Image.fromarray(np.zeros((3, 4), np.uint8), "L").save(tmp_path / "C" / "a.png")
    args = SL.parse_args(["select", "--seg_dir", str(tmp_path / "S"), "--conf_dir", str(tmp_path / "C"), "--out_dir",
                          str(tmp_path / "O"), "--portion", "0.5"])
    with pytest.raises(FileNotFoundError, match="b.png"):
        SL.run_select(args)
    assert not (tmp_path / "O").exists()


def test_package_exports():
    import muscle_amd
    from muscle_amd import selflabel as SL
    for name in ("conf_code", "ConfStats", "thresholds", "quality_curve", "select", "code_of", "code_interval"):
        assert getattr(muscle_amd, name) is getattr(SL, name)


RULE = "(bits(u) >> 20) - 823"


def test_header_and_documents_state_the_rule():
    sigs = _lib.parse_header()
    assert sigs.get("mx_conf_code") == "piiippppppp"
    assert sigs.get("mx_code_hist") == "ppplipppp"
    assert sigs.get("mx_conf_select") == "ppplippp"
    texts = {"header": open(_lib.HEADER_PATH).read(), "kernel": open(os.path.join(ROOT, "muscle_amd", "csrc", "selflabel.hip")).read()}
    for doc in ("DESIGN.md", "INTEGRATION.md"):
        texts[doc] = open(os.path.join(ROOT, doc)).read()
    for where, text in texts.items():
        flat = " ".join(text.replace(" * ", " ").replace("// ", " ").split())
        for words in (RULE, "1.0f - conf", "NaN", "255", "193", "first maximum"):
            assert words in flat, (where, words)
    assert "Self-training labels" in texts["DESIGN.md"]
    readme = open(os.path.join(ROOT, "README.md")).read()
    assert "muscle_amd.selflabel select" in readme and "--out_conf" in readme


def test_entry_points_refuse_bad_arguments_before_any_launch():
    import ctypes
    LL = _lib.lib()
    word = ctypes.c_longlong(0)
    p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    for args in ((None, 21, 4, 4, p, p, None, p, None, None), (p, 21, 4, 4, None, p, None, p, None, None),
                 (p, 21, 4, 4, p, p, None, None, None, None), (p, 0, 4, 4, p, p, None, p, None, None),
                 (p, 25, 4, 4, p, p, None, p, None, None), (p, 21, 0, 4, p, p, None, p, None, None),
                 (p, 21, 65536, 32768, p, p, None, p, None, None),                     # H*W = 2^31
                 (p, 21, 4, 4, p, p, p, p, None, None), (p, 21, 4, 4, p, p, None, p, p, p), (p, 21, 4, 4, p, p, p, p, p, None)):
        assert LL.mx_conf_code(*args, None) < 0, args
        assert b"conf_code" in LL.mx_last_error()
    for args in ((None, p, None, 4, 21, p, None, None), (p, p, None, 0, 21, p, None, None), (p, p, None, 2 ** 31, 21, p, None, None),
                 (p, p, None, 4, 25, p, None, None), (p, p, p, 4, 21, p, None, p), (p, p, None, 4, 21, None, None, None)):
        assert LL.mx_code_hist(*args, None) < 0, args
        assert b"code_hist" in LL.mx_last_error()
    for args in ((None, p, p, 4, 21, p, p), (p, p, None, 4, 21, p, p), (p, p, p, 4, 21, p, None), (p, p, p, 0, 21, p, p),
                 (p, p, p, 2 ** 31, 21, p, p), (p, p, p, 4, 0, p, p), (p, p, p, 4, 25, p, p)):
        assert LL.mx_conf_select(*args, None) < 0, args
        assert b"conf_select" in LL.mx_last_error()
