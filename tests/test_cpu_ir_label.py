"""Host side of IR-label generation (no kernel is launched): the header declares mx_ir_label_ws / mx_ir_label / mx_crf_label and
the library exports them, argument errors come back negative before any launch, combine_conf against a hand-written table, the
label unary against crf_ref.unary of a one-hot map, the script module imports cleanly, and tests/golden/ir_label.npz is what the
fp64 restatement (ir_label_ref.py) gives."""
import ctypes
import inspect
import os
import subprocess
import sys

import numpy as np
import pytest

import crf_ref as R
import ir_label_ref as IR
from muscle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "ir_label.npz")
ENTRIES = ("mx_ir_label_ws", "mx_ir_label", "mx_crf_label")


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_ir_label_ws"] == "iii" and "mx_ir_label_ws" in _lib.LONG_RETURNS
    assert sigs["mx_ir_label"] == "pppiiiffifffffffippppp"
    assert sigs["mx_crf_label"] == "ppiiiifffffffpppp"
    text = open(_lib.HEADER_PATH).read()
    assert text.count("src/imutils.py:477-491") >= 3           # every entry cites the reference
    if not os.path.exists(_lib.LIB_PATH):
        from muscle_amd import _build
        _build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_workspace_bytes():
    L = _lib.lib()
    n = L.mx_ir_label_ws(3, 375, 500)
    assert n >= 375 * 500 * (4 * (3 * 32 + 2 + 4) + 4) and n % 16 == 0      # Q x 2, the message, normalisers, colours, four maps
    assert L.mx_ir_label_ws(2, 1, 1) > 0 and L.mx_ir_label_ws(21, 4, 4) > 0
    assert L.mx_ir_label_ws(2, 7, 9) == L.mx_ir_label_ws(21, 7, 9)           # one workspace per image size
    for args in ((1, 4, 4), (0, 4, 4), (22, 4, 4), (3, 0, 4), (3, 4, 0), (3, -1, 4)):
        assert L.mx_ir_label_ws(*args) < 0, args
        assert b"ir_label_ws" in L.mx_last_error()


def test_bad_arguments_before_any_launch():
    """rc < 0 with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    ok = dict(rgb=p, cams=p, keys=p, C=3, H=4, W=4, fg=0.3, bg=0.05, t=10, gt_prob=0.7, sxy_g=3.0, w_g=3.0, sxy_b=50.0, srgb=5.0,
              w_b=10.0, trunc=4.0, fused=1, ws=p, conf=p, pred2=None, q_out=None, stream=None)
    bad = [dict(C=0), dict(C=21), dict(C=-1), dict(conf=None), dict(rgb=None), dict(cams=None), dict(keys=None), dict(ws=None),
           dict(H=0), dict(W=0), dict(t=-1), dict(gt_prob=0.0), dict(gt_prob=1.0), dict(sxy_g=0.0), dict(sxy_b=-1.0), dict(srgb=0.0),
           dict(ws=p + 4)]
    for b in bad:
        a = dict(ok, **b)
        assert L.mx_ir_label(*a.values()) < 0, b
        assert b"ir_label" in L.mx_last_error(), b
    okl = dict(rgb=p, labels=p, L=4, H=4, W=4, t=10, gt_prob=0.7, sxy_g=3.0, w_g=3.0, sxy_b=50.0, srgb=5.0, w_b=10.0, trunc=4.0, ws=p,
               pred=p, q_out=None, stream=None)
    for b in (dict(L=1), dict(L=22), dict(labels=None), dict(rgb=None), dict(ws=None), dict(pred=None, q_out=None), dict(H=0),
              dict(t=-2), dict(gt_prob=1.5), dict(ws=p + 8)):
        a = dict(okl, **b)
        assert L.mx_crf_label(*a.values()) < 0, b
        assert b"crf_label" in L.mx_last_error(), b


def test_combine_conf_table():
    """All four (fg, bg) cases: class/class, class/background, background/class -> 255, background/background -> 0."""
    from muscle_amd.ir_label import combine_conf
    fg = np.array([[5, 5, 0, 0], [20, 1, 0, 0]], np.uint8)
    bg = np.array([[5, 0, 7, 0], [3, 1, 20, 0]], np.uint8)
    want = np.array([[5, 5, 255, 0], [20, 1, 255, 0]], np.uint8)
    got = combine_conf(fg, bg)
    assert got.dtype == np.uint8 and np.array_equal(got, want)
    assert np.array_equal(IR.combine_conf(fg, bg), want)
    assert np.array_equal(fg, [[5, 5, 0, 0], [20, 1, 0, 0]])                # the inputs are left alone
    assert np.array_equal(combine_conf(fg.astype(np.int64), bg.astype(np.int64)), want)


@pytest.mark.parametrize("L", [2, 4, 16, 17, 21])
def test_label_unary_is_the_one_hot_unary(L):
    """unary_from_labels(gt_prob) is crf_ref.unary of the one-hot map at confidence (gt_prob - 1/L) / (1 - 1/L): the label CRF is
    the existing model with another unary and other weights."""
    g = np.random.default_rng(L)
    lab = g.integers(0, L, (5, 7))
    onehot = (np.arange(L)[:, None, None] == lab[None]).astype(np.float64)
    a = R.unary(onehot, IR.one_hot_confidence(L))
    b = IR.unary_from_labels(lab, L)
    assert np.abs(a - b).max() <= 1e-12
    assert np.allclose(np.exp(-b).sum(0), 1.0, atol=1e-12)      # gt_prob and (1 - gt_prob) / (L - 1) are a distribution


def test_thresholded_argmax_ties_go_to_background():
    cams = np.zeros((2, 1, 4), np.float32)
    cams[0, 0] = [np.float32(0.30), np.nextafter(np.float32(0.30), np.float32(1)), 0.04, 0.6]
    cams[1, 0] = [0.10, np.nextafter(np.float32(0.30), np.float32(1)), np.float32(0.05), 0.6]
    labs = IR.label_maps(cams)
    assert labs[0].tolist() == [[0, 1, 0, 1]]                   # equal to the threshold: background; equal CAMs: the lower class
    assert labs[1].tolist() == [[1, 1, 0, 1]]


def test_public_names_and_signatures():
    import muscle_amd
    from muscle_amd.crf import crf_inference_label
    from muscle_amd.ir_label import cam_to_ir_label
    assert muscle_amd.crf_inference_label is crf_inference_label and callable(muscle_amd.cam_to_ir_label)
    c = inspect.signature(crf_inference_label).parameters                                   # src/imutils.py:477
    assert list(c)[:5] == ["img", "labels", "t", "n_labels", "gt_prob"]
    assert (c["t"].default, c["n_labels"].default, c["gt_prob"].default) == (10, 21, 0.7)
    assert c["trunc"].default == 4.0 and c["trunc"].kind is inspect.Parameter.KEYWORD_ONLY
    s = inspect.signature(cam_to_ir_label).parameters
    assert list(s)[:2] == ["img", "cam_dict"]
    assert (s["conf_fg_thres"].default, s["conf_bg_thres"].default, s["trunc"].default, s["fused"].default) == (0.30, 0.05, 4.0, True)
    assert all(s[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("conf_fg_thres", "conf_bg_thres", "trunc", "fused"))
    with pytest.raises(ValueError):
        cam_to_ir_label(np.zeros((4, 4, 3), np.uint8), {})


def test_script_module_imports_cleanly():
    """A fresh interpreter imports the script module without side effects and without cv2, imageio or pydensecrf; the command
    line has the issue's arguments; the package's function of the same name stays callable once the module is imported."""
    code = ("import sys, muscle_amd\n"
            "f = muscle_amd.cam_to_ir_label\n"
            "import muscle_amd.cam_to_ir_label as m\n"
            "assert not ({'cv2', 'imageio', 'pydensecrf'} & {k.split('.')[0] for k in sys.modules}), 'forbidden import'\n"
            "a = m.parse_args(['--cam_dir', 'c', '--ir_label_out_dir', 'o'])\n"
            "assert (a.voc12_root, a.infer_list, a.conf_fg_thres, a.conf_bg_thres, a.crf_trunc) == "
            "('data/VOC2012', 'data/train_aug.txt', 0.30, 0.05, 4.0), a\n"
            "assert a.num_workers >= 1 and callable(m.main) and callable(muscle_amd.cam_to_ir_label)\n"
            "try:\n"
            "    muscle_amd.cam_to_ir_label(None, {})\n"
            "except ValueError:\n"
            "    print('ok')\n")
    r = subprocess.run([sys.executable, "-c", code], cwd=ROOT, env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True,
                       timeout=120)
    assert r.returncode == 0 and r.stdout.strip() == "ok", r.stderr[-2000:]
    src = open(os.path.join(ROOT, "muscle_amd", "cam_to_ir_label.py")).read() + open(os.path.join(ROOT, "muscle_amd", "ir_label.py")).read()
    for name in ("cv2", "imageio", "pydensecrf"):
        assert f"import {name}" not in src


def test_script_names_missing_and_empty_dicts(tmp_path, capsys):
    import importlib
    script = importlib.import_module("muscle_amd.cam_to_ir_label")
    cam = tmp_path / "cam"
    cam.mkdir()
    np.save(cam / "2007_000001.npy", {3: np.zeros((2, 2), np.float32)})
    np.save(cam / "2007_000002.npy", {})
    (tmp_path / "list.txt").write_text("2007_000001\n2007_000002\n2007_000003\n")
    rc = script.main(["--cam_dir", str(cam), "--ir_label_out_dir", str(tmp_path / "out"), "--infer_list", str(tmp_path / "list.txt")])
    err = capsys.readouterr().err
    assert rc != 0 and "2007_000002" in err and "2007_000003" in err and "2007_000001" not in err
    assert not (tmp_path / "out").exists()


def test_golden_is_the_fp64_restatement():
    """tests/golden/ir_label.npz (tools/gen_ir_label_golden.py) holds the inputs and the fp64 Q_t, pred and conf of every case; the
    inputs are the named synthetic cases and the results are reproduced here.  Case (b) has background, ignore and two classes."""
    assert os.path.getsize(GOLDEN) <= 1 << 20
    z = np.load(GOLDEN)
    assert {k.split("/")[0] for k in z.files} == set(IR.CASES)
    for name, (_, H, W, C, trunc, _) in IR.CASES.items():
        img, cams, keys, tr = IR.case(name)
        assert tr == trunc and img.shape == (H, W, 3) and cams.shape == (C, H, W)
        assert np.array_equal(z[name + "/img"], img) and np.array_equal(z[name + "/keys"], keys)
        assert z[name + "/cams"].dtype == np.float16 and np.array_equal(z[name + "/cams"].astype(np.float32), cams)
        r = IR.ir_label(z[name + "/img"], z[name + "/cams"].astype(np.float32), z[name + "/keys"], trunc=trunc)
        q = z[name + "/q"]
        assert q.dtype == np.float64 and q.shape == (2, C + 1, H, W)
        assert np.abs(r["q"] - q).max() <= 1e-12                # the same fp64 program; BLAS may order the sums differently
        ok = IR.top2_gap(q) >= 1e-9
        assert np.array_equal(r["pred"][ok], z[name + "/pred"][ok]) and np.array_equal(z[name + "/pred"], q.argmax(1))
        assert np.array_equal(z[name + "/conf"], IR.combine_conf(keys[z[name + "/pred"][0]], keys[z[name + "/pred"][1]]))
        assert np.abs(q.sum(1) - 1).max() <= 1e-12
    vals = set(np.unique(z["b_48x72/conf"]).tolist())
    assert 0 in vals and 255 in vals and len(vals - {0, 255}) >= 2


def test_float32_switch():
    img, cams, keys, trunc = IR.case("f_9x45")
    q32 = IR.ir_label(img, cams, keys, trunc=trunc, dtype=np.float32)["q"]
    q64 = IR.ir_label(img, cams, keys, trunc=trunc)["q"]
    assert q32.dtype == np.float32 and q64.dtype == np.float64
    assert 0 < float(np.abs(q32 - q64).max()) < 1e-3
