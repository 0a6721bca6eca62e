"""Host side of the permutohedral-lattice backend (no kernel is launched): the numpy restatement (lattice_ref.py) against the exact
Gaussian kernel it approximates, its barycentric weights, the header and the library's exports, argument errors before any launch,
the command lines and the `pairwise` keyword."""
import ctypes
import os

import numpy as np
import pytest

import crf_ref as R
import lattice_ref as LR
from muscle_amd import _lib

ENTRIES = ("mx_lattice_ws", "mx_lattice_build", "mx_lattice_filter", "mx_lattice_export", "mx_crf_lattice_ws",
           "mx_crf_inference_lattice", "mx_crf_label_lattice", "mx_ir_label_lattice")
H, W = 40, 56


def _xy():
    yy, xx = np.mgrid[0:H, 0:W]
    return np.stack([xx.ravel(), yy.ravel()], 1).astype(np.int64), xx, yy


def _smooth_image():
    _, xx, yy = _xy()
    img = np.zeros((H, W, 3), np.uint8)
    img[..., 0], img[..., 1], img[..., 2] = 3 * xx, 4 * yy, 100
    return img


def _feats(name):
    if name == "d2_sxy3":
        return LR.features((H, W), 3.0)
    if name == "d2_sxy6":
        return LR.features((H, W), 6.0)
    return LR.features(_smooth_image(), 20.0, 10.0)


@pytest.mark.parametrize("name", ["d2_sxy3", "d2_sxy6", "d5_smooth"])
def test_oracle_against_the_exact_kernel(name):
    """filter(v) / filter(1) against K v / K 1 of crf_ref.Kernel(R=None) on dense inputs, v = three channels of uniform noise
    (the prototype's input: it gave 0.0155, 0.0061 and 0.0175); each bounded at 0.035, twice the worst."""
    f = _feats(name)
    xy = _xy()[0]
    v = np.random.default_rng(1).random((H * W, 3))
    one = np.ones(H * W)
    lat = LR.Lattice(f)
    K = R.Kernel(f.astype(np.float64), xy, None, np.float64)
    a = lat.filter(v) / lat.filter(one)[:, None]
    b = K.apply(v) / K.apply(one)[:, None]
    err = float(np.abs(a - b).max())
    print(name, "vertices", lat.M, "err", err)
    assert lat.M < H * W                                        # dense: fewer vertices than pixels
    assert err <= 0.035


@pytest.mark.parametrize("name", ["d2_sxy3", "d5_smooth", "d5_noisy"])
def test_weights(name):
    f = LR.features(R.standard_input()[0], 32.0 / 6.0, 10.0) if name == "d5_noisy" else _feats(name)
    lat = LR.Lattice(f)
    assert lat.w.dtype == np.float32 and lat.w.shape == (H * W, f.shape[1] + 1)
    assert np.abs(lat.w.astype(np.float64).sum(1) - 1).max() <= 2e-7
    assert lat.w.min() >= -1e-6
    # every pixel's D+1 vertices are distinct, and every neighbour relation is mutual
    assert all(len(set(r)) == len(r) for r in lat.vid.tolist())
    for j in range(lat.D + 1):
        has = lat.n1[:, j] >= 0
        assert np.array_equal(lat.n2[lat.n1[has, j], j], np.nonzero(has)[0])


def test_float32_switch():
    lat = LR.Lattice(LR.features(R.standard_input()[0], 32.0 / 6.0, 10.0))
    v = np.random.default_rng(2).random((H * W, 2))
    a, b = lat.filter(v), lat.filter(v, np.float32)
    assert a.dtype == np.float64 and b.dtype == np.float32
    assert 0 < float(np.abs(a - b).max()) < 1e-4 * float(np.abs(a).max())


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_lattice_ws"] == "iiii" and "mx_lattice_ws" in _lib.LONG_RETURNS
    assert sigs["mx_crf_lattice_ws"] == "iii" and "mx_crf_lattice_ws" in _lib.LONG_RETURNS
    assert sigs["mx_lattice_build"] == "piiffpp"
    assert sigs["mx_lattice_filter"] == "pppip"
    assert sigs["mx_lattice_export"] == "ppppppp"
    # the argument lists of the windowed counterparts without trunc / fused
    assert sigs["mx_crf_inference_lattice"] == sigs["mx_crf_inference"].replace("fffffffp", "ffffffp") == "ppiiiiffffffpppp"
    assert sigs["mx_crf_label_lattice"] == "ppiiiiffffffpppp" and len(sigs["mx_crf_label"]) == len(sigs["mx_crf_label_lattice"]) + 1
    assert sigs["mx_ir_label_lattice"] == "pppiiiffiffffffppppp" and len(sigs["mx_ir_label"]) == len(sigs["mx_ir_label_lattice"]) + 2
    import re
    text = open(_lib.HEADER_PATH).read()
    for name in ENTRIES:                                        # every entry cites the reference in the comment above it
        m = re.search(r"/\*((?:(?!\*/).)*)\*/\s*(?:int|long)\s+" + name + r"\s*\(", text, flags=re.S)
        assert m, name
        assert "src/imutils.py:439-456" in m.group(1) or "src/imutils.py:477-491" in m.group(1), name
    if not os.path.exists(_lib.LIB_PATH):
        from muscle_amd import _build
        _build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_workspace_bytes():
    L = _lib.lib()
    n = L.mx_lattice_ws(5, 375, 500, 32)
    N = 375 * 500
    assert n >= N * 6 * 32 * 4 * 2 and n % 16 == 0              # at least two value buffers of N (D+1) vertices x C channels
    assert L.mx_lattice_ws(2, 1, 1, 1) > 0
    assert L.mx_lattice_ws(5, 40, 56, 32) > L.mx_lattice_ws(5, 40, 56, 1) > L.mx_lattice_ws(2, 40, 56, 1)
    for args in ((3, 4, 4, 1), (5, 0, 4, 1), (5, 4, 0, 1), (5, -1, 4, 1), (5, 4, 4, 0), (5, 4, 4, 33), (2, 4096, 4096, 1)):
        assert L.mx_lattice_ws(*args) < 0, args
        assert b"lattice_ws" in L.mx_last_error()
    assert L.mx_crf_lattice_ws(21, 375, 500) > 0 and L.mx_crf_lattice_ws(21, 375, 500) % 16 == 0
    for args in ((0, 4, 4), (25, 4, 4), (21, 0, 4), (21, 4, 0)):
        assert L.mx_crf_lattice_ws(*args) < 0, args
        assert b"crf_lattice_ws" in L.mx_last_error()


def test_bad_arguments_before_any_launch():
    """rc < 0 with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    ok = dict(rgb=p, H=4, W=4, sxy=3.0, srgb=10.0, ws=p, stream=None)
    for b in (dict(ws=None), dict(rgb=None), dict(H=0), dict(W=0), dict(H=-3), dict(sxy=0.0), dict(sxy=-1.0), dict(ws=p + 4),
              dict(sxy=1e-9),                                   # the key range does not fit the packed key
              dict(srgb=1e-12), dict(H=4096, W=4096)):
        a = dict(ok, **b)
        assert L.mx_lattice_build(*a.values()) < 0, b
        assert b"lattice_build" in L.mx_last_error(), b
    assert L.mx_lattice_build(*dict(ok, sxy=1e-9).values()) < 0 and b"key range" in L.mx_last_error()
    okf = dict(ws=p, inp=p, out=p, C=3, stream=None)
    for b in (dict(ws=None), dict(inp=None), dict(out=None), dict(C=0), dict(C=33), dict()):     # the last: no lattice in ws
        a = dict(okf, **b)
        assert L.mx_lattice_filter(*a.values()) < 0, b
        assert b"lattice_filter" in L.mx_last_error(), b
    assert L.mx_lattice_export(p, p, p, p, p, p, None) < 0 and b"lattice_export" in L.mx_last_error()
    assert L.mx_lattice_export(p, None, p, p, p, p, None) < 0 and b"lattice_export" in L.mx_last_error()

    oki = dict(rgb=p, prob=p, L=21, H=4, W=4, t=4, confidence=0.5, sxy_g=2.0, w_g=1.0, sxy_b=21.0, srgb=10.0, w_b=10.0, ws=p, q_out=p,
               pred=p, stream=None)
    for b in (dict(L=0), dict(L=25), dict(t=-1), dict(sxy_g=0.0), dict(sxy_b=-1.0), dict(srgb=0.0), dict(rgb=None), dict(prob=None),
              dict(ws=None), dict(H=0), dict(W=0), dict(q_out=None, pred=None), dict(ws=p + 4), dict(sxy_g=1e-9), dict(srgb=1e-12)):
        a = dict(oki, **b)
        assert L.mx_crf_inference_lattice(*a.values()) < 0, b
        assert b"crf_inference_lattice" in L.mx_last_error(), b
    okl = dict(rgb=p, labels=p, L=4, H=4, W=4, t=10, gt_prob=0.7, sxy_g=3.0, w_g=3.0, sxy_b=50.0, srgb=5.0, w_b=10.0, ws=p, pred=p,
               q_out=p, stream=None)
    for b in (dict(L=1), dict(L=22), dict(t=-1), dict(gt_prob=0.0), dict(gt_prob=1.0), dict(sxy_b=0.0), dict(rgb=None),
              dict(labels=None), dict(ws=None), dict(H=0), dict(pred=None, q_out=None), dict(ws=p + 8), dict(sxy_b=1e-9)):
        a = dict(okl, **b)
        assert L.mx_crf_label_lattice(*a.values()) < 0, b
        assert b"crf_label_lattice" in L.mx_last_error(), b
    okr = dict(rgb=p, cams=p, keys=p, C=3, H=4, W=4, fg=0.3, bg=0.05, t=10, gt_prob=0.7, sxy_g=3.0, w_g=3.0, sxy_b=50.0, srgb=5.0,
               w_b=10.0, ws=p, conf=p, pred2=p, q_out=p, stream=None)
    for b in (dict(C=0), dict(C=21), dict(t=-1), dict(gt_prob=1.5), dict(srgb=-1.0), dict(rgb=None), dict(cams=None), dict(keys=None),
              dict(ws=None), dict(conf=None), dict(W=0), dict(ws=p + 4), dict(sxy_g=1e-9)):
        a = dict(okr, **b)
        assert L.mx_ir_label_lattice(*a.values()) < 0, b
        assert b"ir_label_lattice" in L.mx_last_error(), b


def test_command_lines():
    import importlib
    script = importlib.import_module("muscle_amd.cam_to_ir_label")
    from muscle_amd import infer_seg
    base = ["--cam_dir", "c", "--ir_label_out_dir", "o"]
    assert script.parse_args(base).crf_pairwise == "window"
    assert script.parse_args(base + ["--crf_pairwise", "lattice"]).crf_pairwise == "lattice"
    with pytest.raises(SystemExit) as e:
        script.parse_args(base + ["--crf_pairwise", "exact"])
    assert e.value.code != 0
    a = infer_seg.parse_args(["--weights", "w.pth", "--crf", "2"])
    assert a.crf_pairwise == "window"
    a = infer_seg.parse_args(["--weights", "w.pth", "--crf", "2", "--crf_pairwise", "lattice"])
    assert a.crf == 2 and a.crf_pairwise == "lattice"
    with pytest.raises(SystemExit) as e:
        infer_seg.parse_args(["--weights", "w.pth", "--crf", "2", "--crf_pairwise", "nonsense"])
    assert e.value.code != 0
    with pytest.raises(SystemExit) as e:                        # --crf 1 stays refused whatever the backend
        infer_seg.parse_args(["--weights", "w.pth", "--crf", "1", "--crf_pairwise", "lattice"])
    assert e.value.code != 0


def test_pairwise_keyword():
    """Keyword only, default "window", anything else a ValueError before the device is touched (the inputs are host arrays and no
    device exists here)."""
    import inspect
    import muscle_amd
    from muscle_amd import crf, infer, ir_label
    assert muscle_amd.PermutohedralLattice is muscle_amd.lattice.PermutohedralLattice
    for fn in (crf.crf_inference, crf.crf_run, crf.crf_inference_label, crf.crf_label_run, ir_label.ir_label_run, ir_label.cam_to_ir_label):
        s = inspect.signature(fn).parameters["pairwise"]
        assert s.default == "window" and s.kind is inspect.Parameter.KEYWORD_ONLY, fn
    assert inspect.signature(infer.infer_seg).parameters["crf_pairwise"].default == "window"
    img = np.zeros((4, 4, 3), np.uint8)
    probs = np.full((3, 4, 4), 1 / 3, np.float32)
    labs = np.zeros((4, 4), np.int64)
    with pytest.raises(ValueError):
        crf.crf_inference(img, probs, labels=3, pairwise="nonsense")
    with pytest.raises(ValueError):
        crf.crf_run(img, probs, 1, 1.5, 3, 0.5, 4.0, pairwise="Lattice")
    with pytest.raises(ValueError):
        crf.crf_inference_label(img, labs, n_labels=3, pairwise="nonsense")
    with pytest.raises(ValueError):
        crf.crf_label_run(img, labs, 1, 3, 0.7, 4.0, pairwise="")
    with pytest.raises(ValueError):
        ir_label.ir_label_run(img, probs[:2], [0, 1, 2], pairwise="nonsense")
    with pytest.raises(ValueError):
        ir_label.cam_to_ir_label(img, {0: probs[0]}, pairwise="nonsense")
    with pytest.raises(ValueError):
        infer.infer_seg(None, [None], 4, 4, crf_pairwise="nonsense")
