"""Host side of the dense CRF (no kernel is launched): argument errors of the mx_crf_* entries are reported before any launch,
the header declares the entries and the library exports them, the command line accepts --crf 2 and still refuses --crf 1,
and the numpy restatement (crf_ref.py) documents the default window: trunc = 4 and 5 against all pairs."""
import ctypes
import os

import numpy as np
import pytest

import crf_ref as R
from muscle_amd import _lib

ENTRIES = ("mx_crf_workspace_bytes", "mx_crf_normalizers", "mx_crf_inference")


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_crf_workspace_bytes"] == "iii" and "mx_crf_workspace_bytes" in _lib.LONG_RETURNS
    assert sigs["mx_crf_normalizers"] == "piiffffpppp"
    assert sigs["mx_crf_inference"] == "ppiiiifffffffpppp"
    text = open(_lib.HEADER_PATH).read()
    assert text.count("src/imutils.py:439-456") >= 3           # every entry cites the reference
    if not os.path.exists(_lib.LIB_PATH):
        from muscle_amd import _build
        _build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_workspace_bytes():
    L = _lib.lib()
    n = L.mx_crf_workspace_bytes(21, 375, 500)
    assert n >= 375 * 500 * 4 * (2 * 32 + 2) and n % 16 == 0   # at least two Q buffers and the two normalisers
    assert L.mx_crf_workspace_bytes(21, 1, 1) > 0
    for args in ((0, 4, 4), (25, 4, 4), (21, 0, 4), (21, 4, 0), (21, -1, 4)):
        assert L.mx_crf_workspace_bytes(*args) < 0, args
        assert b"crf_workspace_bytes" in L.mx_last_error()


def test_bad_arguments_before_any_launch():
    """rc < 0 with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = ctypes.addressof(buf) & ~15
    p = p + 16
    ok = dict(rgb=p, prob=p, L=21, H=4, W=4, t=4, confidence=0.5, sxy_g=2.0, w_g=1.0, sxy_b=21.0, srgb=10.0, w_b=10.0, trunc=4.0,
              workspace=p, q_out=p, pred=p, stream=None)
    bad = [dict(L=0), dict(L=25), dict(t=-1), dict(sxy_g=0.0), dict(sxy_b=-1.0), dict(srgb=0.0), dict(rgb=None), dict(prob=None),
           dict(workspace=None), dict(H=0), dict(W=0), dict(q_out=None, pred=None), dict(workspace=p + 4)]
    for b in bad:
        a = dict(ok, **b)
        assert L.mx_crf_inference(*a.values()) < 0, b
        assert b"crf_inference" in L.mx_last_error(), b
    okn = dict(rgb=p, H=4, W=4, sxy_g=2.0, sxy_b=21.0, srgb=10.0, trunc=4.0, workspace=p, n_g=p, n_b=p, stream=None)
    for b in (dict(rgb=None), dict(workspace=None), dict(n_g=None), dict(n_b=None), dict(H=0), dict(W=0), dict(sxy_g=0.0),
              dict(sxy_b=0.0), dict(srgb=-2.0)):
        a = dict(okn, **b)
        assert L.mx_crf_normalizers(*a.values()) < 0, b
        assert b"crf_normalizers" in L.mx_last_error(), b


def test_command_line():
    from muscle_amd import infer_seg
    a = infer_seg.parse_args(["--weights", "w.pth", "--crf", "2"])
    assert a.crf == 2 and a.crf_trunc == 4.0
    a = infer_seg.parse_args(["--weights", "w.pth", "--crf", "2", "--crf_trunc", "3"])
    assert a.crf_trunc == 3.0
    assert infer_seg.parse_args(["--weights", "w.pth"]).crf == 0


@pytest.mark.parametrize("crf", ["1", "3"])
def test_crf_1_still_refused_and_points_to_2(crf, capsys):
    from muscle_amd import infer_seg
    with pytest.raises(SystemExit) as e:
        infer_seg.main(["--weights", "none.pth", "--crf", crf])
    assert e.value.code != 0
    err = capsys.readouterr().err
    assert "CRF" in err and "--crf 2" in err


def test_infer_seg_signature():
    import inspect
    from muscle_amd.crf import crf_inference
    from muscle_amd.infer import infer_seg
    s = inspect.signature(infer_seg).parameters
    assert s["crf_img"].default is None and s["crf_t"].default == 4 and s["crf_trunc"].default == 4.0
    c = inspect.signature(crf_inference).parameters                                          # src/imutils.py:439
    assert list(c)[:6] == ["img", "probs", "t", "scale_factor", "labels", "confidence"]
    assert (c["t"].default, c["scale_factor"].default, c["labels"].default, c["confidence"].default) == (2, 1.5, 21, 0.5)
    assert c["trunc"].default == 4.0 and c["trunc"].kind is inspect.Parameter.KEYWORD_ONLY


def test_window_documents_the_default():
    """Standard image, scale_factor 6 (the window is cut inside the image), t = 4, fp64: the windowed model against all pairs.
    Measured: 7.7e-5 at trunc = 4 (the default) and 1.2e-6 at trunc = 5."""
    img, probs = R.standard_input()
    assert img.shape == (40, 56, 3) and img.dtype == np.uint8 and probs.shape == (21, 40, 56)
    full = R.crf_ref(img, probs, 4, scale_factor=6.0, trunc=0.0)
    assert np.abs(full.sum(0) - 1).max() < 1e-12
    d4 = float(np.abs(R.crf_ref(img, probs, 4, scale_factor=6.0, trunc=4.0) - full).max())
    d5 = float(np.abs(R.crf_ref(img, probs, 4, scale_factor=6.0, trunc=5.0) - full).max())
    print("trunc 4 / 5 against all pairs:", d4, d5)
    assert 0 < d4 < 1e-3 and 0 < d5 < 1e-5
    # the CRF moves labels towards the colour edges
    assert float((full.argmax(0) != probs.argmax(0)).mean()) > 0.05


def test_float32_switch():
    img, probs = R.standard_input()
    q32 = R.crf_ref(img, probs, 2, scale_factor=6.0, dtype=np.float32)
    q64 = R.crf_ref(img, probs, 2, scale_factor=6.0)
    assert q32.dtype == np.float32 and q64.dtype == np.float64
    assert 0 < float(np.abs(q32 - q64).max()) < 1e-4
