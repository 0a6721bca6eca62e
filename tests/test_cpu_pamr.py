"""The PAMR model as tests/pamr_ref.py restates it (include/muscle_hip.h, mx_pamr_affinity ..): its invariants, an independent torch
formulation, and the argument checks of muscle_amd/pamr.py, infer.infer_seg / infer_cam_fused and the two scripts, which raise before
anything touches a device.  Nothing here needs a GPU."""
import ctypes

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import pamr_ref as R
from muscle_amd import _lib

DIL = R.DEFAULT_DILATIONS


def _img(kind, H, W, seed=0):
    g = np.random.default_rng(seed)
    if kind == "noise":
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(3 * x + y) % 256, (2 * y + 5) % 256, (x + 2 * y) % 256], axis=-1).astype(np.uint8)
    if kind == "blocks":                                    # 8x8 constant blocks: std = 0 in their interiors for dilation (1,)
        b = g.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(b, 8, axis=0), 8, axis=1)[:H, :W])
    raise KeyError(kind)


def _mask(C, H, W, seed=1):
    return np.random.default_rng(seed).random((C, H, W))


@pytest.mark.parametrize("kind", ["noise", "ramp", "blocks"])
@pytest.mark.parametrize("dil", [(1,), DIL])
def test_rows_sum_to_one_and_output_stays_in_range(kind, dil):
    img, m = _img(kind, 13, 17), _mask(3, 13, 17)
    out, w = R.pamr(img, m, 3, dil)
    assert w.shape == (1, 8 * len(dil), 13, 17) and w.dtype == np.float64
    assert float(np.abs(w.sum(axis=1) - 1.0).max()) <= 1e-12 and float(w.min()) >= 0.0
    assert out.shape == m.shape and float(out.min()) >= float(m.min()) - 1e-12 and float(out.max()) <= float(m.max()) + 1e-12
    same, _ = R.pamr(img, m, 0, dil)
    assert np.array_equal(same, m)                           # num_iter = 0 is the identity


def test_constant_image_gives_uniform_weights():
    img = np.full((9, 11, 3), 77, np.uint8)
    for dtype in (np.float64, np.float32):
        w = R.affinity(img, DIL, dtype)
        assert w.dtype == dtype and np.array_equal(w, np.full_like(w, dtype(1) / dtype(48)))
    b = R.affinity(_img("blocks", 24, 24), (1,))             # the interior of an 8x8 block sees one colour at dilation 1
    assert np.array_equal(b[0, :, 1:7, 1:7], np.full((8, 6, 6), 1.0 / 8))
    assert float(np.abs(b[0, :, 7, 7] - 1.0 / 8).max()) > 1e-3            # a block corner does not


def test_float32_switch():
    img, m = _img("noise", 12, 10), _mask(4, 12, 10)
    a, wa = R.pamr(img, m, 10)
    b, wb = R.pamr(img, m, 10, dtype=np.float32)
    assert a.dtype == wa.dtype == np.float64 and b.dtype == wb.dtype == np.float32
    assert 0 < float(np.abs(wa - wb).max()) < 1e-5 and 0 < float(np.abs(a - b).max()) < 1e-4
    u8 = R.affinity(img)
    f32 = R.affinity(np.ascontiguousarray(img.transpose(2, 0, 1)).astype(np.float32))
    assert np.array_equal(u8, f32)                           # the two image layouts state the same model


def _torch_pamr(img, mask, num_iter, dil):
    """An independent formulation in float64: replicate F.pad once, shifted slices, torch.std, torch.softmax."""
    I = torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).double()[None]       # [1,3,H,W]
    H, W = I.shape[-2:]
    r = max(dil)

    def taps(x, centre):
        xp = F.pad(x, (r, r, r, r), mode="replicate")
        return [xp[..., r + d * dy:r + d * dy + H, r + d * dx:r + d * dx + W]
                for d in dil for dy in (-1, 0, 1) for dx in (-1, 0, 1) if centre or (dy, dx) != (0, 0)]

    std = torch.stack(taps(I, True), dim=0).std(dim=0, unbiased=True)
    a = torch.stack([-(I - t).abs() / (1e-8 + 0.1 * std) for t in taps(I, False)], dim=0).mean(dim=2)      # [P,1,H,W]
    w = torch.softmax(a, dim=0)
    m = torch.from_numpy(mask).double()[None]
    for _ in range(num_iter):
        m = sum(w[p][:, None] * t for p, t in enumerate(taps(m, False)))
    return m[0].numpy(), w[:, 0].numpy()


@pytest.mark.parametrize("kind,H,W,dil", [("noise", 5, 7, DIL), ("ramp", 1, 9, DIL), ("blocks", 19, 21, (1,)), ("noise", 30, 27, (2, 5))])
def test_restatement_equals_torch_formulation(kind, H, W, dil):
    img, m = _img(kind, H, W, 3), _mask(2, H, W, 4)
    out, w = R.pamr(img, m, 4, dil)
    tout, tw = _torch_pamr(img, m, 4, dil)
    assert float(np.abs(w[0] - tw).max()) <= 1e-12
    assert float(np.abs(out - tout).max()) <= 1e-12


# ---- the argument checks: ValueError (argparse error in the scripts) before a device is touched -------------------------------------
def test_pamr_argument_checks():
    import muscle_amd
    from muscle_amd import pamr as P
    assert muscle_amd.PAMR is P.PAMR and muscle_amd.pamr_affinity is P.pamr_affinity and muscle_amd.pamr_apply is P.pamr_apply
    p = P.PAMR()
    assert p.num_iter == 10 and p.dilations == (1, 2, 4, 8, 12, 24)
    for bad in ((), (0,), (65,), (1, 2, 3, 4, 5, 6, 7, 8, 9), (1.5,), ("1",), (True,), 3):
        with pytest.raises(ValueError):
            P.PAMR(2, bad)
        with pytest.raises(ValueError):
            P.pamr_affinity(np.zeros((4, 4, 3), np.uint8), bad)
    for bad in (-1, 1.0, None, True):
        with pytest.raises(ValueError):
            P.PAMR(bad)
    img, mask = np.zeros((6, 5, 3), np.uint8), torch.zeros(2, 6, 5)
    for bad_img in (np.zeros((6, 5), np.uint8), np.zeros((6, 5, 4), np.uint8), np.zeros((6, 5, 3), np.int32),
                    torch.zeros(6, 5, 3), torch.zeros(3, 6, 5, dtype=torch.float64), torch.zeros(2, 2, 6, 5)):
        with pytest.raises(ValueError):
            p(bad_img, mask)
        with pytest.raises(ValueError):
            P.pamr_affinity(bad_img)
    for bad_mask in (np.zeros((2, 6, 5), np.float32), torch.zeros(6, 5), torch.zeros(2, 6, 5, dtype=torch.float64),
                     torch.zeros(2, 6, 5, dtype=torch.uint8), torch.zeros(2, 5, 6), torch.zeros(2, 2, 6, 5), torch.zeros(0, 6, 5)):
        with pytest.raises(ValueError):
            p(img, bad_mask)
    with pytest.raises(ValueError):                          # a size mismatch: PAMR here does not resize
        p(np.zeros((12, 10, 3), np.uint8), mask)
    with pytest.raises(ValueError):
        p(np.zeros((2, 6, 5, 3), np.uint8), mask)            # two images, one mask
    with pytest.raises(ValueError):
        P.pamr_apply(torch.zeros(48, 6, 4), mask)            # w of another size
    with pytest.raises(ValueError):
        P.pamr_apply(torch.zeros(8, 6, 5), mask)             # w of other dilations
    with pytest.raises(ValueError):
        P.pamr_apply(torch.zeros(48, 6, 5), mask, -1)
    # host tensors of the right shape: no CPU path
    with pytest.raises(_lib.MuscleHipError):
        p(torch.zeros(6, 5, 3, dtype=torch.uint8), mask)
    with pytest.raises(_lib.MuscleHipError):
        p(img, mask)                                         # the mask is checked before the numpy image is uploaded
    with pytest.raises(_lib.MuscleHipError):
        P.pamr_affinity(torch.zeros(3, 6, 5))
    with pytest.raises(_lib.MuscleHipError):
        P.pamr_apply(torch.zeros(48, 6, 5), mask, 1)
    with pytest.raises(_lib.MuscleHipError):
        P.planar_argmax(mask)


def test_infer_argument_checks():
    from muscle_amd import PAMR, infer
    img = np.zeros((4, 4, 3), np.uint8)
    label = torch.zeros(1, 20)
    for fn, args in ((infer.infer_seg, (None, [None], 4, 4)), (infer.infer_cam_fused, (None, [None], label, 4, 4))):
        with pytest.raises(ValueError, match="pamr_img"):
            fn(*args, pamr=PAMR(2))
        with pytest.raises(ValueError, match="without pamr"):
            fn(*args, pamr_img=img)
        with pytest.raises(ValueError, match="PAMR"):
            fn(*args, pamr=2, pamr_img=img)
        with pytest.raises(ValueError, match="output"):
            fn(*args, pamr=PAMR(2), pamr_img=np.zeros((4, 5, 3), np.uint8))
        with pytest.raises(ValueError, match="uint8"):
            fn(*args, pamr=PAMR(2), pamr_img=np.zeros((3, 4, 4), np.float32))
    with pytest.raises(ValueError, match="one of them"):      # PAMR and the CRF are refused together
        infer.infer_seg(None, [None], 4, 4, crf_img=img, pamr=PAMR(2), pamr_img=img)


def test_script_argument_checks(capsys):
    from muscle_amd import infer_mcl, infer_seg
    a = infer_mcl.parse_args(["--weights", "w"])
    assert a.pamr_iters == 0 and a.pamr_dilations == [1, 2, 4, 8, 12, 24]
    a = infer_mcl.parse_args(["--weights", "w", "--pamr_iters", "3", "--pamr_dilations", "1", "3"])
    assert a.pamr_iters == 3 and a.pamr_dilations == [1, 3]
    s = infer_seg.parse_args(["--weights", "w"])
    assert s.pamr_iters == 0 and s.pamr_dilations == [1, 2, 4, 8, 12, 24] and s.crf == 0
    s = infer_seg.parse_args(["--weights", "w", "--pamr_iters", "10"])
    assert s.pamr_iters == 10
    for mod in (infer_mcl, infer_seg):
        for bad in (["--pamr_iters", "-1"], ["--pamr_iters", "2", "--pamr_dilations", "0"], ["--pamr_dilations", "65"],
                    ["--pamr_dilations"] + ["1"] * 9, ["--pamr_iters", "x"]):
            with pytest.raises(SystemExit) as e:
                mod.parse_args(["--weights", "w"] + bad)
            assert e.value.code == 2
            assert "pamr" in capsys.readouterr().err
    with pytest.raises(SystemExit) as e:                     # the --crf 2 refusal
        infer_seg.parse_args(["--weights", "w", "--crf", "2", "--pamr_iters", "2"])
    assert e.value.code == 2 and "--pamr_iters with --crf" in capsys.readouterr().err
    assert infer_seg.parse_args(["--weights", "w", "--crf", "2"]).pamr_iters == 0


# ---- the C ABI: declared, exported, and its limits are argument errors before any launch ---------------------------------------------
def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_pamr_affinity"] == "piiiipipp"
    assert sigs["mx_pamr_step"] == "pppiiiipip"
    assert sigs["mx_pamr_ws"] == "iiiii" and "mx_pamr_ws" in _lib.LONG_RETURNS
    assert sigs["mx_pamr"] == "pippiiiipiiplp"
    assert sigs["mx_planar_argmax"] == "piiiipp"
    L = _lib.lib()
    for name in ("mx_pamr_affinity", "mx_pamr_step", "mx_pamr_ws", "mx_pamr", "mx_planar_argmax"):
        assert hasattr(L, name), name


def test_limits_are_argument_errors():
    """rc < 0 with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(4096)
    p = (ctypes.addressof(buf) & ~255) + 256
    q = p + 1024
    dil = lambda *d: (ctypes.c_int * len(d))(*d)  # noqa: E731
    N = 375 * 500
    assert L.mx_pamr_ws(1, 21, 375, 500, 6) >= N * 48 * 4 + N * 21 * 4 and L.mx_pamr_ws(1, 21, 375, 500, 6) % 16 == 0
    assert L.mx_pamr_ws(1, 25, 5, 7, 1) > 0                   # no cap on the class count
    for args in ((0, 1, 4, 4, 1), (1, 0, 4, 4, 1), (1, 1, 0, 4, 1), (1, 1, 4, 0, 1), (1, 1, 4, 4, 0), (1, 1, 4, 4, 9),
                 (1, 64, 8192, 4096, 1), (1, 1, 8192, 8192, 4)):               # N max(C,P) H W = 2^31
        assert L.mx_pamr_ws(*args) < 0, args
        assert b"mx_pamr_ws" in L.mx_last_error()
    assert L.mx_pamr_ws(1, 63, 8192, 4096, 1) > 0
    for d in (dil(0), dil(65), dil(-3)):
        assert L.mx_pamr_affinity(p, 0, 1, 4, 4, d, 1, q, None) < 0 and b"mx_pamr_affinity" in L.mx_last_error()
        assert L.mx_pamr_step(p, q, q + 1024, 1, 1, 4, 4, d, 1, None) < 0 and b"mx_pamr_step" in L.mx_last_error()
        assert L.mx_pamr(p, 0, q, q + 1024, 1, 1, 4, 4, d, 1, 1, p, 4096, None) < 0 and b"mx_pamr" in L.mx_last_error()
    one = dil(1)
    assert L.mx_pamr_affinity(p, 2, 1, 4, 4, one, 1, q, None) < 0 and b"img_kind" in L.mx_last_error()
    assert L.mx_pamr_affinity(None, 0, 1, 4, 4, one, 1, q, None) < 0
    assert L.mx_pamr_affinity(p, 0, 1, 4, 4, one, 0, q, None) < 0 and L.mx_pamr_affinity(p, 0, 1, 4, 4, one, 9, q, None) < 0
    assert L.mx_pamr_affinity(p, 0, 1, 4, 4, None, 1, q, None) < 0
    assert L.mx_pamr_step(p, q, q, 1, 2, 4, 4, one, 1, None) < 0 and b"overlap" in L.mx_last_error()
    assert L.mx_pamr_step(p, q, q + 64, 1, 2, 4, 4, one, 1, None) < 0 and b"overlap" in L.mx_last_error()
    assert L.mx_pamr(p, 0, q, q, 1, 2, 4, 4, one, 1, 1, p, 4096, None) < 0 and b"overlap" in L.mx_last_error()
    assert L.mx_pamr(p, 0, q, q + 1024, 1, 2, 4, 4, one, 1, -1, p, 4096, None) < 0 and b"num_iter" in L.mx_last_error()
    assert L.mx_pamr(p, 0, q, q + 1024, 1, 2, 4, 4, one, 1, 1, p, 16, None) < 0 and b"mx_pamr_ws" in L.mx_last_error()
    assert L.mx_pamr(p, 0, q, q + 1024, 1, 2, 4, 4, one, 1, 1, p + 4, 4096, None) < 0 and b"aligned" in L.mx_last_error()
    assert L.mx_pamr(p, 0, q, q + 1024, 1, 2, 4, 4, one, 1, 1, None, 4096, None) < 0
    assert L.mx_planar_argmax(p, 1, 257, 4, 4, q, None) < 0 and L.mx_planar_argmax(p, 1, 0, 4, 4, q, None) < 0
    assert b"mx_planar_argmax" in L.mx_last_error()
