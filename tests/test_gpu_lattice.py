"""GPU parity of the permutohedral-lattice backend (muscle_amd.lattice / csrc/lattice.hip; the filter pydensecrf evaluates the CRFs of
src/imutils.py:439-456 and :477-491 on) against its numpy restatement lattice_ref.py.

Structure: exact (key set, per-pixel vertex keys, bit-equal weights, every neighbour entry).  Values: e32 = the error of the
np.float32 restatement against the fp64 one on the same structure is computed here per case, and the kernels must stay within
F * e32 + 1e-7 * max|reference|.  F follows the protocol of profiles/crf_bench.txt: the err / e32 pairs of the first GPU run are in
profiles/lattice_bench.txt; the worst was 19.7 (the single-pixel case, where e32 is one rounding error; 4.6 otherwise) and F is
twice it, rounded up: 40.  Labels: pred and conf equal the fp64 ones on every pixel whose fp64
top-two gap is >= 1e-3 in the problems that decide it; at most 0.5 % of the pixels may be left out (GAP and MAX_LEFT_OUT of
test_gpu_ir_label.py)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_ref as R
import ir_label_ref as IR
import lattice_ref as LR
from muscle_amd import synth
from muscle_amd.arch import net_cfg

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
F_TOL, GAP, MAX_LEFT_OUT = 40.0, 1e-3, 0.005


def _noisy(seed, H, W):
    return IR.synthetic(seed, H, W, 1)[0]


def _constant():
    img = np.empty((32, 48, 3), np.uint8)
    img[:] = (90, 140, 60)
    return img


def _two_halves():
    half = _noisy(31, 24, 20)
    return np.concatenate([half, half], 1)


# name -> (image, sxy, srgb or None)
CASES = {
    "1_std_sf1.5": lambda: (R.standard_input()[0], 32.0 / 1.5, 10.0),
    "2_std_label": lambda: (R.standard_input()[0], 50.0, 5.0),
    "3_std_sf6": lambda: (R.standard_input()[0], 32.0 / 6.0, 10.0),     # fp32 and fp64 construction disagree here
    "4_d2_sxy2": lambda: (R.standard_input()[0], 2.0, None),
    "4_d2_sxy3": lambda: (R.standard_input()[0], 3.0, None),
    "5_37x53": lambda: (_noisy(21, 37, 53), 32.0 / 1.5, 10.0),
    "5_37x53_d2": lambda: (_noisy(21, 37, 53), 0.5, None),
    "6_1x1": lambda: (_noisy(22, 1, 1), 50.0, 5.0),
    "6_1x1_d2": lambda: (_noisy(22, 1, 1), 3.0, None),
    "7_5x70": lambda: (_noisy(23, 5, 70), 32.0 / 6.0, 10.0),
    "8_45x9": lambda: (_noisy(24, 45, 9), 50.0, 5.0),
    "9_constant": lambda: (_constant(), 50.0, 5.0),                      # the heaviest contention in the hash insert and the splat
    "10_two_halves": lambda: (_two_halves(), 32.0 / 1.5, 10.0),
}

_ORACLE, _GPU = {}, {}


def _oracle(name):
    """(img, sxy, srgb, lattice_ref.Lattice), built once."""
    if name not in _ORACLE:
        img, sxy, srgb = CASES[name]()
        f = LR.features(img, sxy, srgb) if srgb else LR.features(tuple(img.shape[:2]), sxy)
        _ORACLE[name] = (img, sxy, srgb, LR.Lattice(f))
    return _ORACLE[name]


def _lattice(name):
    """The device lattice of a case, built once."""
    if name not in _GPU:
        from muscle_amd import PermutohedralLattice
        img, sxy, srgb, _ = _oracle(name)
        _GPU[name] = PermutohedralLattice(img, sxy, srgb)
        torch.cuda.synchronize()
    return _GPU[name]


def _bound(err, e32, ref, what):
    scale = float(np.abs(ref).max())
    print(f"{what}: err={err:.3e} e32={e32:.3e} ratio={err / max(e32, 1e-30):.3f} max|ref|={scale:.3e}")
    assert err <= F_TOL * e32 + 1e-7 * scale, (what, err, e32)


@pytest.mark.parametrize("name", list(CASES))
def test_structure(name):
    img, sxy, srgb, ref = _oracle(name)
    lat = _lattice(name)
    vid, w, keys, nbr, M = [x.cpu().numpy() if torch.is_tensor(x) else x for x in lat.export()]
    D, N = ref.D, ref.N
    assert lat.D == D and vid.shape == (N, D + 1) and keys.shape == (M, D)
    gk = [tuple(k) for k in keys.tolist()]
    assert M == ref.M and len(set(gk)) == M and set(gk) == set(ref.index)             # the key set, exactly
    assert vid.min() >= 0 and vid.max() < M
    assert np.array_equal(keys[vid], ref.pixel_keys)                                   # per pixel and r: the vertex's key
    assert np.array_equal(w.view(np.uint32), ref.w.view(np.uint32))                    # the weights, bit for bit
    gid = {k: n for n, k in enumerate(gk)}
    perm = np.array([gid[tuple(k)] for k in ref.keys.tolist()], np.int64)              # oracle id -> device id
    cap = N * (D + 1)
    assert nbr.shape == (2 * (D + 1), cap)
    for j in range(D + 1):
        for s, table in ((0, ref.n1), (1, ref.n2)):
            want = np.where(table[:, j] >= 0, perm[np.maximum(table[:, j], 0)], -1)
            assert np.array_equal(nbr[2 * j + s][perm], want), (j, s)
    print(f"{name}: D={D} N={N} vertices={M} absent neighbours {float((nbr[:, :M] < 0).mean()):.3f}")


@pytest.mark.parametrize("C", [1, 3, 21, 32])
@pytest.mark.parametrize("name", list(CASES))
def test_filter(name, C):
    """C random channels (one of them scaled by 1e3, one constant) against the fp64 filter on the oracle's structure."""
    img, sxy, srgb, ref = _oracle(name)
    H, W = img.shape[:2]
    x = np.random.default_rng(100 + C).normal(0, 1, (C, H, W)).astype(np.float32)
    if C >= 3:
        x[1] *= 1e3
        x[2] = 1.0
    out = _lattice(name).filter(T(x).to(DEV))
    torch.cuda.synchronize()
    out = out.cpu().numpy().reshape(C, -1).T.astype(np.float64)
    v = x.reshape(C, -1).T
    r64 = ref.filter(v, np.float64)
    r32 = ref.filter(v, np.float32)
    assert np.isfinite(out).all()
    for c in range(C):                                         # per channel: a channel's tolerance is its own scale
        e32 = float(np.abs(r32[:, c].astype(np.float64) - r64[:, c]).max())
        _bound(float(np.abs(out[:, c] - r64[:, c]).max()), e32, r64[:, c], f"filter {name} C={C} c={c}")


@pytest.mark.parametrize("name", ["3_std_sf6", "9_constant"])
def test_reproducible_bits(name):
    """Two builds and filters in one process: vertex ids may differ, the values may not."""
    from muscle_amd import PermutohedralLattice
    img, sxy, srgb, _ = _oracle(name)
    x = T(np.random.default_rng(7).normal(0, 1, (21,) + img.shape[:2]).astype(np.float32)).to(DEV)
    a = PermutohedralLattice(img, sxy, srgb, max_channels=21)
    ya = a.filter(x)
    b = PermutohedralLattice(T(img).to(DEV), sxy, srgb, max_channels=21)
    yb, ya2 = b.filter(x), a.filter(x)
    torch.cuda.synchronize()
    assert torch.equal(ya, yb) and torch.equal(ya, ya2)
    assert torch.equal(ya[3], a.filter(x[3]))                   # a channel does not depend on its neighbours ([H,W] in, [H,W] out)
    with pytest.raises(ValueError):
        a.filter(torch.zeros(22, *img.shape[:2]))


# ---- the CRF of crf_inference ------------------------------------------------------------------------------------------------

def _probs(seed, H, W, L):
    """A smooth probability map of any size (the construction of crf_ref.standard_input)."""
    import scipy.ndimage
    g = np.random.default_rng(seed)
    lab = np.zeros((H, W), int)
    lab[:, :2 * W // 5] = 1 % L
    lab[H // 5:4 * H // 5, W // 4:6 * W // 7] = (L - 1) // 2
    lab[:, 3 * W // 4:] = L - 1
    logit = g.normal(0, 1.0, (L, H, W))
    for k in range(L):
        logit[k] += 2.5 * (lab == k)
    logit = scipy.ndimage.gaussian_filter(logit, (0, 3, 3)) * 3
    probs = np.exp(logit)
    return probs / probs.sum(0, keepdims=True)


_CRF = {"std_sf1.5": lambda: R.standard_input() + (1.5,), "std_sf6": lambda: R.standard_input() + (6.0,),
        "ragged_37x53": lambda: (_noisy(21, 37, 53), _probs(1, 37, 53, 21), 1.5)}
_CRF_LATS = {}


def _crf_case(name):
    if name not in _CRF_LATS:
        img, probs, sf = _CRF[name]()
        _CRF_LATS[name] = (img, probs, sf, LR.lattices(img, R.GAUSS_SXY / sf, R.BILATERAL_SXY / sf, R.BILATERAL_SRGB))
    return _CRF_LATS[name]


@pytest.mark.parametrize("t", [1, 4])
@pytest.mark.parametrize("name", list(_CRF))
def test_crf_inference_lattice(name, t):
    from muscle_amd.crf import crf_inference, crf_run
    img, probs, sf, lats = _crf_case(name)
    q64 = LR.crf_lattice_ref(img, probs, t, sf, lats=lats)
    q32 = LR.crf_lattice_ref(img, probs, t, sf, dtype=np.float32, lats=lats)
    assert q32.dtype == np.float32
    q = crf_inference(img, probs.astype(np.float32), t=t, scale_factor=sf, pairwise="lattice")
    torch.cuda.synchronize()
    assert q.is_cuda and q.dtype == torch.float32
    q = q.cpu().numpy()
    assert np.isfinite(q).all() and np.abs(q.sum(0) - 1).max() <= 1e-5
    _bound(float(np.abs(q - q64).max()), float(np.abs(q32.astype(np.float64) - q64).max()), q64, f"crf {name} t={t}")
    q2, pred = crf_run(T(img).to(DEV), T(probs.astype(np.float32)).to(DEV), t, sf, 21, 0.5, 4.0, want_pred=True, pairwise="lattice")
    assert np.array_equal(q2.cpu().numpy(), q) and np.array_equal(pred.cpu().numpy(), q.argmax(0))
    print(f"  labels changed by the CRF {(q64.argmax(0) != probs.argmax(0)).mean():.3f}")


def test_crf_t0_and_default_is_window():
    from muscle_amd.crf import crf_inference
    img, probs, sf, _ = _crf_case("std_sf6")
    p32 = probs.astype(np.float32)
    q0 = crf_inference(img, p32, t=0, scale_factor=sf, pairwise="lattice").cpu().numpy()
    assert np.abs(q0 - R.crf_ref(img, probs, 0, sf)).max() <= 1e-6
    a = crf_inference(img, p32, t=2, scale_factor=sf)
    b = crf_inference(img, p32, t=2, scale_factor=sf, pairwise="window")
    c = crf_inference(img, p32, t=2, scale_factor=sf, pairwise="lattice")
    assert torch.equal(a, b)                                    # the default, bit for bit
    assert float((a - c).abs().max()) > 1e-3                    # no silent fallback: a different model


# ---- the label CRF and the IR labels ----------------------------------------------------------------------------------------------

LABEL_CASES = ["a_40x56", "c_37x53", "d_24x40", "e_24x40", "f_9x45", "f_70x5"]
_IRL = {}


def _irl(name):
    """(img, cams, keys, fp64 reference dict, e32, device (conf, pred2, q)), computed once."""
    if name not in _IRL:
        from muscle_amd.ir_label import ir_label_run
        img, cams, keys, _ = IR.case(name)
        lats = LR.lattices(img, IR.GAUSS_SXY, IR.BILATERAL_SXY, IR.BILATERAL_SRGB)
        r64 = LR.ir_label_lattice_ref(img, cams, keys, lats=lats)
        q32 = LR.ir_label_lattice_ref(img, cams, keys, dtype=np.float32, lats=lats)["q"]
        assert q32.dtype == np.float32
        e32 = float(np.abs(q32.astype(np.float64) - r64["q"]).max())
        conf, pred2, q = ir_label_run(img, cams, keys.tolist(), pairwise="lattice", want_pred=True, want_q=True)
        torch.cuda.synchronize()
        _IRL[name] = (img, cams, keys, r64, e32, (conf.cpu().numpy(), pred2.cpu().numpy(), q.cpu().numpy()))
    return _IRL[name]


@pytest.mark.parametrize("name", LABEL_CASES)
def test_ir_label_lattice(name):
    img, cams, keys, r64, e32, (conf, pred2, q) = _irl(name)
    q64 = r64["q"]
    assert np.isfinite(q).all() and np.abs(q.sum(1) - 1).max() <= 1e-5
    _bound(float(np.abs(q - q64).max()), e32, q64, f"ir_label {name}")
    ok = IR.top2_gap(q64) >= GAP
    both = ok[0] & ok[1]
    print(f"  left out: pred {1 - ok.mean():.4f} conf {1 - both.mean():.4f}; labels changed by the CRF {(r64['pred'] != r64['labs']).mean():.3f}")
    assert 1 - ok.mean() <= MAX_LEFT_OUT and 1 - both.mean() <= MAX_LEFT_OUT
    assert np.array_equal(pred2[ok], r64["pred"][ok])
    assert np.array_equal(conf[both], r64["conf"][both])
    assert np.array_equal(pred2, q.argmax(1))
    assert np.array_equal(conf, IR.combine_conf(keys[pred2[0]], keys[pred2[1]]))
    assert (r64["pred"] != r64["labs"]).mean() > 0.01           # the CRF moves labels: the comparison is not vacuous


@pytest.mark.parametrize("name", LABEL_CASES)
def test_crf_inference_label_lattice(name):
    """One problem per call on each thresholded map: the same Q bound, the same argmax rule."""
    from muscle_amd.crf import crf_inference_label, crf_label_run
    img, cams, keys, r64, e32, (_, pred2, q) = _irl(name)
    L = len(keys)
    for g in range(2):
        q1, p1 = crf_label_run(img, r64["labs"][g], IR.T, L, IR.GT_PROB, 4.0, want_q=True, pairwise="lattice")
        torch.cuda.synchronize()
        q1, p1 = q1.cpu().numpy(), p1.cpu().numpy()
        _bound(float(np.abs(q1 - r64["q"][g]).max()), e32, r64["q"][g], f"crf_label {name} problem {g}")
        ok = IR.top2_gap(r64["q"][g]) >= GAP
        assert 1 - ok.mean() <= MAX_LEFT_OUT
        assert np.array_equal(p1[ok], r64["pred"][g][ok]) and np.array_equal(p1, q1.argmax(0))
    p0 = crf_inference_label(T(img).to(DEV), T(r64["labs"][0]).to(DEV), n_labels=L, pairwise="lattice")
    assert p0.is_cuda and p0.dtype == torch.uint8
    ok = IR.top2_gap(r64["q"][0]) >= GAP
    assert np.array_equal(p0.cpu().numpy()[ok], r64["pred"][0][ok])


def test_lattice_is_not_the_window_and_default_is_window():
    from muscle_amd.ir_label import ir_label_run
    img, cams, keys, r64, e32, (conf, pred2, q) = _irl("a_40x56")
    a = ir_label_run(img, cams, keys.tolist(), want_pred=True, want_q=True)
    b = ir_label_run(img, cams, keys.tolist(), want_pred=True, want_q=True, pairwise="window")
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y)                                # the default, bit for bit
    d = float(np.abs(a[2].cpu().numpy() - q).max())
    print("lattice against window, a_40x56: max|dQ| =", d, "labels that differ:", float((a[1].cpu().numpy() != pred2).mean()))
    assert d > 1e-3                                             # no silent fallback: a different model
    # t = 0: Q_0 and the thresholded maps, both backends
    c0, p0, q0 = ir_label_run(img, cams, keys.tolist(), t=0, want_pred=True, want_q=True, pairwise="lattice")
    assert np.array_equal(p0.cpu().numpy(), r64["labs"])
    assert np.abs(q0.cpu().numpy() - IR.crf_labels(img, r64["labs"], len(keys), t=0)).max() <= 1e-6
    assert np.array_equal(c0.cpu().numpy(), IR.combine_conf(keys[r64["labs"][0]], keys[r64["labs"][1]]))


# ---- the script and infer_seg -----------------------------------------------------------------------------------------------------

def test_script_and_infer_seg(tmp_path):
    """python -m muscle_amd.cam_to_ir_label --crf_pairwise lattice once, in a fresh process, on two tiny images: the PNGs equal
    cam_to_ir_label(pairwise="lattice") on the decoded JPEGs.  infer_seg(crf_img=..., crf_pairwise="lattice") is
    crf_inference(pairwise="lattice") on the map without the CRF."""
    import PIL.Image
    from muscle_amd.ir_label import cam_to_ir_label
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (tmp_path / "cam").mkdir()
    names = ["2007_000033", "2007_000042"]
    dicts = {}
    for n, (nm, (h, w, c)) in enumerate(zip(names, [(24, 40, 3), (37, 21, 1)])):
        img, cams, keys = IR.synthetic(80 + n, h, w, c)
        PIL.Image.fromarray(img, "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=95)
        dicts[nm] = {int(k) - 1: cams[i] for i, k in enumerate(keys[1:])}
        np.save(tmp_path / "cam" / f"{nm}.npy", dicts[nm])
    (tmp_path / "list.txt").write_text("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in names))
    r = subprocess.run([sys.executable, "-m", "muscle_amd.cam_to_ir_label", "--voc12_root", str(root), "--infer_list",
                        str(tmp_path / "list.txt"), "--cam_dir", str(tmp_path / "cam"), "--ir_label_out_dir", str(tmp_path / "out"),
                        "--num_workers", "1", "--crf_pairwise", "lattice"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    differ = 0
    for nm in names:
        jpg = np.array(PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB"))
        png = np.array(PIL.Image.open(tmp_path / "out" / f"{nm}.png"))
        want = cam_to_ir_label(jpg, dicts[nm], pairwise="lattice").cpu().numpy()
        assert np.array_equal(png, want), nm
        differ += int((want != cam_to_ir_label(jpg, dicts[nm]).cpu().numpy()).sum())
    assert differ > 0                                           # not the windowed maps

    import muscle_amd
    from muscle_amd.crf import crf_inference
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    seed, H, W, K = 61, 72, 96, 21
    sd = synth.synth_state_dict(net_cfg("efficientnet-b0", True), seed, mode="dec", layers=3)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec")
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    model = model.to(DEV).eval()
    img = _noisy(seed, H, W)
    imgs = MSFStager(DEV)(PIL.Image.fromarray(img, "RGB"), (1.0,))
    _, prob0 = infer_seg(model, imgs, H, W, return_prob=True)
    pred, q = infer_seg(model, imgs, H, W, return_prob=True, crf_img=img, crf_pairwise="lattice")
    ref = crf_inference(img, prob0, t=4, labels=K, pairwise="lattice")
    assert torch.equal(q, ref) and torch.equal(pred.cpu(), T(ref.cpu().numpy().argmax(0).astype(np.uint8)))
    _, qw = infer_seg(model, imgs, H, W, return_prob=True, crf_img=img)
    assert not torch.equal(q, qw)
