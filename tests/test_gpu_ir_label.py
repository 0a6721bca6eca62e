"""GPU parity of IR-label generation (muscle_amd.ir_label / mx_ir_label, mx_crf_label; IRN's cam_to_ir_label around
src/imutils.py:477-491) against the numpy restatement of its model in ir_label_ref.py, WITH THE SAME WINDOW; the fp64 results
are those of tests/golden/ir_label.npz (tests/test_cpu_ir_label.py reproduces that file).

Protocol of the Q_t comparison (the one of tests/test_gpu_crf.py): e32 = max|Q_float32-numpy - Q_fp64| is computed here for the
same case (what fp32 rounding alone does to the model, reference arithmetic on the CPU) and the kernel must stay within 4 * e32.
Labels: pred and conf equal the fp64 ones on every pixel whose fp64 top-two gap is >= 1e-3 in the problems that decide it; at
most 0.5 % of the pixels may be left out (the fixture's smallest gap is 1.5e-3: none is)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import ir_label_ref as IR

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
F_TOL, GAP, MAX_LEFT_OUT = 4.0, 1e-3, 0.005
CASES = list(IR.CASES)

_Z = {}
_E32 = {}
_GPU = {}


def _golden(name):
    """(img, cams float32, keys, trunc, Q_t fp64, pred, conf) from the fixture."""
    if not _Z:
        _Z["z"] = np.load(os.path.join(ROOT, "tests", "golden", "ir_label.npz"))
    z = _Z["z"]
    trunc = IR.CASES[name][4]
    return (z[name + "/img"], z[name + "/cams"].astype(np.float32), z[name + "/keys"].astype(np.int64), trunc, z[name + "/q"],
            z[name + "/pred"], z[name + "/conf"])


def _e32(name):
    """max|Q_float32-numpy - Q_fp64| of a case, computed once."""
    if name not in _E32:
        img, cams, keys, trunc, q64 = _golden(name)[:5]
        q32 = IR.ir_label(img, cams, keys, trunc=trunc, dtype=np.float32)["q"]
        assert q32.dtype == np.float32
        _E32[name] = float(np.abs(q32.astype(np.float64) - q64).max())
    return _E32[name]


def _run(img, cams, keys, trunc, fused=True, t=IR.T, want_pred=True, want_q=True):
    from muscle_amd.ir_label import ir_label_run
    conf, pred2, q = ir_label_run(img, cams, keys.tolist(), trunc=trunc, fused=fused, t=t, want_pred=want_pred, want_q=want_q)
    torch.cuda.synchronize()
    return conf.cpu().numpy(), (None if pred2 is None else pred2.cpu().numpy()), (None if q is None else q.cpu().numpy())


def _gpu(name, fused=True):
    """(conf, pred2, Q_t) of a case on the device, computed once per (case, fused) and left unchanged."""
    if (name, fused) not in _GPU:
        img, cams, keys, trunc = _golden(name)[:4]
        _GPU[(name, fused)] = _run(img, cams, keys, trunc, fused)
    return _GPU[(name, fused)]


@pytest.mark.parametrize("name,fused", [("a_40x56", True), ("a_40x56", False), ("c_37x53", True), ("d_24x40", True), ("e_24x40", True)])
def test_q0_and_label_maps(name, fused):
    """t = 0: both thresholded argmax maps on every pixel and Q_0 = softmax(-U) within 1e-6 (one log, one exp, one division of
    values <= 1).  Pixels are planted whose CAM value equals a threshold bit for bit (background wins), exceeds it by one ulp, and
    where two classes tie above it (the lower class wins)."""
    img, cams, keys, trunc = _golden(name)[:4]
    cams = cams.copy()
    C = cams.shape[0]
    f, b = np.float32(IR.FG_THRES), np.float32(IR.BG_THRES)
    cams[:, 0, 0] = 0.0; cams[C - 1, 0, 0] = f                                  # == fg threshold: fg 0, bg class C
    cams[:, 0, 1] = 0.0; cams[C - 1, 0, 1] = np.nextafter(f, np.float32(1))     # one ulp above: fg class C
    cams[:, 0, 2] = 0.0; cams[0, 0, 2] = b                                      # == bg threshold: both 0
    cams[:, 0, 3] = 0.0; cams[0, 0, 3] = np.nextafter(b, np.float32(1))         # fg 0, bg class 1
    cams[:, 0, 4] = 0.5                                                         # all classes tie: class 1
    conf, pred2, q = _run(img, cams, keys, trunc, fused, t=0)
    labs = IR.label_maps(cams)
    assert labs[:, 0, :5].tolist() == [[0, C, 0, 0, 1], [C, C, 0, 1, 1]]
    assert np.array_equal(pred2, labs)
    ref = IR.crf_labels(img, labs, C + 1, t=0)
    err = float(np.abs(q - ref).max())
    print("q0 err", name, fused, err)
    assert err <= 1e-6
    assert np.array_equal(conf, IR.combine_conf(keys[labs[0]], keys[labs[1]]))


@pytest.mark.parametrize("name", CASES)
def test_q_vs_fp64(name):
    """Q_t, the two argmax maps and conf against the fp64 restatement with the same window."""
    img, cams, keys, trunc, q64, pred64, conf64 = _golden(name)
    e32 = _e32(name)
    conf, pred2, q = _gpu(name)
    err = float(np.abs(q.astype(np.float64) - q64).max())
    print(f"ir_label case {name}: err={err:.3e} e32={e32:.3e} ratio={err / max(e32, 1e-30):.3f}")
    assert np.isfinite(q).all()
    assert np.abs(q.sum(1) - 1).max() <= 1e-5
    assert err <= F_TOL * e32, (err, e32)
    ok = IR.top2_gap(q64) >= GAP                               # [2,H,W]: per problem
    both = ok[0] & ok[1]
    print(f"  left out: pred {1 - ok.mean():.4f} conf {1 - both.mean():.4f}; labels changed by the CRF {(pred64 != IR.label_maps(cams)).mean():.3f}")
    assert 1 - ok.mean() <= MAX_LEFT_OUT and 1 - both.mean() <= MAX_LEFT_OUT
    assert np.array_equal(pred2[ok], pred64[ok])
    assert np.array_equal(conf[both], conf64[both])
    assert np.array_equal(pred2, q.argmax(1))
    assert np.array_equal(conf, IR.combine_conf(keys[pred2[0]], keys[pred2[1]]))
    assert set(np.unique(conf).tolist()) <= {0, 255} | set(keys.tolist())


@pytest.mark.parametrize("name", CASES)
def test_fused_equals_unfused(name):
    """Both problems as columns of one pass and one problem per pass give the same bits: a column depends on its own B column
    and the shared K only, summed in the same order.  (L = 17 runs one problem per pass either way.)"""
    a, b = _gpu(name, True), _gpu(name, False)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["a_40x56", "b_48x72", "c_37x53"])
def test_cross_check_against_mx_crf_inference(name):
    """The existing kernels on the same model: mx_crf_inference with this model's widths and weights, one-hot probabilities and
    confidence (gt_prob - 1/L) / (1 - 1/L) (its unary then is the label unary).  Same argmax; Q_t within twice the fp32 error of
    the restatement (the two unaries are formed by different fp32 expressions)."""
    from muscle_amd._lib import call, lib, ptr, stream
    img, cams, keys, trunc = _golden(name)[:4]
    e32 = _e32(name)
    _, pred2, q = _gpu(name)
    labs = IR.label_maps(cams)
    L, (H, W) = len(keys), img.shape[:2]
    ws = torch.empty(lib().mx_crf_workspace_bytes(L, H, W) // 4, device=DEV)
    im = T(img).to(DEV)
    for g in range(2):
        onehot = T((np.arange(L)[:, None, None] == labs[g][None]).astype(np.float32)).to(DEV)
        qo = torch.empty(L, H, W, device=DEV)
        po = torch.empty(H, W, dtype=torch.uint8, device=DEV)
        call("mx_crf_inference", ptr(im), ptr(onehot), L, H, W, IR.T, IR.one_hot_confidence(L), IR.GAUSS_SXY, IR.GAUSS_W,
             IR.BILATERAL_SXY, IR.BILATERAL_SRGB, IR.BILATERAL_W, trunc, ptr(ws), ptr(qo), ptr(po), stream())
        torch.cuda.synchronize()
        d = float(np.abs(qo.cpu().numpy() - q[g]).max())
        print(f"cross-check {name} problem {g}: |dQ|={d:.3e} e32={e32:.3e}")
        assert np.array_equal(po.cpu().numpy(), pred2[g])
        assert d <= 2 * e32


def test_repeat_bits_and_output_selection():
    img, cams, keys, trunc = _golden("b_48x72")[:4]
    conf, pred2, q = _gpu("b_48x72")
    c1, p1, q1 = _run(img, cams, keys, trunc)
    assert np.array_equal(conf, c1) and np.array_equal(pred2, p1) and np.array_equal(q, q1)
    c2, none_p, none_q = _run(img, cams, keys, trunc, want_pred=False, want_q=False)
    assert none_p is None and none_q is None and np.array_equal(conf, c2)
    c3, p3, none_q = _run(img, cams, keys, trunc, fused=False, want_q=False)
    assert none_q is None and np.array_equal(conf, c3) and np.array_equal(pred2, p3)
    c4, none_p, q4 = _run(img, cams, keys, trunc, want_pred=False)
    assert none_p is None and np.array_equal(conf, c4) and np.array_equal(q, q4)


@pytest.mark.parametrize("name", ["a_40x56", "e_24x40"])
def test_crf_inference_label_is_one_problem(name):
    """crf_inference_label (one problem, G = 1) on each thresholded label map is that problem of the two-problem call."""
    from muscle_amd.crf import crf_inference_label, crf_label_run
    img, cams, keys, trunc = _golden(name)[:4]
    _, pred2, q = _gpu(name)
    labs = IR.label_maps(cams)
    p0 = crf_inference_label(img, labs[0], n_labels=len(keys), trunc=trunc)
    assert p0.is_cuda and p0.dtype == torch.uint8 and np.array_equal(p0.cpu().numpy(), pred2[0])
    q1, p1 = crf_label_run(T(img).to(DEV), T(labs[1]).to(DEV), 10, len(keys), 0.7, trunc, want_q=True)     # device tensors in
    assert np.array_equal(p1.cpu().numpy(), pred2[1]) and np.array_equal(q1.cpu().numpy(), q[1])


def test_cam_to_ir_label_on_a_dict():
    """The public call on an infer_mcl dict (keys in any order, float64 maps) is the ABI call on the stacked maps."""
    from muscle_amd.ir_label import cam_to_ir_label
    img, cams, keys, trunc, _, _, conf64 = _golden("a_40x56")
    conf = _gpu("a_40x56")[0]
    d = {int(k) - 1: cams[n].astype(np.float64) for n, k in reversed(list(enumerate(keys[1:])))}
    got = cam_to_ir_label(img, d, trunc=trunc)
    assert got.is_cuda and got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), conf)
    got = cam_to_ir_label(T(img).to(DEV), {k: T(v).to(DEV) for k, v in d.items()}, fused=False)              # default trunc = 4
    assert np.array_equal(got.cpu().numpy(), conf)
    with pytest.raises(ValueError):
        cam_to_ir_label(img, {})


def test_script_writes_the_labels_train_irn_reads(tmp_path):
    """python -m muscle_amd.cam_to_ir_label once, in a fresh process: three images of two sizes; the PNGs equal cam_to_ir_label
    on the decoded JPEGs, and train_irn's dataset reads them."""
    import PIL.Image
    from muscle_amd.ir_label import cam_to_ir_label
    from muscle_amd.train_irn import VOC12AffinityDataset
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (tmp_path / "cam_sgc").mkdir()
    names = ["2007_000033", "2007_000042", "2007_000061"]
    dicts = {}
    for n, (nm, (h, w, c)) in enumerate(zip(names, [(40, 56, 3), (37, 53, 1), (40, 56, 2)])):
        img, cams, keys = IR.synthetic(70 + n, h, w, c)
        PIL.Image.fromarray(img, "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=95)
        dicts[nm] = {int(k) - 1: cams[i] for i, k in enumerate(keys[1:])}
        np.save(tmp_path / "cam_sgc" / f"{nm}.npy", dicts[nm])
    (tmp_path / "list.txt").write_text("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in names))
    r = subprocess.run([sys.executable, "-m", "muscle_amd.cam_to_ir_label", "--voc12_root", str(root), "--infer_list",
                        str(tmp_path / "list.txt"), "--cam_dir", str(tmp_path / "cam_sgc"), "--ir_label_out_dir",
                        str(tmp_path / "ir_label"), "--num_workers", "2"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-3000:]
    for nm in names:
        jpg = np.array(PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB"))
        png = PIL.Image.open(tmp_path / "ir_label" / f"{nm}.png")
        assert png.mode == "L"
        want = cam_to_ir_label(jpg, dicts[nm]).cpu().numpy()
        assert np.array_equal(np.array(png), want), nm
        assert set(np.unique(want).tolist()) <= {0, 255} | {k + 1 for k in dicts[nm]}
    ds = VOC12AffinityDataset(names, str(root), str(tmp_path / "ir_label"), 32)
    for i in range(len(names)):
        s = ds[i]
        assert s["img"].shape == (3, 32, 32) and s["label"].shape == (8, 8) and s["label"].dtype == np.uint8


def test_full_size():
    """375 x 500, C = 2, t = 10, trunc = 4 (R_b = 200): completes, the bits repeat, the values lie in {0, 255, keys}."""
    img, cams, keys = IR.synthetic(7, 375, 500, 2)
    conf, _, _ = _run(img, cams, keys, 4.0, want_pred=False, want_q=False)
    again, _, _ = _run(img, cams, keys, 4.0, want_pred=False, want_q=False)
    assert conf.shape == (375, 500) and np.array_equal(conf, again)
    vals = set(np.unique(conf).tolist())
    assert vals <= {0, 255} | set(keys.tolist()) and len(vals) >= 2
