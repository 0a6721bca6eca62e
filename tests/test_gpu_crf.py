"""GPU parity of the dense CRF (muscle_amd.crf / mx_crf_inference; src/imutils.py:439-456) against the numpy restatement of
its model in crf_ref.py, WITH THE SAME WINDOW: unary and Q_0, the normalisers, Q_t, the label maps, run-to-run and
output-selection bits, infer_seg(crf_img=...), the command line with --crf 2, and one full-size run.

Tolerance of the Q_t comparisons: e32 = max|Q_float32-numpy - Q_fp64| is computed at run time for the same input (what fp32
rounding alone does to the model, reference arithmetic on the CPU) and the kernel must stay within F * e32 + 1e-7.
F = 4 is twice the worst ratio max|Q_gpu - Q_fp64| / e32 measured over all cases below, rounded up (profiles/crf_bench.txt
lists them); the kernel is deterministic, so the margin is for other inputs, not for noise."""
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import crf_ref as R
from muscle_amd import synth
from muscle_amd.arch import net_cfg

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
F_TOL = 4.0


def _synthetic(seed, H, W, L):
    """A blocky noisy image and a smooth probability map of any size (the construction of the standard image)."""
    import scipy.ndimage
    g = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    img[:, :W // 3] = [200, 30, 30]
    img[H // 4:3 * H // 4, W // 3:4 * W // 5] = [20, 180, 60]
    img[:, 4 * W // 5:] = [30, 40, 200]
    img = np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)
    lab = np.zeros((H, W), int)
    lab[:, :2 * W // 5] = 1 % L
    lab[H // 5:4 * H // 5, W // 4:6 * W // 7] = (L - 1) // 2
    lab[:, 3 * W // 4:] = L - 1
    logit = g.normal(0, 1.0, (L, H, W))
    for k in range(L):
        logit[k] += 2.5 * (lab == k)
    logit = scipy.ndimage.gaussian_filter(logit, (0, 3, 3)) * 3
    probs = np.exp(logit)
    probs /= probs.sum(0, keepdims=True)
    return img, probs


def _case(name):
    """(img, probs, scale_factor, trunc)"""
    if name.startswith("std"):
        img, probs = R.standard_input()
        return img, probs, (6.0 if name == "std_sf6" else 1.5), 4.0
    if name == "ragged_37x53":
        return _synthetic(1, 37, 53, 21) + (6.0, 4.0)
    if name == "two_labels":
        return _synthetic(2, 40, 56, 2) + (6.0, 4.0)
    if name == "narrow_45x9":                                  # narrower than one 16-pixel tile, window cut inside it
        return _synthetic(3, 45, 9, 21) + (12.0, 4.0)
    if name == "short_5x70":                                   # lower than one 8-row tile
        return _synthetic(4, 5, 70, 5) + (6.0, 4.0)
    if name == "mid_64x96":                                    # R_bilateral = 43: several source tiles, cut by all four borders
        return _synthetic(5, 64, 96, 21) + (1.5, 2.0)
    raise KeyError(name)


def _gpu(img, probs, t, sf, trunc, labels=None, want_q=True, want_pred=True):
    from muscle_amd.crf import crf_run
    q, pred = crf_run(img, probs.astype(np.float32), t, sf, labels or probs.shape[0], 0.5, trunc, want_q=want_q, want_pred=want_pred)
    torch.cuda.synchronize()
    return (None if q is None else q.cpu().numpy()), (None if pred is None else pred.cpu().numpy())


_REF = {}


def _refs(name, t):
    """(Q_fp64, e32) of a case, the fp64 reference on the float32 copy of probs (what the kernel is given)."""
    if (name, t) not in _REF:
        img, probs, sf, trunc = _case(name)
        p32 = probs.astype(np.float32)
        q64 = R.crf_ref(img, p32, t, sf, 0.5, trunc, np.float64)
        q32 = R.crf_ref(img, p32, t, sf, 0.5, trunc, np.float32)
        assert q32.dtype == np.float32
        _REF[(name, t)] = (q64, float(np.abs(q32.astype(np.float64) - q64).max()))
    return _REF[(name, t)]


def _margin(q):
    s = np.sort(q, 0)
    return s[-1] - s[-2] if q.shape[0] > 1 else np.ones(q.shape[1:])


def test_unary_and_q0():
    """t = 0: Q_0 = softmax(-U) of the clipped, confidence-mixed map; a pixel with probs == 0 in a channel, a pixel whose
    mixed value needs the 1e-5 clip from below (confidence 1) and an un-normalised, --cls_dir-scaled map (values > 1 hit the
    upper clip)."""
    img, probs = R.standard_input()
    probs = probs.copy()
    probs[4, 3, 5] = 0.0
    probs[:, 7, 9] = 0.0
    probs[2, 7, 9] = 1.0
    scaled = probs.copy()
    scaled[1:] *= np.linspace(0.0, 3.0, 20)[:, None, None]
    for p, conf in ((probs, 0.5), (probs, 1.0), (scaled, 0.5), (scaled * 4, 0.9)):
        from muscle_amd.crf import crf_run
        q, pred = crf_run(img, p.astype(np.float32), 0, 1.5, 21, conf, 4.0, want_q=True, want_pred=True)
        ref = R.crf_ref(img, p.astype(np.float32), 0, confidence=conf)
        got = q.cpu().numpy()
        print("q0 err", conf, float(np.abs(got - ref).max()))
        assert np.abs(got - ref).max() <= 1e-6                 # a few ulp of values <= 1: one log, one exp, one division
        ok = _margin(ref) > 4e-6
        assert np.array_equal(pred.cpu().numpy()[ok], ref.argmax(0)[ok])
        assert np.array_equal(pred.cpu().numpy(), got.argmax(0))
    assert ref[:, 7, 9].min() > 0                              # the clip keeps every label alive


def _gpu_normalizers(img, sf, trunc):
    from muscle_amd._lib import call, lib, ptr, stream
    H, W = img.shape[:2]
    ws = torch.empty(lib().mx_crf_workspace_bytes(1, H, W) // 4, device=DEV)
    ng = torch.full((H, W), -1.0, device=DEV)
    nb = torch.full((H, W), -1.0, device=DEV)
    im = T(np.ascontiguousarray(img)).to(DEV)
    call("mx_crf_normalizers", ptr(im), H, W, R.GAUSS_SXY / sf, R.BILATERAL_SXY / sf, R.BILATERAL_SRGB, trunc, ptr(ws), ptr(ng),
         ptr(nb), stream())
    torch.cuda.synchronize()
    return ng.cpu().numpy(), nb.cpu().numpy()


@pytest.mark.parametrize("sf", [1.5, 6.0])
def test_normalizers(sf):
    """n_m = 1 / sqrt(window sum of k_m): window covering the image (1.5) and cut inside it (6).  Relative tolerance 2e-6: the
    sums are of positive terms (no cancellation), every weight carries ~4 roundings of 6e-8."""
    img, _ = R.standard_input()
    ng, nb = _gpu_normalizers(img, sf, 4.0)
    rg, rb = R.normalizers(img, sf, 4.0)
    eg, eb = float(np.abs(ng / rg - 1).max()), float(np.abs(nb / rb - 1).max())
    print("normaliser rel err", sf, eg, eb)
    assert eg <= 2e-6 and eb <= 2e-6


def test_normalizers_flat_image():
    """On a flat-colour image the colour term is 1: the bilateral normaliser is a Gaussian one of sxy = 32 / scale_factor."""
    H, W, sf = 33, 47, 6.0
    img = np.full((H, W, 3), (90, 200, 17), np.uint8)
    _, nb = _gpu_normalizers(img, sf, 4.0)
    yy, xx = np.mgrid[0:H, 0:W]
    xy = np.stack([xx.ravel(), yy.ravel()], 1)
    sb = R.BILATERAL_SXY / sf
    k = R.Kernel(xy / sb, xy, R.radius(4.0, sb), np.float64)
    ref = (1.0 / np.sqrt(k.apply(np.ones(H * W)) + 1e-20)).reshape(H, W)
    assert np.abs(nb / ref - 1).max() <= 2e-6
    rb = R.normalizers(img, sf, 4.0)[1]
    assert np.abs(rb / ref - 1).max() <= 1e-12


CASES = [("std_sf1.5", 1), ("std_sf1.5", 4), ("std_sf6", 1), ("std_sf6", 4), ("ragged_37x53", 4), ("two_labels", 4),
         ("narrow_45x9", 4), ("short_5x70", 4), ("mid_64x96", 4)]


@pytest.mark.parametrize("name,t", CASES)
def test_q_vs_fp64(name, t):
    """Q_t and the label map against the fp64 restatement with the same window."""
    img, probs, sf, trunc = _case(name)
    q64, e32 = _refs(name, t)
    q, pred = _gpu(img, probs, t, sf, trunc)
    err = float(np.abs(q.astype(np.float64) - q64).max())
    tol = F_TOL * e32 + 1e-7
    print(f"crf case {name} t={t}: err={err:.3e} e32={e32:.3e} ratio={err / max(e32, 1e-30):.3f}")
    assert np.isfinite(q).all()
    assert err <= tol, (err, e32)
    ok = _margin(q64) > 2 * tol
    assert ok.mean() >= 0.99
    assert np.array_equal(pred[ok], q64.argmax(0)[ok])
    assert np.array_equal(pred, q.argmax(0))
    assert np.abs(q.sum(0) - 1).max() <= 1e-5


@pytest.mark.parametrize("name", ["std_sf1.5", "std_sf6"])
def test_labels_standard_image(name):
    """No pixel of the standard image is exempt from the label comparison (the restatement's smallest top-2 margin is above
    1e-2 in both settings), and the CRF is not a no-op: it changes at least 5 % of the labels (restatement: 13.5 % / 12.8 %)."""
    img, probs, sf, trunc = _case(name)
    q64, e32 = _refs(name, 4)
    assert _margin(q64).min() > 1e-2 > 2 * (F_TOL * e32 + 1e-7)
    _, pred = _gpu(img, probs, 4, sf, trunc, want_q=False)
    assert np.array_equal(pred, q64.argmax(0))
    changed = float((pred != probs.argmax(0)).mean())
    print("labels changed", name, changed)
    assert changed >= 0.05


def test_all_pairs_trunc():
    """trunc <= 0 is all pairs; on the standard image at scale_factor 6 it differs from trunc = 4 as the restatement says."""
    img, probs = R.standard_input()
    p32 = probs.astype(np.float32)
    qa, _ = _gpu(img, probs, 4, 6.0, 0.0)
    ra = R.crf_ref(img, p32, 4, 6.0, 0.5, 0.0)
    r32 = R.crf_ref(img, p32, 4, 6.0, 0.5, 0.0, np.float32)
    e32 = float(np.abs(r32 - ra).max())
    assert np.abs(qa - ra).max() <= F_TOL * e32 + 1e-7
    q4, _ = _gpu(img, probs, 4, 6.0, 4.0)
    d = float(np.abs(q4 - qa).max())
    assert 2e-5 <= d <= 1e-3, d                                # restatement: 7.7e-5


def test_output_selection_and_repeat_bits():
    img, probs, sf, trunc = _case("ragged_37x53")
    q, pred = _gpu(img, probs, 4, sf, trunc)
    q1, none = _gpu(img, probs, 4, sf, trunc, want_pred=False)
    none2, p2 = _gpu(img, probs, 4, sf, trunc, want_q=False)
    q3, p3 = _gpu(img, probs, 4, sf, trunc)
    assert none is None and none2 is None
    assert np.array_equal(q, q1) and np.array_equal(q, q3)
    assert np.array_equal(pred, p2) and np.array_equal(pred, p3)
    assert np.abs(q.sum(0) - 1).max() <= 1e-5
    from muscle_amd.crf import crf_inference
    q4 = crf_inference(img, T(probs.astype(np.float32)).to(DEV), t=4, scale_factor=sf)        # device tensor in, public entry
    assert q4.is_cuda and q4.dtype == torch.float32 and np.array_equal(q4.cpu().numpy(), q)
    q5 = crf_inference(T(img).to(DEV), probs.astype(np.float32), scale_factor=sf)               # default t = 2
    assert np.array_equal(q5.cpu().numpy(), _gpu(img, probs, 2, sf, 4.0)[0])


def _sd(name, seed):
    """Synthetic decoder weights with non-identity BatchNorm running statistics."""
    sd = synth.synth_state_dict(net_cfg(name, True), seed, mode="dec", layers=3)
    rng = np.random.default_rng(seed + 1000)
    for k in sorted(sd):
        if k.endswith("running_mean"):
            sd[k] = rng.normal(0.0, 0.5, sd[k].shape).astype(np.float32)
        elif k.endswith("running_var"):
            sd[k] = rng.uniform(0.5, 2.0, sd[k].shape).astype(np.float32)
    return sd


def _model(name, sd):
    import muscle_amd
    m = muscle_amd.MuSCLe(21, name, layers=3, last_pooling=True, mode="dec")
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def test_infer_seg_with_crf():
    """infer_seg(crf_img=img) is crf_inference(img, the map without the CRF, t=4) bit for bit; crf_img=None takes the path
    that has no CRF in it (one mx_seg_infer call: restated here)."""
    import PIL.Image  # noqa: F401
    from muscle_amd._lib import call, ptr, stream
    from muscle_amd.crf import crf_inference
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    seed, H, W, K = 61, 72, 96, 21
    model = _model("efficientnet-b0", _sd("efficientnet-b0", seed))
    img, _ = _synthetic(seed, H, W, K)
    import PIL.Image as PI
    imgs = MSFStager(DEV)(PI.fromarray(img, "RGB"), (0.5, 1.0, 1.25))
    cls = np.linspace(0.2, 1.0, K).astype(np.float32)
    pred0, prob0 = infer_seg(model, imgs, H, W, cls_label=cls, return_prob=True)
    pred0b, prob0b = infer_seg(model, imgs, H, W, cls_label=cls, return_prob=True, crf_img=None)
    assert torch.equal(pred0, pred0b) and torch.equal(prob0, prob0b)
    # the parent's computation: the decoder's low-res logits through one mx_seg_infer launch
    rows, keep = [], []
    with torch.no_grad():
        for n in range(0, len(imgs), 2):                       # a scale and its flip as one batch-2 forward
            lr = model(torch.cat([imgs[n], imgs[n + 1]], dim=0).float(), cam="seg_lr")
            keep.append(lr)
            for b in range(2):
                rows.append([lr[b].data_ptr(), lr.shape[1], lr.shape[2], imgs[n].shape[2], imgs[n].shape[3], b, 0, 0])
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    pp = torch.empty(H, W, dtype=torch.uint8, device=DEV)
    pr = torch.empty(K, H, W, device=DEV)
    call("mx_seg_infer", ptr(tab), len(rows), 24, K, H, W, ptr(T(cls).to(DEV)), ptr(pp), ptr(pr), stream())
    torch.cuda.synchronize()
    assert torch.equal(pp, pred0) and torch.equal(pr, prob0)
    pred, q = infer_seg(model, imgs, H, W, cls_label=cls, return_prob=True, crf_img=img)
    ref = crf_inference(img, prob0, t=4, labels=K)
    assert torch.equal(q, ref)
    assert torch.equal(pred.cpu(), T(ref.cpu().numpy().argmax(0).astype(np.uint8)))
    pred2, none = infer_seg(model, imgs, H, W, cls_label=cls, crf_img=T(img))
    assert none is None and torch.equal(pred2, pred)
    assert not torch.equal(pred, pred0)


def test_cli_crf2(tmp_path):
    """python -m muscle_amd.infer_seg --crf 2 in a fresh process: PNGs equal to infer_seg(crf_img=...)'s pred and different
    from the --crf 0 PNGs."""
    import PIL.Image
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    from muscle_amd.infer_seg import DEFAULT_SCALES
    seed = 67
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    names = ["2007_000033", "2007_000042"]
    for n, (nm, (h, w)) in enumerate(zip(names, [(72, 96), (80, 72)])):
        PIL.Image.fromarray(_synthetic(seed + n, h, w, 21)[0], "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=95)
    (tmp_path / "val.txt").write_text("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in names))
    sd = _sd("efficientnet-b0", seed)
    torch.save({k: T(v) for k, v in sd.items()}, tmp_path / "w.pth")
    env = dict(os.environ, PYTHONPATH=ROOT)
    for crf in ("2", "0"):
        r = subprocess.run([sys.executable, "-m", "muscle_amd.infer_seg", "--weights", str(tmp_path / "w.pth"),
                            "--infer_list", str(tmp_path / "val.txt"), "--voc12_root", str(root), "--pretrained", "b0",
                            "--out_seg", str(tmp_path / f"seg{crf}"), "--crf", crf],
                           cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=80)
        assert r.returncode == 0, r.stderr[-3000:]
    model = _model("efficientnet-b0", sd)
    stager = MSFStager(DEV)
    differ = 0
    for nm in names:
        img = PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB")
        pred, _ = infer_seg(model, stager(img, DEFAULT_SCALES), img.size[1], img.size[0], crf_img=np.asarray(img))
        png2 = np.array(PIL.Image.open(tmp_path / "seg2" / f"{nm}.png"))
        png0 = np.array(PIL.Image.open(tmp_path / "seg0" / f"{nm}.png"))
        assert np.array_equal(png2, pred.cpu().numpy()), nm
        differ += int((png2 != png0).sum())
    assert differ > 0


def test_full_size():
    """375 x 500, 21 labels, t = 4, trunc = 4 (R = 86): finishes, finite, valid labels, columns sum to 1."""
    img, probs = _synthetic(7, 375, 500, 21)
    q, pred = _gpu(img, probs, 4, 1.5, 4.0)
    assert q.shape == (21, 375, 500) and pred.shape == (375, 500)
    assert np.isfinite(q).all() and q.min() >= 0
    assert pred.max() < 21
    assert np.abs(q.sum(0) - 1).max() <= 1e-5
    assert np.array_equal(pred, q.argmax(0))
