"""GPU checks of the class-balanced self-training labels (csrc/selflabel.hip, muscle_amd/selflabel.py) against the numpy
restatement of the rule in selflabel_ref.py.  Everything is exact equality: label, code, the three integer tables, the
selection; then infer_seg's pred against the label, and the two scripts end to end on the smallest decoder."""
import math
import os

import numpy as np
import pytest
import torch

import selflabel_ref as R

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
F = np.float32
T = lambda a: torch.from_numpy(np.array(a))  # noqa: E731  (a copy: the shared references are read-only)

SHAPES = [(1, 1), (1, 7), (7, 1), (5, 5), (67, 130), (130, 67)]      # the last two: several workgroups and a ragged tail
KS = [1, 2, 21, 24]


def _set(prob, i, label, conf, other):
    """Pixel i of prob [K,n]: channel `label` = conf, every other channel = other."""
    prob[:, i] = other
    prob[label, i] = conf


def _case(K, H, W, seed):
    """A random softmax map sharpened so that the codes spread over 1..192, with planted pixels where there is room, and a
    ground truth with void rows and a stripe of values >= K."""
    g = np.random.default_rng(seed)
    n = H * W
    z = g.standard_normal((K, n)) * np.exp(g.uniform(-2.0, 3.5, n))[None]
    e = np.exp(z - z.max(0, keepdims=True))
    prob = (e / e.sum(0, keepdims=True)).astype(np.float32)
    one = F(1.0)
    plant = []
    if K >= 2:
        last = K - 1
        plant += [lambda i: _set(prob, i, 0, F(0.375), F(0.375)),                        # all channels equal: class 0
                  lambda i: (_set(prob, i, last, F(0.5), F(0.125)), prob.__setitem__((0, i), F(0.5))),      # exact tie of 0 and K-1
                  lambda i: _set(prob, i, last, one, F(0.0)),                            # conf exactly 1
                  lambda i: _set(prob, i, last, F(1.25), F(0.0)),                        # above 1
                  lambda i: _set(prob, i, 0, F(np.nan), F(0.75)),                        # a NaN winner: channel 0 is never displaced
                  lambda i: _set(prob, i, last, F(np.nan), F(0.25)),                     # a NaN loser: class 0 wins with 0.25
                  lambda i: _set(prob, i, last, F(0.0), F(-1.0)),                        # conf 0, and below
                  lambda i: _set(prob, i, last, F(-0.5), F(-1.0))]
        if K >= 3:
            plant.append(lambda i: (_set(prob, i, 1, F(0.25), F(0.0625)), prob.__setitem__((K - 1, i), F(0.25))))   # tie: the first wins
        for e_ in range(1, 25):                                                          # conf = 1 - 2^-e
            plant.append(lambda i, e_=e_: _set(prob, i, e_ % K, one - F(2.0 ** -e_), F(0.0)))
        for e_ in (1, 4, 12):                                                            # the fp32 neighbours of three boundaries
            b = one - F(2.0 ** -e_)
            plant.append(lambda i, b=b: _set(prob, i, last, np.nextafter(b, F(0)), F(0.0)))
            plant.append(lambda i, b=b: _set(prob, i, last, np.nextafter(b, F(2)), F(0.0)))
    else:
        plant += [lambda i: _set(prob, i, 0, one, one), lambda i: _set(prob, i, 0, F(np.nan), F(np.nan)),
                  lambda i: _set(prob, i, 0, F(1.5), F(1.5)), lambda i: _set(prob, i, 0, F(0.0), F(0.0))]
        for e_ in range(1, 25):
            plant.append(lambda i, e_=e_: _set(prob, i, 0, one - F(2.0 ** -e_), F(0.0)))
    where = g.permutation(n)[:len(plant)]                                                # small maps take the first few
    for f, i in zip(plant, where):
        f(int(i))
    prob = prob.reshape(K, H, W)
    gt = g.integers(0, K, (H, W)).astype(np.uint8)
    lab = R.scan_argmax(prob)[0]
    agree = g.random((H, W)) < 0.6
    gt[agree] = lab[agree]
    gt[::5] = 255                                                                        # void rows
    gt[:, W // 2] = np.where(np.arange(H) % 2, K, 254)                                   # a stripe of values >= K
    return prob, gt


_CASES = {}


def _ref(K, H, W):
    """(prob, gt, label, code, hist, val, hit), computed once per (K, shape) and left unchanged."""
    key = (K, H, W)
    if key not in _CASES:
        prob, gt = _case(K, H, W, 1000 * K + 10 * H + W)
        label, conf = R.scan_argmax(prob)
        code = R.code_fast(conf)
        for a in (prob, gt, label, code):
            a.setflags(write=False)
        _CASES[key] = (prob, gt, label, code) + R.tables(label, code, gt, K)
    return _CASES[key]


def test_the_inputs_spread_over_the_scale():
    """What the other tests rely on: the vectorised reference code equals the scalar one, the sharpened maps use the scale,
    and the planted pixels are there."""
    prob, gt, label, code, hist, val, hit = _ref(21, 67, 130)
    assert np.array_equal(code, R.code(R.scan_argmax(prob)[1]))
    used = np.unique(code)
    assert used.min() == 0 and 255 in used and 193 in used and 1 in used and len(used) > 120
    assert (np.unique(label).size == 21) and hist.sum() == 67 * 130 and 0 < hit.sum() < val.sum() < hist.sum()
    with np.errstate(invalid="ignore"):
        assert np.isnan(prob).sum() == 2 and (prob > 1).sum() == 1


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_conf_code_vs_reference(K, shape):
    from muscle_amd import selflabel as SL
    H, W = shape
    prob, gt, label, code, hist, val, hit = _ref(K, H, W)
    p, g = T(prob).to(DEV), T(gt).to(DEV)
    st = SL.ConfStats(DEV, K)
    lab, cd = st.add(p, g)
    assert lab.dtype == cd.dtype == torch.uint8 and lab.shape == cd.shape == (H, W)
    assert np.array_equal(lab.cpu().numpy(), label) and np.array_equal(cd.cpu().numpy(), code)
    got = st.tables()
    for a, b, nm in zip(got, (hist, val, hit), ("hist", "val", "hit")):
        assert a.dtype == np.int64 and np.array_equal(a, b), nm
    lab2, cd2 = st.add(p)                                              # without gt: hist alone; two calls accumulate to the sum
    assert torch.equal(lab2, lab) and torch.equal(cd2, cd)
    st.add(p, g)
    for a, b, nm in zip(st.tables(), (3 * hist, 2 * val, 2 * hit), ("hist", "val", "hit")):
        assert np.array_equal(a, b), nm
    lab3, cd3 = SL.conf_code(p)                                        # no stats: the maps alone
    assert torch.equal(lab3, lab) and torch.equal(cd3, cd)
    # mx_code_hist on the stored pair gives the same tables
    st2 = SL.ConfStats(DEV, K)
    st2.add_coded(lab, cd, g)
    for a, b in zip(st2.tables(), (hist, val, hit)):
        assert np.array_equal(a, b)
    st2.add_coded(lab.reshape(-1), cd.reshape(-1))
    assert np.array_equal(st2.tables()[0], 2 * hist) and np.array_equal(st2.tables()[1], val)


def test_two_runs_give_identical_tables():
    from muscle_amd import selflabel as SL
    prob, gt, *_ = _ref(21, 130, 67)
    p, g = T(prob).to(DEV), T(gt).to(DEV)
    runs = []
    for _ in range(2):
        st = SL.ConfStats(DEV, 21)
        lab, cd = st.add(p, g)
        runs.append((lab.cpu(), cd.cpu()) + tuple(T(t) for t in st.tables()))
    assert all(torch.equal(a, b) for a, b in zip(*runs))


def test_code_hist_ignores_labels_beyond_k():
    from muscle_amd import selflabel as SL
    K = 21
    _, gt, label, code, *_ = _ref(K, 67, 130)
    lab = label.copy()
    lab[3::7, ::3] = 21
    lab[::11, 1::5] = 255
    cd = code.copy()
    cd[5::9] = 200                                                     # an unused code in a stored map: counted as 255
    st = SL.ConfStats(DEV, K)
    st.add_coded(T(lab).to(DEV), T(cd).to(DEV), T(gt).to(DEV))
    ref = R.tables(lab, np.where(cd == 200, 255, cd), gt, K)
    for a, b in zip(st.tables(), ref):
        assert np.array_equal(a, b)
    assert ref[0].sum() == (lab < K).sum() < lab.size


@pytest.mark.parametrize("K", KS)
@pytest.mark.parametrize("shape", [(1, 1), (5, 5), (67, 130), (130, 67)], ids=lambda s: "%dx%d" % s)
def test_select_vs_reference(K, shape):
    from muscle_amd import selflabel as SL
    H, W = shape
    _, _, label, code, hist, _, _ = _ref(K, H, W)
    lab, cd = T(label).to(DEV), T(code).to(DEV)
    tcs = [SL.thresholds(hist, p) for p in (0.2, 0.5, 1.0)] + [np.zeros(K, np.uint8), SL.thresholds(hist, 1.0, min_conf=0.9)]
    for p, tc in zip((0.2, 0.5, 1.0, None, None), tcs):
        if p is not None:
            assert np.array_equal(tc, R.thresholds(hist, p))
        out, kept = SL.select(lab, cd, tc)
        ro, rk = R.select(label, code, tc)
        assert out.dtype == torch.uint8 and out.shape == (H, W) and kept.dtype == torch.int64 and kept.shape == (K, 2)
        assert np.array_equal(out.cpu().numpy(), ro) and np.array_equal(kept.cpu().numpy(), rk)
        if p is not None:                                              # at least the portion of every class, NaN pixels apart
            need = np.minimum(hist[:, :194].sum(1), np.ceil(p * hist.sum(1)))
            assert np.all(rk[:, 0] >= need) and np.array_equal(rk[:, 1], hist.sum(1))
    full, _ = SL.select(lab, cd, T(tcs[2]).to(DEV))                    # portion 1.0 (tcode on the device): the map back, NaN pixels apart
    assert np.array_equal(full.cpu().numpy(), np.where(code == 255, 255, label))


def test_select_drops_labels_beyond_k():
    from muscle_amd import selflabel as SL
    K = 21
    _, _, label, code, *_ = _ref(K, 130, 67)
    lab = label.copy()
    lab[2::5, ::4] = 21
    lab[::13] = 255
    lab[1::13] = 24
    tc = np.full(K, 193, np.uint8)
    out, kept = SL.select(T(lab).to(DEV), T(code).to(DEV), tc)
    ro, rk = R.select(lab, code, tc)
    assert np.array_equal(out.cpu().numpy(), ro) and np.array_equal(kept.cpu().numpy(), rk)
    assert (ro[lab >= K] == 255).all() and rk[:, 1].sum() == (lab < K).sum()
    flat, kf = SL.select(T(lab).to(DEV).reshape(-1), T(code).to(DEV).reshape(-1), tc)      # any shape: n pixels
    assert np.array_equal(flat.cpu().numpy(), ro.reshape(-1)) and torch.equal(kf, kept)


# ---- end to end: the smallest decoder the seg tests use, random weights, two scales plus flips, 48 x 64 --------------------------

H0, W0, SCALES = 48, 64, (0.75, 1.0)              # smallest pass 36 x 48: above the backbone's static-padding minimum
NAMES = ["2007_000032", "2007_000039", "2007_000063"]


@pytest.fixture(scope="module")
def tree(tmp_path_factory):
    """A VOC-shaped tree of three 48 x 64 images, weights on disk and the model; shared, never modified."""
    import PIL.Image
    from test_gpu_seg_infer import _model, _sd
    tmp = tmp_path_factory.mktemp("selflabel")
    root = tmp / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    g = np.random.default_rng(61)
    for nm in NAMES:
        yy, xx = np.mgrid[:H0, :W0]
        img = np.stack([(yy * 5 + g.integers(0, 40)) % 256, (xx * 4 + g.integers(0, 40)) % 256, ((yy + xx) * 3) % 256], -1)
        img = np.clip(img + g.integers(-30, 30, img.shape), 0, 255).astype(np.uint8)
        PIL.Image.fromarray(img, "RGB").save(root / "JPEGImages" / f"{nm}.jpg")
        PIL.Image.fromarray(g.choice([0, 1, 4, 12, 255], size=(H0, W0)).astype(np.uint8), "L").save(root / "SegmentationClass" / f"{nm}.png")
    (tmp / "val.txt").write_text("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in NAMES))
    sd = _sd("efficientnet-b0", 61)
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, tmp / "w.pth")
    base = ["--weights", str(tmp / "w.pth"), "--infer_list", str(tmp / "val.txt"), "--voc12_root", str(root), "--num_classes", "21",
            "--bifpn", "3", "--pretrained", "b0", "--scales", ",".join(str(s) for s in SCALES)]
    return {"tmp": tmp, "root": root, "model": _model("efficientnet-b0", sd), "base": base}


def _passes(tree, nm):
    import PIL.Image
    from muscle_amd.data import MSFStager
    img = PIL.Image.open(tree["root"] / "JPEGImages" / f"{nm}.jpg").convert("RGB")
    assert img.size == (W0, H0)
    return MSFStager(DEV)(img, SCALES), np.asarray(img, dtype=np.uint8)


def _png(path):
    import PIL.Image
    im = PIL.Image.open(path)
    assert im.mode == "L"
    return np.array(im)


@pytest.mark.parametrize("crf", [False, True], ids=["mean", "crf"])
def test_label_is_infer_segs_pred(tree, crf):
    from muscle_amd import conf_code
    from muscle_amd.infer import infer_seg
    for nm in NAMES[:2]:
        passes, img = _passes(tree, nm)
        assert len(passes) == 4
        pred, prob = infer_seg(tree["model"], passes, H0, W0, return_prob=True, crf_img=img if crf else None)
        label, code = conf_code(prob)
        assert torch.equal(label, pred)
        p = prob.cpu().numpy()
        assert np.isfinite(p).all() and np.array_equal(label.cpu().numpy(), p.argmax(0))
        assert np.array_equal(code.cpu().numpy(), R.code_fast(p.max(0)))


def test_scripts_end_to_end(tree, tmp_path, capsys):
    from muscle_amd import infer_seg as script, selflabel as SL
    from muscle_amd.infer import infer_seg, save_seg_png
    gt_dir = str(tree["root"] / "SegmentationClass")
    # without --out_conf: the files of infer_seg() + save_seg_png, byte for byte, and the printed lines of before
    assert script.main(tree["base"] + ["--out_seg", str(tmp_path / "seg0")]) == 0
    progress = [f"{nm} {i}" for i, nm in enumerate(NAMES)]
    assert [ln for ln in capsys.readouterr().out.splitlines() if ln[:4] == "2007"] == progress
    probs = {}
    for nm in NAMES:
        pred, prob = infer_seg(tree["model"], _passes(tree, nm)[0], H0, W0, return_prob=True)
        save_seg_png(str(tmp_path / "direct.png"), pred)
        assert (tmp_path / "seg0" / f"{nm}.png").read_bytes() == (tmp_path / "direct.png").read_bytes(), nm
        probs[nm] = (pred.cpu().numpy(), prob.cpu().numpy())
    assert sorted(os.listdir(tmp_path / "seg0")) == [f"{nm}.png" for nm in NAMES]
    # with --out_conf: the same label maps, the code maps, the statistics and the curve
    assert script.main(tree["base"] + ["--out_seg", str(tmp_path / "seg"), "--out_conf", str(tmp_path / "conf"), "--gt_dir", gt_dir]) == 0
    lines = capsys.readouterr().out.splitlines()
    assert lines[-11].startswith("portion") and [float(ln.split()[0]) for ln in lines[-10:]] == [i / 10 for i in range(1, 11)]
    assert sorted(os.listdir(tmp_path / "conf")) == [f"{nm}.png" for nm in NAMES] + ["stats.npz"]
    ref = [np.zeros((21, 256), np.int64) for _ in range(3)]
    for nm in NAMES:
        assert (tmp_path / "seg" / f"{nm}.png").read_bytes() == (tmp_path / "seg0" / f"{nm}.png").read_bytes()
        pred, prob = probs[nm]
        code = _png(tmp_path / "conf" / f"{nm}.png")
        assert np.array_equal(code, R.code_fast(prob.max(0)))
        for a, b in zip(ref, R.tables(pred, code, _png(os.path.join(gt_dir, nm + ".png")), 21)):
            a += b
    st = SL.ConfStats.load(str(tmp_path / "conf" / "stats.npz"))
    for a, b in zip(st.tables(), ref):
        assert np.array_equal(a, b)
    hist = ref[0]
    assert 100 * SL.quality_curve(*ref, [1.0])["coverage_all"][0] == pytest.approx(float(lines[-1].split()[1].rstrip("%")), abs=6e-4)
    sel = ["select", "--seg_dir", str(tmp_path / "seg"), "--conf_dir", str(tmp_path / "conf")]
    # --portion 1.0 reproduces the --out_seg maps (there are no NaN pixels here)
    assert SL.main(sel + ["--out_dir", str(tmp_path / "self10"), "--portion", "1.0"]) == 0
    capsys.readouterr()
    for nm in NAMES:
        assert np.array_equal(_png(tmp_path / "self10" / f"{nm}.png"), probs[nm][0])
    # --portion 0.3: per class at least ceil(0.3 n_c) pixels, and only whole codes
    assert SL.main(sel + ["--out_dir", str(tmp_path / "self03"), "--portion", "0.3", "--gt_dir", gt_dir]) == 0
    out = capsys.readouterr().out
    assert "precision" in out and "kept" in out
    tc = R.thresholds(hist, 0.3)
    kept = np.zeros(21, np.int64)
    for nm in NAMES:
        got = _png(tmp_path / "self03" / f"{nm}.png")
        pred, code = probs[nm][0], _png(tmp_path / "conf" / f"{nm}.png")
        assert np.array_equal(got, R.select(pred, code, tc)[0])        # whole codes: every pixel within the threshold, none beyond
        kept += np.bincount(got[got != 255], minlength=21)
    n_c = hist.sum(1)
    assert n_c.sum() == len(NAMES) * H0 * W0 and np.all(kept >= np.ceil(0.3 * n_c)) and np.all(kept[n_c == 0] == 0)
    assert [math.ceil(0.3 * int(n)) <= k <= n for n, k in zip(n_c, kept)] == [True] * 21
    # without a stats file the histograms are counted from the files: the same thresholds, the same maps
    os.rename(tmp_path / "conf" / "stats.npz", tmp_path / "stats_moved.npz")
    assert SL.main(sel + ["--out_dir", str(tmp_path / "self03b"), "--portion", "0.3", "--list", str(tree["tmp"] / "val.txt")]) == 0
    assert SL.main(sel + ["--out_dir", str(tmp_path / "self03c"), "--portion", "0.3", "--stats", str(tmp_path / "stats_moved.npz")]) == 0
    capsys.readouterr()
    for nm in NAMES:
        a = (tmp_path / "self03" / f"{nm}.png").read_bytes()
        assert (tmp_path / "self03b" / f"{nm}.png").read_bytes() == a and (tmp_path / "self03c" / f"{nm}.png").read_bytes() == a
