"""Input path of decoder training (muscle_amd.segdata: VOC12SegDataset / plan_seg_item / SegStager / SegLoader), the per-epoch
validation (muscle_amd.evaluation.SegValidation) and `python -m muscle_amd.train_muscle`, against tests/segdata_ref.py - the
numpy / scipy / PIL restatement of src/data.py:93-123.

Bounds of the GPU mask test: every output is a convex combination of source values formed in at most ~64 fp32 rounding
steps of 2^-24 relative each (6 x 6 taps at scale 0.5, products and sums, plus the rounding of the two weight rows), whichever
order the kernel sums in: |out - ref| <= 4e-6 * max|mask|.  The arg-max test excludes pixels whose top-two gap in the
restatement is below twice that."""
import os
import random
import re
import subprocess
import sys
import zlib

import numpy as np
import pytest
import torch

import segdata_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HERE = os.path.dirname(os.path.abspath(__file__))
SCALES = (0.5, 0.77, 1.0, 1.31, 1.75)


def _seed(s=11):
    random.seed(s)
    torch.manual_seed(s)


# ---- CPU --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("augment", [True, False])
def test_planner_follows_the_reference_draw_order(augment):
    from muscle_amd import segdata as D
    img, mask = R.synth_image(75, 100, 1), R.synth_label(75, 100, 1)
    for seed in range(6):
        for crop in (64, 160):                                        # window smaller / larger than the rescaled image
            _seed(seed)
            p = D.plan_seg_item(img, mask, 0.5, 1.75, crop, augment=augment)
            after = (random.random(), float(torch.rand(1)))
            _seed(seed)
            d = R.ref_draws(100, 75, 0.5, 1.75, crop, augment)
            assert (random.random(), float(torch.rand(1))) == after   # both generators consumed identically
            assert R.plan_as_draws(p) == d
            assert p.resize_to == (round(100 * p.scale), round(75 * p.scale))
    assert round(2.5) == 2 and round(3.5) == 4                        # Python's round: half to even, as in the reference


@pytest.mark.parametrize("size", [(375, 500), (41, 67)])
def test_axis_tables_equal_the_scipy_composition(size):
    from muscle_amd.segdata import mask_axis_table
    H, W = size
    m = np.random.default_rng(3).uniform(0, 1, (H, W, 4))
    for s in SCALES:
        oh, ow = round(H * s), round(W * s)
        ty, tx = mask_axis_table(H, oh), mask_axis_table(W, ow)
        for (st, w), n_in in ((ty, H), (tx, W)):
            assert st.min() >= 0 and (st + w.shape[1]).max() <= n_in and np.all(np.diff(st) >= 0)
            assert np.abs(w.sum(1) - 1).max() <= 1e-14 and w.min() >= 0
            assert w.shape[1] == (6 if s == 0.5 else 4 if s == 0.77 else 2)
        err = np.abs(R.apply_tables(m, ty, tx) - R.skresize_ref(m, oh, ow)).max()
        print(f"size {size} scale {s}: tables vs scipy {err:.2e}")
        assert err <= 1e-12
        if s == 1.0:
            assert np.array_equal(R.apply_tables(m, ty, tx), m)
            assert np.array_equal(ty[0], np.minimum(np.arange(H), H - 2)) and set(np.unique(ty[1])) == {0.0, 1.0}
        lo, cnt = oh // 3, oh // 2                                     # a window of rows is the same rows of the whole table
        st, w = mask_axis_table(H, oh, lo, cnt)
        assert np.array_equal(st, ty[0][lo:lo + cnt]) and np.array_equal(w, ty[1][lo:lo + cnt])


def _plan_mask_cpu(p, crop):
    """What mx_mask_stage computes from a plan, in numpy (fp32 weights, fp64 sums)."""
    (sy, wy), (sx, wx) = p.mask_y, p.mask_x
    win = R.apply_tables(p.mask_src.astype(np.float64), (sy, wy.astype(np.float64)), (sx, wx.astype(np.float64)))
    out = np.zeros((crop, crop, win.shape[-1]))
    out[p.place[0]:p.place[0] + win.shape[0], p.place[1]:p.place[1] + win.shape[1]] = win
    return (np.fliplr(out) if p.flip else out).transpose(2, 0, 1)


def _voc_tree(tmp_path, dtypes=(np.float16, np.float32, np.float64, np.float16), sizes=((75, 100), (96, 72), (80, 120), (64, 64))):
    """A tiny VOC-style tree: JPEGImages/*.jpg, soft labels <name>.npy [H,W,21], SegmentationClass/*.png, lists, labels."""
    import PIL.Image
    root, mroot = tmp_path / "VOC2012", tmp_path / "soft"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    mroot.mkdir()
    names = [f"2007_{i:06d}" for i in range(len(sizes))]
    g = np.random.default_rng(5)
    for i, (nm, (h, w)) in enumerate(zip(names, sizes)):
        R.synth_image(h, w, i).save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        np.save(mroot / f"{nm}.npy", R.synth_label(h, w, i).astype(dtypes[i % len(dtypes)]))
        PIL.Image.fromarray(g.choice([0, 1, 4, 255], size=(h, w)).astype(np.uint8), "L").save(root / "SegmentationClass" / f"{nm}.png")
    lst = tmp_path / "train_aug.txt"
    lst.write_text("".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png\n" for n in names))
    labels = {n: np.eye(20, dtype=np.float32)[i % 20] for i, n in enumerate(names)}
    return str(lst), str(root), str(mroot), labels, names


def test_dataset_and_loader_on_a_tree(tmp_path):
    import PIL.Image
    from muscle_amd import segdata as D
    lst, root, mroot, labels, names = _voc_tree(tmp_path)
    with pytest.raises(NotImplementedError, match="soft"):
        D.VOC12SegDataset(lst, root, mroot, mask_type="hard", labels=labels)
    ds = D.VOC12SegDataset(lst, root, mroot, min_scale=0.5, max_scale=1.75, crop_size=96, labels=labels)
    assert len(ds) == 4 and ds.names == names
    _seed(4)
    for i, nm in enumerate(names):
        name, p, lab = ds[i]
        src = np.load(os.path.join(mroot, nm + ".npy"))
        assert name == nm and np.array_equal(lab, labels[nm])
        assert p.mask_src.dtype == (np.float16 if src.dtype == np.float16 else np.float32)      # float64 files: shipped as fp32
        assert p.mask_src.shape[0] <= src.shape[0] and p.mask_src.shape[1:] == src.shape[1:]
        assert p.img_u8.shape == src.shape[:2] + (3,)
        # the plan's tables on the shipped rows are the restatement's crop of the resized label
        ref = R.ref_mask(src, R.plan_as_draws(p), 96)
        assert np.abs(_plan_mask_cpu(p, 96) - ref).max() <= 1e-6
    # the loader: sequential plan calls on the caller's generators without workers; workers hand the plans back intact
    loader = D.SegLoader(ds, batch_size=2, device=torch.device("cpu"), num_workers=0, shuffle=False)
    assert len(loader) == 2
    _seed(4)
    torch.empty((), dtype=torch.int64).random_()       # the base seed a DataLoader iterator draws first
    direct = [ds.plan(i) for i in range(4)]
    _seed(4)
    seq = [it for batch in loader.loader for it in batch]
    for (n0, p0, l0), (n1, p1, l1) in zip(direct, seq):
        assert n0 == n1 and R.plan_as_draws(p0) == R.plan_as_draws(p1) and np.array_equal(p0.mask_src, p1.mask_src)
    got = []
    for batch in D.SegLoader(ds, batch_size=2, device=torch.device("cpu"), num_workers=2, shuffle=False).loader:
        for name, p, lab in batch:
            assert p.img_u8.dtype == np.uint8 and p.mask_y[1].dtype == np.float32 and lab.shape == (20,)
            got.append(name)
    assert got == names


def test_script_parses_the_reference_arguments():
    from muscle_amd import train_muscle
    a = train_muscle.parse_args(["--batch_size", "16", "--max_epoches", "8", "--lr", "1e-5", "--num_workers", "8", "--wt_dec", "1e-5",
                                 "--train_list", "t.txt", "--num_classes", "21", "--session_name", "runs/x", "--crop_size", "448",
                                 "--weights", "w.pth", "--voc12_root", "V", "--mask_root", "M", "--k", "128", "--step", "7",
                                 "--lamb", "0.05", "--tblog_dir", "tb", "--cls_dir", "C", "--crf", "1", "--seed", "221",
                                 "--pretrained", "b7", "--bifpn", "3"])
    assert a.batch_size == 16 and a.mask_root == "M" and a.crf == 1 and a.val_list == "data/val.txt" and a.lamb == 0.05
    d = train_muscle.parse_args(["--mask_root", "M"])
    assert (d.batch_size, d.max_epoches, d.lr, d.num_workers, d.wt_dec, d.k, d.step, d.lamb, d.crf, d.seed, d.pretrained, d.bifpn) == \
        (6, 8, 1e-5, 8, 1e-5, 128, 7, 5e-2, 0, 221, "b7", 3)


# ---- GPU --------------------------------------------------------------------------------------------------------------
DEV = "cuda:0"


def _plans(cases, crop, augment=True, seed=7, dtype=np.float16):
    """cases: (H, W, scale, flip) -> (images, masks, plans) with the scale and the flip bit forced."""
    from muscle_amd import segdata as D
    ims, masks, plans = [], [], []
    _seed(seed)
    for i, (H, W, s, flip) in enumerate(cases):
        ims.append(R.synth_image(H, W, 10 + i))
        masks.append(R.synth_label(H, W, 20 + i).astype(dtype))
        p = D.plan_seg_item(ims[-1], masks[-1], s, s, crop, augment=augment)      # random.uniform(s, s) == s
        assert p.scale == s
        p.flip = bool(flip)
        plans.append(p)
    return ims, masks, plans


MASK_CASES = [(375, 500, 0.5, 0), (375, 500, 1.0, 1), (333, 500, 1.75, 0), (500, 375, 0.77, 1), (120, 90, 1.31, 1)]


@pytest.mark.gpu
def test_mask_stage_vs_fp64_restatement():
    from muscle_amd import segdata as D
    S = 448
    ims, masks, plans = _plans(MASK_CASES, S)
    stager = D.SegStager(torch.device(DEV), len(plans), S)
    out = stager(plans)["mask"]
    torch.cuda.synchronize()
    assert out.shape == (len(plans), 21, S, S) and out.dtype == torch.float32
    got = out.cpu().numpy()
    small = 0
    for i, (p, m) in enumerate(zip(plans, masks)):
        d = R.plan_as_draws(p)
        ref = R.ref_mask(m, d, S)
        err, bound = np.abs(got[i] - ref).max(), 4e-6 * float(np.abs(m.astype(np.float64)).max())
        print(f"item {i} {MASK_CASES[i]}: |out - ref| {err:.3e} (bound {bound:.3e})")
        assert err <= bound
        win = R.window(d, S)
        small += int(not win.all())
        assert np.all(got[i][:, ~win] == 0.0)                          # exactly zero outside the placed window
    assert small >= 2                                                  # cases with a zero border were among them
    for p in plans:
        p.flip = not p.flip
    flipped = stager(plans)["mask"]
    assert torch.equal(flipped, torch.flip(out, dims=[3]))             # flip on == flip off reversed along X, bit for bit
    # float32 sources holding the same values give the same bits; the rows shipped are a slice of the file
    _, _, plans32 = _plans(MASK_CASES, S, dtype=np.float32)
    for p, q in zip(plans, plans32):
        q.flip = p.flip
        assert q.mask_src.dtype == np.float32
    assert torch.equal(stager(plans32)["mask"], flipped)
    assert plans[2].mask_src.shape[0] < 333 and plans[0].mask_src.shape[0] == 375


@pytest.mark.gpu
def test_mask_stage_argmax_agreement():
    """argmax_c (what the cross entropy consumes) equals the restatement's wherever its top-two gap is >= 8e-6; the excluded
    share stays <= 1e-3.  Counted over the placed window (outside it every channel is exactly 0)."""
    from muscle_amd import segdata as D
    S = 448
    cases = [(375, 500, s, i % 2) for i, s in enumerate(SCALES)]
    _, masks, plans = _plans(cases, S, seed=9)
    got = D.SegStager(torch.device(DEV), len(plans), S)(plans)["mask"].cpu().numpy()
    for i, (p, m) in enumerate(zip(plans, masks)):
        d = R.plan_as_draws(p)
        ref = R.ref_mask(m, d, S)
        win = R.window(d, S)
        srt = np.sort(ref, axis=0)
        sure = (srt[-1] - srt[-2]) >= 8e-6
        excluded = float((~sure & win).sum()) / float(win.sum())
        bad = int(((got[i].argmax(0) != ref.argmax(0)) & sure & win).sum())
        print(f"scale {cases[i][2]}: excluded share {excluded:.2e}, disagreeing pixels {bad}")
        assert excluded <= 1e-3
        assert bad == 0


IMG_CASES = [(375, 500, 0.5, 1), (375, 500, 1.0, 0), (333, 500, 1.75, 1), (90, 120, 1.31, 0)]


@pytest.mark.gpu
@pytest.mark.parametrize("augment", [True, False])
def test_image_path_bit_exact_with_pil(augment):
    from muscle_amd import segdata as D
    S = 448
    ims, _, plans = _plans(IMG_CASES, S, augment=augment, seed=13)
    assert all((p.jitter is not None) == augment for p in plans)
    out = D.SegStager(torch.device(DEV), len(plans), S)(plans)["img"].cpu().numpy()
    for i, (im, p) in enumerate(zip(ims, plans)):
        ref = R.ref_image(im, R.plan_as_draws(p), S)
        assert ref.dtype == np.float32 and np.array_equal(out[i], ref), (i, np.abs(out[i] - ref).max())


@pytest.mark.gpu
def test_staged_batch_feeds_muscle_step_and_repeats_bit_for_bit():
    import muscle_amd
    from muscle_amd import segdata as D
    S = 96
    cases = [(75, 100, 0.6, 0), (96, 72, 1.0, 1), (80, 120, 1.6, 0), (64, 64, 1.2, 1)]
    _, _, plans = _plans(cases, S, seed=17)
    labels = torch.zeros(4, 20)
    labels[:, 3] = 1; labels[1, 7] = 1
    dev = torch.device(DEV)
    a = D.SegStager(dev, 4, S)(plans, labels=labels)
    b = D.SegStager(dev, 4, S)(plans, labels=labels)
    assert set(a) == {"img", "mask", "label"} and a["img"].shape == (4, 3, S, S) and a["mask"].shape == (4, 21, S, S)
    for k in a:
        assert torch.equal(a[k], b[k]), k
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(dev)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-5, weight_decay=1e-5)
    out = muscle_amd.muscle_step(model, opt, a, lamb=0.05, step=7, k=32)
    for k, v in out.items():
        assert np.isfinite(float(v)), k


def _crc(t):
    return zlib.crc32(t.detach().cpu().contiguous().numpy().tobytes())


def loader_digest(tmp, workers):
    """(names, CRC-32 of img / mask / label) per batch of one epoch; run by the child process of the next test.
    workers > 0: SegLoader with that many worker processes.  workers == 0: the same plans made inline, each worker's share
    of the batches on the seeds torch's DataLoader gives that worker (base seed + worker id for torch and random)."""
    import pathlib
    from muscle_amd import segdata as D
    lst, root, mroot, labels, names = _voc_tree(pathlib.Path(tmp), sizes=((75, 100), (96, 72), (80, 120), (64, 64), (70, 90), (88, 66)))
    ds = D.VOC12SegDataset(lst, root, mroot, 0.5, 1.75, crop_size=96, labels=labels)
    dev, W = torch.device(DEV), 2
    gen = torch.Generator().manual_seed(3)
    if workers:
        loader = D.SegLoader(ds, 2, dev, num_workers=W, shuffle=False, generator=gen)
        return [(nm, [_crc(b[k]) for k in ("img", "mask", "label")]) for nm, b in loader]
    base = int(torch.empty((), dtype=torch.int64).random_(generator=gen).item())
    stager, out = D.SegStager(dev, 2, 96), {}
    for w in range(W):
        random.seed(base + w)
        torch.manual_seed(base + w)
        for bi in range(w, len(ds) // 2, W):
            items = [ds.plan(i) for i in (2 * bi, 2 * bi + 1)]
            b = stager([it[1] for it in items], labels=torch.from_numpy(np.stack([it[2] for it in items])))
            out[bi] = ([it[0] for it in items], [_crc(b[k]) for k in ("img", "mask", "label")])
    return [out[bi] for bi in sorted(out)]


@pytest.mark.gpu
def test_loader_with_workers_in_a_fresh_process(tmp_path):
    """SegLoader(num_workers=2) the way the training script runs it - a fresh process creates the stager, the DataLoader forks
    its workers at the first iteration - yields the batches the inline path yields for the same seeds."""
    code = ("import sys, torch; sys.path.insert(0, %r); sys.path.insert(0, %r); torch.set_num_threads(2)\n"
            "import test_seg_input_path as t\n"
            "a = t.loader_digest(sys.argv[1] + '/a', 2); b = t.loader_digest(sys.argv[1] + '/b', 0)\n"
            "assert len(a) == 3 and a == b, (a, b)\n"
            "print('LOADER-OK')\n") % (HERE, ROOT)
    (tmp_path / "a").mkdir(); (tmp_path / "b").mkdir()
    r = subprocess.run([sys.executable, "-c", code, str(tmp_path)], capture_output=True, text=True, timeout=150)
    assert r.returncode == 0 and "LOADER-OK" in r.stdout, (r.stdout[-1000:], r.stderr[-3000:])


def _hand_counts(pred, gt, K=21):
    cal = gt < 255
    hit = (pred == gt) * cal
    return np.array([[np.sum((gt == i) * hit), np.sum((pred == i) * cal), np.sum((gt == i) * cal)] for i in range(K)], np.int64)


@pytest.mark.gpu
@pytest.mark.parametrize("with_cls", [False, True])
def test_validation_counts_equal_a_hand_count(tmp_path, with_cls):
    """SegValidation against train_muscle.py:269-280 counted by hand on the arg-max of infer_seg's mean map."""
    import PIL.Image
    import muscle_amd
    from muscle_amd.data import MSFStager
    from muscle_amd.evaluation import SegValidation, validate_seg
    from muscle_amd.infer import infer_seg
    lst, root, _, _, names = _voc_tree(tmp_path, sizes=((72, 96), (80, 72)))
    dev = torch.device(DEV)
    torch.manual_seed(1)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(dev).eval()
    cls_dir = None
    if with_cls:
        cls_dir = tmp_path / "cls"
        cls_dir.mkdir()
        for i, nm in enumerate(names):
            np.save(cls_dir / f"{nm}.npy", np.linspace(0.2, 1.0, 21, dtype=np.float32)[None] ** (i + 1))
    val = SegValidation(dev, 21, cls_dir=None if cls_dir is None else str(cls_dir))
    want, stager = np.zeros((21, 3), np.int64), MSFStager(dev)
    for nm in names:
        img = PIL.Image.open(os.path.join(root, "JPEGImages", nm + ".jpg")).convert("RGB")
        gt = np.array(PIL.Image.open(os.path.join(root, "SegmentationClass", nm + ".png")))
        pred = val.add(model, img, gt, nm)
        cls = None if cls_dir is None else np.load(cls_dir / f"{nm}.npy").squeeze()
        _, prob = infer_seg(model, stager(img, (1,))[:1], gt.shape[0], gt.shape[1], cls_label=cls, return_prob=True)
        hand = prob.cpu().numpy().argmax(0)
        assert np.array_equal(pred.cpu().numpy(), hand)
        want += _hand_counts(hand, gt)
    assert np.array_equal(val.table.counts.cpu().numpy(), want)
    iou = [want[i, 0] / (want[i, 2] + want[i, 1] - want[i, 0] + 1e-10) for i in range(21)]
    assert val.miou() == pytest.approx(float(np.mean(np.array(iou))), rel=1e-12, abs=1e-15)
    assert validate_seg(model, names, root, dev, 21, cls_dir=None if cls_dir is None else str(cls_dir)) == val.miou()


@pytest.mark.gpu
def test_train_script_smoke(tmp_path):
    """python -m muscle_amd.train_muscle in a fresh process: B0, four synthetic items, one epoch, batch 2."""
    import muscle_amd
    lst, root, mroot, labels, names = _voc_tree(tmp_path)
    (tmp_path / "data").mkdir()
    np.save(tmp_path / "data" / "cls_labels.npy", labels)
    (tmp_path / "val.txt").write_text("".join(f"/JPEGImages/{n}.jpg\n" for n in names[:2]))
    ses = tmp_path / "runs"
    r = subprocess.run([sys.executable, "-m", "muscle_amd.train_muscle", "--batch_size", "2", "--max_epoches", "1", "--num_workers", "0",
                        "--train_list", lst, "--val_list", str(tmp_path / "val.txt"), "--voc12_root", root, "--mask_root", mroot,
                        "--session_name", str(ses), "--tblog_dir", str(tmp_path / "tb"), "--crop_size", "96", "--k", "32",
                        "--pretrained", "b0", "--bifpn", "3", "--seed", "221"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=280)
    assert r.returncode == 0, r.stderr[-3000:]
    assert re.search(r"Iter:\s+0/\s+2 loss_seg:\d+\.\d{4} loss_beacon:-?\d+\.\d{4} imps:\d+\.\d Fin:", r.stdout), r.stdout[-2000:]
    m = re.search(r"Epoch:0 val miou:([0-9.e+-]+)", r.stdout)
    assert m and 0.0 <= float(m.group(1)) <= 1.0, r.stdout[-2000:]
    assert (tmp_path / "tb").is_dir()
    sd = torch.load(ses / "_0.pth", map_location="cpu")
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec")
    model.load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
