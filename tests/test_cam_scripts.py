"""The CAM stage as scripts: `python -m muscle_amd.train_mcl`, `python -m muscle_amd.infer_mcl`, `python -m muscle_amd.evaluation`.

CPU: argument lists and defaults of the reference (train_mcl.py:72-86, infer_mcl.py:64-74, src/evaluation.py:107-117, and the
command lines of its README), the header's two new entry points, import hygiene, the writer thread.
GPU: each script in a fresh process on a synthetic VOC tree, B0.  A fresh process runs the library's default GEMM arithmetic
(mode 1, the split); where a test repeats a script's forward in its own process it switches to that mode first, so the
comparison is exact whichever arithmetic the suite is run with."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
DEV = "cuda:0"
LOSSES = ("loss_focal", "loss_softmargin", "loss_pair", "loss_er", "loss_imc", "loss_pixc", "loss_emd")


# ---- CPU --------------------------------------------------------------------------------------------------------------
def test_train_mcl_arguments():
    from muscle_amd import train_mcl
    a = train_mcl.parse_args([])
    assert (a.batch_size, a.max_epoches, a.lr, a.num_workers, a.wt_dec) == (16, 16, 1e-4, 8, 5e-5)
    assert (a.train_list, a.num_classes, a.session_name, a.crop_size) == ("data/train_aug.txt", 21, "runs/EffSeg_mcl", 448)
    assert (a.weights, a.voc12_root, a.tblog_dir, a.seed) == (None, "data/VOC2012", "logs/tblog_mcl", 0)
    assert (a.pretrained, a.eval_list, a.start_epoch) == ("b3", "data/train.txt", 0)
    # the README's command line
    a = train_mcl.parse_args("--voc12_root data --train_list data/train_aug.txt --weights W.pth --tblog_dir logs/tblog_mcl".split())
    assert (a.voc12_root, a.weights) == ("data", "W.pth")
    a = train_mcl.parse_args("--batch_size 4 --max_epoches 13 --lr 2e-4 --num_workers 2 --wt_dec 1e-5 --num_classes 21 --session_name s "
                             "--crop_size 320 --seed 7 --start_epoch 12 --pretrained b0 --eval_list e.txt".split())
    assert (a.batch_size, a.max_epoches, a.start_epoch, a.pretrained, a.eval_list, a.seed) == (4, 13, 12, "b0", "e.txt", 7)
    with pytest.raises(SystemExit):
        train_mcl.parse_args(["--start_epoch", "17"])
    r = subprocess.run([sys.executable, "-m", "muscle_amd.train_mcl", "--help"], env=dict(os.environ, PYTHONPATH=ROOT),
                       capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "--start_epoch" in r.stdout and "moments restart" in " ".join(r.stdout.split())


def test_infer_mcl_arguments():
    from muscle_amd import infer_mcl
    a = infer_mcl.parse_args(["--weights", "w.pth"])
    assert (a.infer_list, a.num_workers, a.num_classes, a.tblog) == ("../data/VOC2012/train.txt", 8, 21, None)
    assert (a.voc12_root, a.out_npy, a.out_cam_npy, a.pretrained) == ("data/VOC2012", None, None, "b3")
    a = infer_mcl.parse_args("--voc12_root V --infer_list L.txt --weights W.ckpt --out_npy OUT".split())       # the README's
    assert (a.voc12_root, a.infer_list, a.weights, a.out_npy) == ("V", "L.txt", "W.ckpt", "OUT")
    a = infer_mcl.parse_args("--weights w --tblog tb --num_workers 0 --out_cam_npy C --pretrained b0".split())
    assert (a.tblog, a.out_cam_npy, a.pretrained) == ("tb", "C", "b0")
    assert infer_mcl.DEFAULT_SCALES == (0.5, 1, 1.5, 2)


def test_evaluation_arguments():
    from muscle_amd import evaluation as E
    a = E.parse_args("--comment C --type npy --list data/train.txt --predict_dir CAM_DIR --curve True".split())       # README
    assert a.curve is True and a.type == "npy" and a.t is None and (a.list, a.predict_dir) == ("data/train.txt", "CAM_DIR")
    a = E.parse_args("--comment C --type png --list data/train.txt --predict_dir D".split())                       # README
    assert a.curve is False and a.type == "png"
    for v in ("true", "1"):
        assert E.parse_args(["--comment", "c", "--curve", v]).curve is True
    for v in ("False", "false", "0"):                     # the reference's type=bool would read these as True
        assert E.parse_args(["--comment", "c", "--curve", v, "--t", "0.3"]).curve is False
    a = E.parse_args(["--comment", "c", "--t", "0.25", "--gt_dir", "G", "--logfile", "L"])
    assert (a.t, a.gt_dir, a.logfile, a.type) == (0.25, "G", "L", "npy")
    for bad in (["--comment", "c"], ["--comment", "c", "--curve", "False"], ["--type", "npy", "--t", "0.3"],
                ["--comment", "c", "--curve", "maybe"], ["--comment", "c", "--t", "-0.1"], ["--comment", "c", "--type", "jpg"]):
        with pytest.raises(SystemExit):
            E.parse_args(bad)


def test_header_declares_the_entry_points():
    from muscle_amd._lib import HEADER_PATH, parse_header
    sigs = parse_header()
    assert sigs["mx_cam_infer"] == "piiiiipippp"
    assert sigs["mx_camdict_confusion"] == "ppippiiiipp"
    text = open(HEADER_PATH).read()
    assert "infer_mcl.py:107-148" in text and "src/evaluation.py:25-50" in text         # declared with their reference lines


def test_modules_import_without_side_effects():
    code = ("import sys, muscle_amd.train_mcl, muscle_amd.infer_mcl, muscle_amd.evaluation, torch\n"
            "bad = [m for m in ('cv2', 'pandas', 'tensorboardX') if m in sys.modules]\n"
            "assert not bad, bad\n"
            "assert not torch.cuda.is_initialized()\n"
            "import muscle_amd._lib as L\n"
            "assert L._lib is None\n"
            "print('IMPORT-OK')\n")
    r = subprocess.run([sys.executable, "-c", code], env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "IMPORT-OK" in r.stdout, r.stderr[-2000:]
    for mod in ("train_mcl", "infer_mcl"):
        src = open(os.path.join(ROOT, "muscle_amd", mod + ".py")).read()
        top = [ln for ln in src.splitlines() if ln.startswith(("import ", "from "))]
        assert not any(re.search(r"\b(torch|pandas|cv2|tensorboardX|tqdm)\b", ln) for ln in top), top


def test_npy_writer_drains_and_reraises(tmp_path):
    from muscle_amd.infer_mcl import NpyWriter
    w = NpyWriter(depth=2)
    for i in range(7):
        w.put(str(tmp_path / f"a{i}.npy"), {i: np.full((3, 4), i, np.float32)})
    w.close()
    for i in range(7):
        d = np.load(tmp_path / f"a{i}.npy", allow_pickle=True).item()
        assert list(d) == [i] and np.array_equal(d[i], np.full((3, 4), i, np.float32))
    w = NpyWriter(depth=2)
    w.put(str(tmp_path / "no_such_dir" / "x.npy"), {0: np.zeros(2)})
    with pytest.raises(OSError):
        w.close()
    w.close()                                             # a second close is a no-op


def test_writelog_block(tmp_path):
    from muscle_amd.evaluation import writelog
    p = tmp_path / "log.txt"
    writelog(str(p), {"a": 1.5, "mIoU": 2}, "first")
    writelog(str(p), {"mIoU": [1.0, 2.0]}, "second")
    lines = p.read_text().splitlines()
    assert re.fullmatch(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\tfirst", lines[0]) and lines[1] == "a:1.5  mIoU:2  "
    assert lines[2] == "=====================================" and lines[3].endswith("\tsecond")
    assert lines[4] == "mIoU:[1.0, 2.0]  " and len(lines) == 6


# ---- GPU: the scripts, each in a fresh process --------------------------------------------------------------------------
def _synth_image(h, w, seed):
    import PIL.Image
    g = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    img = np.stack([127 + 100 * np.sin(xx / (5.0 + c) + seed) * np.cos(yy / (7.0 - c)) for c in range(3)], -1)
    img += g.normal(0, 12, img.shape)
    return PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB")


def _voc_tree(tmp_path, sizes=((75, 100), (100, 75), (80, 104), (72, 96))):
    """JPEGImages/*.jpg, SegmentationClass/*.png, the list and data/cls_labels.npy under tmp_path (the scripts' cwd)."""
    import PIL.Image
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    (tmp_path / "data").mkdir()
    names = [f"2007_{i:06d}" for i in range(len(sizes))]
    g = np.random.default_rng(5)
    labels = {}
    for i, (nm, (h, w)) in enumerate(zip(names, sizes)):
        _synth_image(h, w, i).save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        cls = [3 * i + 1, 3 * i + 2][:1 + i % 2]
        lab = np.zeros(20, np.float32)
        lab[cls] = 1
        labels[nm] = lab
        gt = g.choice([0, cls[0] + 1, cls[-1] + 1, 255], size=(h // 4 + 1, w // 4 + 1), p=[0.5, 0.25, 0.2, 0.05]).astype(np.uint8)
        gt = np.kron(gt, np.ones((4, 4), np.uint8))[:h, :w]
        PIL.Image.fromarray(np.ascontiguousarray(gt), "L").save(root / "SegmentationClass" / f"{nm}.png")
    np.save(tmp_path / "data" / "cls_labels.npy", labels)
    lst = tmp_path / "train.txt"
    lst.write_text("".join(f"/JPEGImages/{n}.jpg /SegmentationClass/{n}.png\n" for n in names))
    return str(lst), str(root), labels, names


def _run(tmp_path, module, *args, timeout=280):
    r = subprocess.run([sys.executable, "-m", "muscle_amd." + module, *args], cwd=str(tmp_path),
                       env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=timeout)
    assert r.returncode == 0, (r.stdout[-1500:], r.stderr[-3000:])
    return r.stdout


def _script_arithmetic():
    import muscle_amd
    muscle_amd.set_gemm_mode(1)            # what a fresh process runs (the autouse fixture restores the suite's mode)


def _iter_losses(stdout):
    m = re.search(r"Iter:\s*(\d+)/\s*(\d+) " + " ".join(k + r":(\S+)" for k in LOSSES) + r" imps:\d+\.\d Fin:.* lr: (\d\.\d{7})", stdout)
    assert m, stdout[-2000:]
    vals = [float(v) for v in m.groups()[2:9]]
    assert all(np.isfinite(vals)), vals
    return int(m.group(1)), int(m.group(2)), dict(zip(LOSSES, vals))


def _train_args(lst, root, ses, tmp_path, *extra):
    return ["--batch_size", "2", "--num_workers", "0", "--train_list", lst, "--eval_list", lst, "--voc12_root", root,
            "--session_name", str(ses), "--tblog_dir", str(tmp_path / "tb"), "--crop_size", "128", "--pretrained", "b0",
            "--seed", "7", *extra]


@pytest.mark.gpu
def test_train_mcl_script(tmp_path):
    """One epoch of B0 on four synthetic items: the checkpoint, the Iter line, the rapid-evaluation line, and run-to-run bits."""
    import PIL.Image
    import muscle_amd
    from muscle_amd.data import MSFStager
    from muscle_amd.evaluation import RapidEval
    lst, root, labels, names = _voc_tree(tmp_path)
    out = _run(tmp_path, "train_mcl", *_train_args(lst, root, tmp_path / "runs", tmp_path, "--max_epoches", "1"))
    it, max_step, losses = _iter_losses(out)
    assert (it, max_step) == (0, 2) and losses["loss_pixc"] == 0 and losses["loss_emd"] == 0 and losses["loss_focal"] > 0
    assert (tmp_path / "tb").is_dir() and not (tmp_path / "training_eval").exists()
    sd = torch.load(tmp_path / "runs" / "_0.pth", map_location="cpu")
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=False)
    model.load_state_dict(sd, strict=True)
    assert all(torch.isfinite(v).all() for v in sd.values() if v.is_floating_point())
    m = re.search(r"Epoch:0 max miou:(\S+) max t:(\S+) Time elapse:", out)
    assert m, out[-2000:]
    # the same evaluation driven by hand over the same list with _0.pth loaded
    _script_arithmetic()
    dev = torch.device(DEV)
    model = model.to(dev).eval()
    ev, stager = RapidEval(dev), MSFStager(dev)
    for nm in names:
        img = PIL.Image.open(os.path.join(root, "JPEGImages", nm + ".jpg")).convert("RGB")
        gt = np.array(PIL.Image.open(os.path.join(root, "SegmentationClass", nm + ".png")))
        ev.add(model, stager(img, (1,))[0], torch.from_numpy(labels[nm]).view(1, -1), torch.from_numpy(gt).to(dev))
    max_miou, max_t, _ = ev.best()
    print("script:", m.group(1), m.group(2), "by hand:", max_miou, max_t)
    assert float(m.group(1)) == float(max_miou) and float(m.group(2)) == float(max_t)
    # a second identical run: the step is bit-reproducible, so the checkpoint is tensor for tensor the same
    _run(tmp_path, "train_mcl", *_train_args(lst, root, tmp_path / "runs2", tmp_path, "--max_epoches", "1"))
    sd2 = torch.load(tmp_path / "runs2" / "_0.pth", map_location="cpu")
    assert list(sd2) == list(sd)
    diff = [k for k in sd if not torch.equal(sd[k], sd2[k])]
    assert not diff, (len(diff), diff[:8])


@pytest.mark.gpu
def test_train_mcl_start_epoch(tmp_path):
    """--weights W --max_epoches 13 --start_epoch 12 (a continued run): exactly one epoch, behind the PixPro and EMD gates.
    The weights are the seeded synthetic ones of the parity tests with the CAM classifier (fc.weight) scaled by 10, so that
    the class maps are peaked as a trained network's are.  The line prints four decimals (the reference's format), and an
    untrained network's softmax-normalised maps are nearly uniform over the classes: measured on this tree, loss_emd is
    1.7e-5 with the synthetic weights as they are (it prints as 0.0000, -0.0000 with default initialisation) and 5.4e-3
    with the scaled classifier."""
    from muscle_amd import synth
    from muscle_amd.arch import net_cfg
    lst, root, _, _ = _voc_tree(tmp_path)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(net_cfg("efficientnet-b0", False), 31).items()}
    sd["fc.weight"] = sd["fc.weight"] * 10.0
    torch.save(sd, tmp_path / "w.pth")
    out = _run(tmp_path, "train_mcl", *_train_args(lst, root, tmp_path / "runs", tmp_path, "--max_epoches", "13", "--start_epoch", "12",
                                                   "--weights", str(tmp_path / "w.pth")))
    print(re.search(r"Iter:.*", out).group(0))
    it, max_step, losses = _iter_losses(out)
    assert (it, max_step) == (24, 26)
    assert losses["loss_pixc"] != 0 and losses["loss_emd"] != 0
    assert sorted(os.listdir(tmp_path / "runs")) == ["_12.pth"]
    assert len(re.findall(r"Epoch:\d+ max miou:", out)) == 1 and "Epoch:12 max miou:" in out


@pytest.mark.gpu
def test_infer_mcl_and_evaluation_scripts(tmp_path):
    import PIL.Image
    import muscle_amd
    from muscle_amd import infer, synth
    from muscle_amd.arch import net_cfg
    from muscle_amd.data import MSFStager
    from muscle_amd.evaluation import CamDictEval, SegEval, categories
    lst, root, labels, names = _voc_tree(tmp_path)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(net_cfg("efficientnet-b0", False), 31).items()}
    torch.save(sd, tmp_path / "w.pth")
    out = _run(tmp_path, "infer_mcl", "--weights", str(tmp_path / "w.pth"), "--infer_list", lst, "--voc12_root", root, "--num_workers", "0",
               "--out_npy", str(tmp_path / "out"), "--out_cam_npy", str(tmp_path / "cam"), "--pretrained", "b0", "--tblog", str(tmp_path / "tbi"))
    assert [ln.split() for ln in out.strip().splitlines()[-len(names):]] == [[n, str(i)] for i, n in enumerate(names)]
    _script_arithmetic()
    dev = torch.device(DEV)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=False)
    model.load_state_dict(sd, strict=True)
    model = model.to(dev).eval()
    stager = MSFStager(dev)
    gts = {}
    for nm in names:
        img = PIL.Image.open(os.path.join(root, "JPEGImages", nm + ".jpg")).convert("RGB")
        W, H = img.size
        rcam, rsgc, _ = infer.infer_cam(model, stager(img), torch.from_numpy(labels[nm]).view(1, -1), H, W)
        for d, ref in ((tmp_path / "out_sgc", rsgc), (tmp_path / "cam", rcam)):
            got = np.load(d / f"{nm}.npy", allow_pickle=True).item()
            assert sorted(got) == sorted(ref) == [int(c) for c in np.nonzero(labels[nm])[0]]
            for k in ref:
                assert got[k].dtype == np.float32 and got[k].shape == (H, W) and np.array_equal(got[k], ref[k]), (nm, k)
        gts[nm] = np.array(PIL.Image.open(os.path.join(root, "SegmentationClass", nm + ".png")))
    assert not os.path.exists(tmp_path / "out")                       # the reference's commented-out directory (:103)
    # without --out_cam_npy no CAM directory appears
    (tmp_path / "one.txt").write_text(f"/JPEGImages/{names[0]}.jpg\n")
    _run(tmp_path, "infer_mcl", "--weights", str(tmp_path / "w.pth"), "--infer_list", str(tmp_path / "one.txt"), "--voc12_root", root,
         "--out_npy", str(tmp_path / "solo"), "--pretrained", "b0")
    assert sorted(p for p in os.listdir(tmp_path) if p.startswith("solo")) == ["solo_sgc"]
    assert os.listdir(tmp_path / "solo_sgc") == [names[0] + ".npy"]

    # evaluation --type npy --curve True on the directory just written
    gt_dir, log = os.path.join(root, "SegmentationClass"), tmp_path / "evallog.txt"
    out = _run(tmp_path, "evaluation", "--list", lst, "--predict_dir", str(tmp_path / "out_sgc"), "--gt_dir", gt_dir, "--logfile", str(log),
               "--comment", "curve of the test", "--type", "npy", "--curve", "True")
    cev = CamDictEval(dev, [i / 100.0 for i in range(60)])
    for nm in names:
        cev.add(np.load(tmp_path / "out_sgc" / f"{nm}.npy", allow_pickle=True).item(), gts[nm])
    mious = cev.mious()
    lines = [ln for ln in out.splitlines() if "background score" in ln]
    assert lines == ['%d/60 background score: %.3f\tmIoU: %.3f%%' % (i, i / 100.0, mious[i]) for i in range(60)]
    assert max(mious) > min(mious)
    block = log.read_text().splitlines()
    assert len(block) == 3 and re.fullmatch(r"\d{4}-\d\d-\d\d \d\d:\d\d:\d\d\tcurve of the test", block[0])
    assert block[1] == "mIoU:%s  " % mious and block[2] == "====================================="

    # evaluation --type png on infer_seg-style PNGs (8-bit class-index maps)
    g = np.random.default_rng(3)
    seg = SegEval(dev)
    (tmp_path / "png").mkdir()
    for nm in names:
        pred = np.where(g.random(gts[nm].shape) < 0.6, np.where(gts[nm] < 21, gts[nm], 0), g.integers(0, 21, gts[nm].shape)).astype(np.uint8)
        infer.save_seg_png(str(tmp_path / "png" / f"{nm}.png"), pred)
        seg.add(torch.from_numpy(pred).to(dev), torch.from_numpy(gts[nm]).to(dev))
    out = _run(tmp_path, "evaluation", "--list", lst, "--predict_dir", str(tmp_path / "png"), "--gt_dir", gt_dir, "--logfile", str(log),
               "--comment", "png", "--type", "png")
    ll = seg.loglist()
    for c in categories:
        assert '%11s:%7.3f%%' % (c, ll[c]) in out
    assert out.rstrip().endswith('%11s:%7.3f%%' % ('mIoU', ll['mIoU'])) and ll['mIoU'] > 5
    block = log.read_text().splitlines()
    assert len(block) == 6 and block[3].endswith("\tpng") and block[4] == "".join('%s:%s  ' % (k, ll[k]) for k in ll)
    # a single threshold: the row of the curve
    out = _run(tmp_path, "evaluation", "--list", lst, "--predict_dir", str(tmp_path / "out_sgc"), "--gt_dir", gt_dir, "--logfile", str(log),
               "--comment", "t", "--t", "0.3")
    assert out.rstrip().endswith('%11s:%7.3f%%' % ('mIoU', mious[30]))
