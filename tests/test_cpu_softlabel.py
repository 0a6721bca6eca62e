"""Host side of the compact soft pseudo-label (muscle_amd.softlabel): the file format, the planner and the dataset of
muscle_amd.segdata on it, the script arguments and the stager's layout.  No kernel is launched here."""
import os
import random
import zipfile

import numpy as np
import pytest
import torch

import segdata_ref as R
from muscle_amd import _lib, synth

GEOMS = [(19, 25, 75, 100), (19, 23, 74, 90), (19, 23, 76, 92), (8, 8, 32, 29)]


def _seed(s=11):
    random.seed(s)
    torch.manual_seed(s)


def _compact(h, w, H, W, keys=(2, 7, 19), seed=3):
    from muscle_amd.softlabel import CompactSoft
    rw = (synth.uniform(seed, "rw", (len(keys), h, w)) ** 2).astype(np.float32)
    return CompactSoft(np.array(keys, np.uint8), rw, (H, W), np.float32(rw.max()), np.float32(0.25), 21)


def _fields(cs):
    return {"version": np.int32(1), "keys": cs.keys, "rw": cs.rw, "size": np.asarray(cs.size, np.int32), "vmax": cs.vmax,
            "bg": cs.bg, "channels": np.int32(cs.channels)}


@pytest.mark.parametrize("geom", GEOMS, ids=str)
def test_file_round_trip(tmp_path, geom):
    from muscle_amd import softlabel as SL
    for keys in ((4,), (2, 7, 19), tuple(range(20))):
        cs = _compact(*geom, keys=keys)
        path = str(tmp_path / f"a{len(keys)}.npz")
        SL.save_compact(path, cs)
        back = SL.load_compact(path)
        assert back.keys.dtype == np.uint8 and np.array_equal(back.keys, cs.keys)
        assert back.rw.dtype == np.float32 and back.rw.flags.c_contiguous and back.rw.tobytes() == cs.rw.tobytes()
        assert back.size == cs.size and isinstance(back.size, tuple) and back.channels == 21
        assert back.vmax.dtype == np.float32 and back.vmax.tobytes() == cs.vmax.tobytes() and back.bg.tobytes() == cs.bg.tobytes()
        with zipfile.ZipFile(path) as z:                                    # uncompressed, plain arrays only
            assert sorted(z.namelist()) == sorted(k + ".npy" for k in _fields(cs))
            assert all(i.compress_type == zipfile.ZIP_STORED for i in z.infolist())
        with np.load(path, allow_pickle=False) as z:
            assert all(z[k].dtype != object for k in z.files)
        assert os.path.getsize(path) < cs.rw.nbytes + 4096


def test_malformed_files_raise(tmp_path):
    from muscle_amd import softlabel as SL
    cs = _compact(19, 23, 74, 90)
    good = _fields(cs)

    def written(**over):
        path = str(tmp_path / "bad.npz")
        np.savez(path, **dict(good, **over))
        return path

    SL.load_compact(written())                                             # the unmodified fields load
    bad = {
        "unknown version": dict(version=np.int32(2)),
        "rw float64": dict(rw=cs.rw.astype(np.float64)),
        "rw float16": dict(rw=cs.rw.astype(np.float16)),
        "keys int64": dict(keys=cs.keys.astype(np.int64)),
        "size int64": dict(size=np.asarray(cs.size, np.int64)),
        "vmax float64": dict(vmax=np.float64(cs.vmax)),
        "bg float64": dict(bg=np.float64(cs.bg)),
        "keys descending": dict(keys=np.array([7, 2, 19], np.uint8)),
        "keys repeated": dict(keys=np.array([2, 2, 19], np.uint8)),
        "key == channels - 1": dict(keys=np.array([2, 7, 20], np.uint8)),
        "H > 4h": dict(size=np.array([77, 90], np.int32)),
        "W > 4w": dict(size=np.array([74, 93], np.int32)),
        "vmax zero": dict(vmax=np.float32(0)),
        "vmax negative": dict(vmax=np.float32(-1)),
        "vmax nan": dict(vmax=np.float32(np.nan)),
        "vmax inf": dict(vmax=np.float32(np.inf)),
        "keys / rw disagree": dict(keys=np.array([2, 7], np.uint8)),
    }
    for what, over in bad.items():
        try:
            SL.load_compact(written(**over))
        except ValueError:
            continue
        raise AssertionError(f"{what}: loaded")
    with pytest.raises(ValueError):                                        # a pickled object is refused, not unpickled
        SL.load_compact(written(keys=np.array([{"a": 1}], dtype=object)))
    with pytest.raises(ValueError):
        SL.save_compact(str(tmp_path / "zero.npz"), SL.CompactSoft(cs.keys, cs.rw, cs.size, 0.0, 0.25, 21))
    assert not (tmp_path / "zero.npz").exists()


def test_expand_has_no_cpu_path():
    from muscle_amd import softlabel as SL
    with pytest.raises(_lib.MuscleHipError):
        SL.expand(_compact(8, 8, 32, 29), "cpu")


@pytest.mark.parametrize("geom", GEOMS, ids=str)
@pytest.mark.parametrize("augment", [True, False])
def test_planner_treats_both_forms_alike(geom, augment):
    from muscle_amd import segdata as D
    h, w, H, W = geom
    cs = _compact(h, w, H, W)
    img, m = R.synth_image(H, W, 1), R.synth_label(H, W, 1)
    narrowed = 0
    for seed in range(6):
        for crop in (24, 64, 160):
            _seed(seed)
            pd = D.plan_seg_item(img, m, 0.5, 1.75, crop, augment=augment)
            after = (random.random(), float(torch.rand(1)))
            _seed(seed)
            pc = D.plan_seg_item(img, cs, 0.5, 1.75, crop, augment=augment)
            assert (random.random(), float(torch.rand(1))) == after       # both generators consumed identically
            assert R.plan_as_draws(pc) == R.plan_as_draws(pd)
            for k in ("scale", "img_crop", "place", "flip", "span_cap", "resize_to", "jitter"):
                assert getattr(pc, k) == getattr(pd, k), k
            assert np.array_equal(pc.tables, pd.tables) and np.array_equal(pc.img_u8, pd.img_u8)
            for a, b in zip(pc.mask_y + pc.mask_x, pd.mask_y + pd.mask_x):
                assert a.dtype == b.dtype and np.array_equal(a, b)
            assert pd.compact is None and pc.compact is cs and pc.mask_src is None
            r0, r1 = pc.mask_rows
            assert pd.mask_rows == (r0, r1) and 0 <= r0 < r1 <= H
            assert np.array_equal(pd.mask_src, m[r0:r1])                   # the rows the dense plan sliced
            assert pc.channels == pd.channels == 21
            narrowed += (r0, r1) != (0, H)
    assert narrowed > 0                                                   # windows narrower than the label were among them


def _tree(tmp_path, kinds):
    """JPEGImages + a list + per name the label files `kinds[i]` names: 'npy', 'npz' or 'both'."""
    from muscle_amd import softlabel as SL
    root, mroot = tmp_path / "VOC2012", tmp_path / "soft"
    (root / "JPEGImages").mkdir(parents=True)
    mroot.mkdir()
    names = [f"2007_{i:06d}" for i in range(len(kinds))]
    for i, (nm, kind) in enumerate(zip(names, kinds)):
        h, w, H, W = GEOMS[i % len(GEOMS)]
        R.synth_image(H, W, i).save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        if kind in ("npy", "both"):
            np.save(mroot / f"{nm}.npy", R.synth_label(H, W, i))
        if kind in ("npz", "both"):
            SL.save_compact(str(mroot / f"{nm}.npz"), _compact(h, w, H, W, seed=i))
    lst = tmp_path / "train_aug.txt"
    lst.write_text("".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png\n" for n in names))
    return str(lst), str(root), str(mroot), names


def test_dataset_chooses_the_file_by_mask_format(tmp_path):
    from muscle_amd import segdata as D
    from muscle_amd.softlabel import CompactSoft
    lst, root, mroot, names = _tree(tmp_path, ("npy", "npz", "both"))
    kind = lambda ds, i: "npz" if isinstance(ds.load_mask(names[i]), CompactSoft) else "npy"        # noqa: E731
    labels = {n: np.zeros(20, np.float32) for n in names}
    ds = {f: D.VOC12SegDataset(lst, root, mroot, 0.5, 1.75, crop_size=64, labels=labels, mask_format=f)
          for f in ("auto", "dense", "compact")}
    assert D.VOC12SegDataset(lst, root, mroot, labels=labels).mask_format == "auto"
    assert [kind(ds["auto"], i) for i in range(3)] == ["npy", "npz", "npy"]
    assert kind(ds["dense"], 0) == "npy" and kind(ds["dense"], 2) == "npy"
    assert kind(ds["compact"], 1) == "npz" and kind(ds["compact"], 2) == "npz"
    with pytest.raises(FileNotFoundError):
        ds["dense"].load_mask(names[1])
    with pytest.raises(FileNotFoundError):
        ds["compact"].load_mask(names[0])
    os.remove(os.path.join(mroot, names[1] + ".npz"))
    with pytest.raises(FileNotFoundError):
        ds["auto"].load_mask(names[1])
    with pytest.raises(ValueError, match="mask_format"):
        D.VOC12SegDataset(lst, root, mroot, labels=labels, mask_format="npz")
    # plan() goes through it: a compact plan from the .npz, a dense plan from the .npy, the same draws under the same seed
    _seed(5)
    _, pc, _ = ds["compact"].plan(2)
    _seed(5)
    _, pd, _ = ds["dense"].plan(2)
    assert pc.compact is not None and pd.compact is None and R.plan_as_draws(pc) == R.plan_as_draws(pd)
    assert pc.mask_rows == pd.mask_rows and pd.mask_src.shape[0] == pd.mask_rows[1] - pd.mask_rows[0]


def test_script_arguments():
    from muscle_amd import infer_irn, train_muscle
    a = infer_irn.parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "c", "--soft_output", "2"])
    assert a.soft_output == 2
    assert infer_irn.parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "c"]).soft_output == 0
    assert train_muscle.parse_args(["--mask_root", "M"]).mask_format == "auto"
    for f in ("auto", "dense", "compact"):
        assert train_muscle.parse_args(["--mask_root", "M", "--mask_format", f]).mask_format == f
    with pytest.raises(SystemExit):
        train_muscle.parse_args(["--mask_root", "M", "--mask_format", "npz"])
    from muscle_amd import softlabel as SL
    u = SL.parse_args(["unpack", "in", "out", "--list", "l.txt"])
    assert (u.cmd, u.in_dir, u.out_dir, u.list) == ("unpack", "in", "out", "l.txt")


def test_stager_layout_of_a_compact_item():
    """A compact item ships K*h*w*4 + K bytes (rw, then keys) where a dense item ships its rows, and owns a scratch region of
    (r1-r0) * W * 42 bytes for the expanded rows; a dense batch is laid out as before."""
    from muscle_amd import segdata as D
    from muscle_amd.softlabel import expand_job
    al = lambda v, a=16: (v + a - 1) // a * a                              # noqa: E731
    stager = D.SegStager(torch.device("cpu"), 4, 64)
    plans = {}
    for form in ("dense", "compact"):
        _seed(2)
        plans[form] = []
        for i, (h, w, H, W) in enumerate(GEOMS):
            src = R.synth_label(H, W, i) if form == "dense" else _compact(h, w, H, W, keys=((4,), (2, 7, 19), tuple(range(20)), (0, 19))[i])
            plans[form].append(D.plan_seg_item(R.synth_image(H, W, i), src, 0.5, 1.75, 64))
    Ld = stager.layout(plans["dense"])
    copied_dense, total_dense = stager.buf.copied, stager.buf.total
    assert Ld["sj"] is None and Ld["exp"] == [None] * 4
    assert total_dense == Ld["sums"] + 4 * 8                               # nothing behind the jitter's sums
    Lc = stager.layout(plans["compact"])
    assert Lc["sj"] % 64 == 0 and Lc["sj"] >= Lc["mj"] + 4 * 64 and Lc["tab"][0] >= Lc["sj"] + 4 * 64
    end = Lc["img"][-1] + plans["compact"][-1].img_u8.size
    for i, p in enumerate(plans["compact"]):
        K, h, w = p.compact.rw.shape
        assert p.compact.nbytes == K * h * w * 4 + K
        assert Lc["msk"][i] == al(end)                                     # exactly the bytes, plus alignment
        end = Lc["msk"][i] + K * h * w * 4 + K
        nxt = Lc["exp"][i + 1] if i + 1 < 4 else stager.buf.total
        r0, r1 = p.mask_rows
        assert Lc["exp"][i] % 16 == 0 and Lc["exp"][i] >= stager.buf.copied
        assert nxt - Lc["exp"][i] == (al((r1 - r0) * p.compact.size[1] * 42) if i + 1 < 4 else (r1 - r0) * p.compact.size[1] * 42)
        job = expand_job(p.compact, Lc["msk"][i], Lc["exp"][i], p.mask_rows)
        assert job.dtype == np.int32 and job.shape == (16,) and not job[13:].any()
        assert job[:11].tolist() == [Lc["msk"][i], Lc["msk"][i] + K * h * w * 4, K, h, w, p.compact.size[0], p.compact.size[1], r0, r1 - r0,
                                     Lc["exp"][i], 21]
        assert job[11:13].view(np.float32).tolist() == [float(p.compact.vmax), 0.25]
    assert stager.buf.copied == end and stager.buf.copied < copied_dense
    # a mixed batch: only the compact items get a job and a scratch region
    mixed = [plans["dense"][0], plans["compact"][1], plans["dense"][2], plans["compact"][3]]
    Lm = stager.layout(mixed)
    assert [e is not None for e in Lm["exp"]] == [False, True, False, True]
    assert Lm["tab"][0] >= Lm["sj"] + 2 * 64


def test_header_declares_the_entry_point():
    sigs = _lib.parse_header()
    assert sigs.get("mx_soft_expand") == "ppip"
    text = open(_lib.HEADER_PATH).read()
    assert "infer_irn.py:79-88" in text and "src/data.py:102" in text
    LL = _lib.lib()                                                        # argument errors are reported before any launch
    assert LL.mx_soft_expand(None, None, 1, None) < 0 and b"soft_expand" in LL.mx_last_error()
    import ctypes
    word = ctypes.c_int(0)
    p = ctypes.cast(ctypes.pointer(word), ctypes.c_void_p)
    for n in (0, -1, 65536):
        assert LL.mx_soft_expand(p, p, n, None) < 0 and b"soft_expand" in LL.mx_last_error()
