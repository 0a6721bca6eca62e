"""Host half of the hard-label-map path (mask_type="label") of decoder training: muscle_amd.segdata.nearest_axis_table pinned
against Pillow itself, plan_label_item against "Pillow resize, crop, pad with 255, flip" done directly, the draws against the
soft path's, and every refusal.  The device half is tests/test_gpu_label_path.py; the restatements are in tests/label_ref.py."""
import os
import random

import numpy as np
import pytest
import torch

import label_ref as LR
import segdata_ref as R


def _seed(s):
    random.seed(s)
    torch.manual_seed(s)


# (n_in, n_out): every small pair, and the two VOC extents over the whole scale range 0.5 .. 1.75
SWEEP = [(i, o) for i in range(1, 65) for o in range(1, 131)] + [(375, o) for o in range(188, 657)] + \
    [(500, o) for o in range(250, 876)]


def test_nearest_table_equals_pillow_over_a_sweep():
    """Pillow steps its source coordinate by repeated addition, so four size pairs prove nothing: every pair of the sweep is
    compared with the row Pillow returns, whole and as a window (a window is a slice of the whole axis)."""
    from muscle_amd.segdata import nearest_axis_table
    differs_from_closed_form = 0
    for k, (n_in, n_out) in enumerate(SWEEP):
        want = LR.pil_nearest_axis(n_in, n_out)
        got = nearest_axis_table(n_in, n_out)
        assert got.dtype == np.int32 and np.array_equal(got, want), (n_in, n_out)
        lo = (k * 7) % n_out
        cnt = 1 + (k * 13) % (n_out - lo)
        assert np.array_equal(nearest_axis_table(n_in, n_out, lo, cnt), want[lo:lo + cnt]), (n_in, n_out, lo, cnt)
        closed = np.floor((np.arange(n_out) + 0.5) * n_in / n_out).astype(np.int32)
        differs_from_closed_form += int(not np.array_equal(closed, want))
    print(f"{len(SWEEP)} size pairs; Pillow differs from floor((x + 0.5) * n_in / n_out) for {differs_from_closed_form} of them")
    with pytest.raises(ValueError):
        nearest_axis_table(5, 7, 3, 5)


# (H, W, crop): smaller than the crop in both axes at every scale (place offsets > 0), larger in both, 1 x 1, 1 x 7, odd widths
PLAN_CASES = [(31, 23, 64), (150, 131, 40), (1, 1, 8), (1, 7, 8), (75, 101, 96), (97, 33, 48)]


@pytest.mark.parametrize("case", PLAN_CASES, ids=lambda c: "x".join(map(str, c)))
def test_plan_tables_equal_pillow_resize_crop_pad_flip(case):
    from muscle_amd import segdata as D
    H, W, crop = case
    img, label = R.synth_image(H, W, 3), LR.synth_label_map(H, W, 5)
    seen = set()
    for seed in range(8):
        low = 1.0 if H == 1 else 0.5                                  # (half of a one-pixel axis rounds to nothing: the plan refuses)
        for s in (low, 1.75, None):                                   # None: a random scale of the range
            _seed(seed)
            lo, hi = (low, 1.75) if s is None else (s, s)
            p = D.plan_label_item(img, label, lo, hi, crop)
            d = R.plan_as_draws(p)
            got = LR.plan_label_cpu(p, crop)
            assert got.dtype == np.uint8 and np.array_equal(got, LR.ref_label(label, d, crop)), (seed, s)
            r0, r1 = p.label_rows
            assert p.label_src.shape == (r1 - r0, W) and np.array_equal(p.label_src, label[r0:r1])       # only the rows it reads
            assert p.label_y.dtype == np.int32 and p.label_y.min() == 0 and p.label_y.max() == r1 - r0 - 1
            seen.add((p.place[0] > 0, p.place[1] > 0, p.flip))
    if (H, W, crop) == (31, 23, 64):
        assert {(True, True, False), (True, True, True)} <= seen      # offsets above 0 in both axes, flipped and not
    if (H, W, crop) == (150, 131, 40):
        assert all(not a and not b for a, b, _ in seen)               # larger than the crop in both axes at every scale


@pytest.mark.parametrize("augment", [True, False])
def test_label_plan_makes_the_soft_plans_draws(augment):
    from muscle_amd import segdata as D
    img, soft, label = R.synth_image(75, 100, 1), R.synth_label(75, 100, 1), LR.synth_label_map(75, 100, 1)
    for seed in range(6):
        for crop in (64, 160):
            _seed(seed)
            a = D.plan_seg_item(img, soft, 0.5, 1.75, crop, augment=augment)
            after = (random.random(), float(torch.rand(1)))
            _seed(seed)
            b = D.plan_label_item(img, label, 0.5, 1.75, crop, augment=augment)
            assert (random.random(), float(torch.rand(1))) == after   # both generators consumed identically
            assert R.plan_as_draws(a) == R.plan_as_draws(b)
            assert np.array_equal(a.img_u8, b.img_u8) and np.array_equal(a.tables, b.tables)


def _tree(tmp_path, sizes=((40, 52), (33, 47))):
    import PIL.Image
    root, mroot = tmp_path / "VOC2012", tmp_path / "png"
    (root / "JPEGImages").mkdir(parents=True)
    mroot.mkdir()
    names = [f"2008_{i:06d}" for i in range(len(sizes))]
    for i, (nm, (h, w)) in enumerate(zip(names, sizes)):
        R.synth_image(h, w, i).save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        im = PIL.Image.fromarray(LR.synth_label_map(h, w, i), "P" if i % 2 else "L")
        if i % 2:
            im.putpalette([v for k in range(256) for v in (k, 255 - k, (k * 7) % 256)])
        im.save(mroot / f"{nm}.png")
    lst = tmp_path / "train.txt"
    lst.write_text("".join(f"/JPEGImages/{n}.jpg /SegmentationClassAug/{n}.png\n" for n in names))
    labels = {n: np.eye(20, dtype=np.float32)[i % 20] for i, n in enumerate(names)}
    return str(lst), str(root), str(mroot), labels, names


def test_dataset_reads_label_maps_and_refuses_bad_files(tmp_path):
    import PIL.Image
    from muscle_amd import segdata as D
    lst, root, mroot, labels, names = _tree(tmp_path)
    with pytest.raises(NotImplementedError, match="soft"):
        D.VOC12SegDataset(lst, root, mroot, mask_type="hard", labels=labels)
    ds = D.VOC12SegDataset(lst, root, mroot, 0.5, 1.75, crop_size=48, mask_type="label", labels=labels, mask_format="compact")
    _seed(2)
    for i, nm in enumerate(names):                                    # mode L and mode P (palette indices, not colours)
        name, p, lab = ds[i]
        assert name == nm and isinstance(p, D.LabelItemPlan) and np.array_equal(lab, labels[nm])
        src = LR.synth_label_map(*((40, 52), (33, 47))[i], i)
        assert np.array_equal(LR.plan_label_cpu(p, 48), LR.ref_label(src, R.plan_as_draws(p), 48))
    # refusals: each names the file and comes from plan(), on the host
    bad = os.path.join(mroot, names[0] + ".png")
    good = PIL.Image.open(bad).copy()
    PIL.Image.fromarray(np.zeros((40, 52, 3), np.uint8), "RGB").save(bad)
    with pytest.raises(ValueError, match=names[0]):
        ds.plan(0)
    PIL.Image.fromarray(np.zeros((41, 52), np.uint8), "L").save(bad)
    with pytest.raises(ValueError, match=names[0]):
        ds.plan(0)
    a = np.array(good)
    a[7, 9] = 37
    PIL.Image.fromarray(a, "L").save(bad)
    with pytest.raises(ValueError, match=names[0] + r".*37"):
        ds.plan(0)
    assert D.VOC12SegDataset(lst, root, mroot, crop_size=48, mask_type="label", labels=labels, num_classes=38).plan(0)[0] == names[0]
    a[7, 9] = 255
    PIL.Image.fromarray(a, "L").save(bad)
    assert ds.plan(0)[0] == names[0]


def test_mixed_batch_is_refused():
    from muscle_amd import segdata as D
    img = R.synth_image(40, 52, 1)
    _seed(1)
    soft = D.plan_seg_item(img, R.synth_label(40, 52, 1), 0.5, 1.75, 48)
    hard = D.plan_label_item(img, LR.synth_label_map(40, 52, 1), 0.5, 1.75, 48)
    stager = D.SegStager(torch.device("cpu"), 2, 48)
    with pytest.raises(ValueError, match="share a batch"):
        stager([soft, hard])
    with pytest.raises(ValueError, match="share a batch"):
        stager.layout([hard, soft])
    L = stager.layout([hard, hard])                                   # a label batch plans without a GPU
    assert len(L["msk"]) == 2 and L["sj"] is None
    with pytest.raises(ValueError):
        D.plan_label_item(img, np.zeros((40, 51), np.uint8))
    with pytest.raises(ValueError):
        D.plan_label_item(img, np.zeros((40, 52), np.int32))


def test_script_takes_mask_type():
    from muscle_amd import train_muscle
    assert train_muscle.parse_args(["--mask_root", "M"]).mask_type == "soft"
    assert train_muscle.parse_args(["--mask_root", "M", "--mask_type", "label"]).mask_type == "label"
    for word in ("hard", "png"):
        with pytest.raises(SystemExit):
            train_muscle.parse_args(["--mask_root", "M", "--mask_type", word])


def test_header_declares_the_three_entries():
    from muscle_amd._lib import parse_header
    sigs = parse_header()
    assert sigs.get("mx_label_stage") == "ppppiiip"
    assert sigs.get("mx_ce_label") == "ppipppiiliplp"
    assert sigs.get("mx_field_mask_label") == "ppipiiiiip"
