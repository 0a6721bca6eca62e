"""The pair-table kernels (csrc/ins_eval.hip) and the evaluation built on them (muscle_amd/ins_eval.py) on the GPU.  Every table
is compared EXACTLY with the numpy restatement tests/ins_eval_ref.py; AP to 1e-12 (float64 on identical integers).

Shapes: 1x1, 1x70, 70x1 (one row, one column), 7x13 (less than one wave, odd W), 33x65 (ragged against 64 lanes, against the
16-pixel groups and against 4-byte packing), 375x500 (46 workgroups).  Tables: 186 cells (LDS tile), 12 341 cells (global
atomics), and 8192 / 8193 cells, the two sides of the threshold between the two.  Inputs are also handed in at every byte offset
0..16 from an aligned address: the packed loads start on an unaligned pixel and end ragged."""
import numpy as np
import pytest
import torch

import ins_eval_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENTINEL = -77
T4 = (0.25, 0.5, 0.7, 0.75)


def _maps(H, W, A, B, seed=0):
    a = R.blobs(H, W, min(A, 400), seed)
    b = R.blobs(H, W, min(B, 255), seed + 100).astype(np.uint8)
    return a, b


def _run_label(a, b, A, B):
    from muscle_amd import label_pair_counts
    t, bad = label_pair_counts(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), A, B)
    return t.cpu().numpy().reshape(A + 1, B + 1), int(bad.cpu())


def _run_mask(masks, b, B):
    from muscle_amd import mask_pair_counts
    t, bad = mask_pair_counts(torch.from_numpy(masks).to(DEV), torch.from_numpy(b).to(DEV), B)
    return t.cpu().numpy().reshape(masks.shape[0] + 1, B + 1), int(bad.cpu())


def _same(got, ref):
    assert got.dtype == np.int32 and got.shape == ref.shape
    diff = int((got.astype(np.int64) != ref).sum())
    print(f"[ins_eval] table {ref.shape}: {diff} cells differ, sum {int(ref.sum())}")
    assert diff == 0


# ---- label-map form ---------------------------------------------------------------------------------------------------------
LABEL_CASES = [(1, 1, 3, 2), (1, 70, 3, 2), (70, 1, 3, 2), (7, 13, 3, 2), (33, 65, 9, 4), (375, 500, 30, 5), (375, 500, 300, 40),
               (33, 65, 0, 0), (33, 65, 0, 254), (33, 65, 5, 255),
               (33, 65, 4095, 1), (33, 65, 2730, 2)]                  # 8192 cells: the largest LDS tile; 8193: the smallest global table


@pytest.mark.parametrize("case", LABEL_CASES, ids=lambda c: "%dx%d-A%d-B%d" % c)
def test_label_table_equals_the_restatement(case):
    H, W, A, B = case
    a, b = _maps(H, W, A, B)
    if A > 400:
        a = (a * (A // 400)).astype(np.int32)                          # spread over the whole table, A itself included
        a[-1, -1] = A
    if B == 255:
        b.reshape(-1)[::7] = 255
        assert (b == 255).sum() > 0
    ref, nbad = R.label_table(a, b, A, B)
    assert nbad == 0 and ref.sum() == H * W
    got, bad = _run_label(a, b, A, B)
    _same(got, ref)
    assert bad == 0


@pytest.mark.parametrize("AB", [(30, 5), (300, 40)], ids=["lds", "global"])
def test_label_contention_one_pair_everywhere(AB):
    H, W = 375, 500
    got, bad = _run_label(np.full((H, W), 7, np.int32), np.full((H, W), 3, np.uint8), *AB)
    assert got[7, 3] == H * W and got.sum() == H * W and bad == 0


@pytest.mark.parametrize("cells", ["lds", "global"])
def test_label_checkerboard_changes_pair_at_every_pixel(cells):
    H, W = 375, 500
    A, B = (30, 5) if cells == "lds" else (300, 40)
    yy, xx = np.mgrid[:H, :W]
    a = np.where((yy + xx) % 2 == 0, A, 1).astype(np.int32)
    b = np.where((yy + xx) % 2 == 0, 0, B).astype(np.uint8)
    got, bad = _run_label(a, b, A, B)
    _same(got, R.label_table(a, b, A, B)[0])
    assert got[A, 0] == (H * W + 1) // 2 and got[1, B] == H * W // 2 and bad == 0


@pytest.mark.parametrize("off", [0, 1, 2, 3, 5, 8, 15, 16])
def test_inputs_at_every_alignment(off):
    """a, b and the mask stack start `off` elements / bytes after an aligned address; the pixel count 33*65 = 2145 is odd."""
    from muscle_amd import label_pair_counts, mask_pair_counts
    H, W, A, B = 33, 65, 9, 4
    a, b = _maps(H, W, A, B, seed=off)
    masks = (np.stack([R.blobs(H, W, 2, 50 + p) for p in range(3)]) > 0).astype(np.uint8)
    n = H * W
    a_buf = torch.zeros(n + 32, dtype=torch.int32, device=DEV)
    b_buf = torch.full((n + 32,), 255, dtype=torch.uint8, device=DEV)             # out of range if a load strays outside
    m_buf = torch.full((3 * n + 32,), 1, dtype=torch.uint8, device=DEV)
    a_buf[off:off + n] = torch.from_numpy(a.reshape(-1)).to(DEV)
    b_buf[off:off + n] = torch.from_numpy(b.reshape(-1)).to(DEV)
    m_buf[off:off + 3 * n] = torch.from_numpy(masks.reshape(-1)).to(DEV)
    t, bad = label_pair_counts(a_buf[off:off + n], b_buf[off:off + n], A, B)
    _same(t.cpu().numpy().reshape(A + 1, B + 1), R.label_table(a, b, A, B)[0])
    assert int(bad.cpu()) == 0
    t, bad = mask_pair_counts(m_buf[off:off + 3 * n].view(3, n), b_buf[off:off + n], B)
    _same(t.cpu().numpy().reshape(4, B + 1), R.mask_table(masks, b, B)[0])
    assert int(bad.cpu()) == 0


# ---- mask form --------------------------------------------------------------------------------------------------------------
def _masks(n, H, W, seed):
    rng = np.random.RandomState(seed)
    out = np.zeros((n, H, W), bool)
    for p in range(n):
        out[p] = (R.blobs(H, W, 2, seed + p) > 0) ^ (rng.rand(H, W) < 0.02)       # rectangles that overlap each other, with noise
    return out


@pytest.mark.parametrize("case", [(0, 47, 63, 6), (1, 47, 63, 6), (37, 47, 63, 6), (30, 375, 500, 5), (3, 1, 1, 2), (2, 7, 13, 255)],
                         ids=lambda c: "n%d-%dx%d-B%d" % c)
def test_mask_table_equals_the_restatement(case):
    n, H, W, B = case
    masks = _masks(n, H, W, 3)
    b = R.blobs(H, W, min(B, 40), 9).astype(np.uint8)
    if B == 255:
        b.reshape(-1)[::5] = 255
    ref, nbad = R.mask_table(masks, b, B)
    got, bad = _run_mask(masks, b, B)
    _same(got, ref)
    assert bad == 0 and nbad == 0 and got[0].sum() == H * W               # row 0 counts every pixel, n = 0 included


def test_mask_all_false_all_true_and_other_non_zero_values():
    H, W, B = 47, 63, 6
    b = R.blobs(H, W, B, 4).astype(np.uint8)
    masks = np.zeros((4, H, W), np.uint8)
    masks[1] = 1
    masks[2] = 255                                                       # any non-zero byte is "set"
    masks[3] = np.random.RandomState(0).randint(0, 3, (H, W)) * 64       # 0, 64, 128
    got, bad = _run_mask(masks, b, B)
    _same(got, R.mask_table(masks, b, B)[0])
    assert not got[1].any() and np.array_equal(got[2], got[0]) and np.array_equal(got[3], got[0]) and got[4].sum() == (masks[3] > 0).sum()
    assert bad == 0


# ---- guards -----------------------------------------------------------------------------------------------------------------
def _guarded(cells):
    buf = torch.full((64 + cells + 64,), SENTINEL, dtype=torch.int32, device=DEV)
    bad = torch.full((3,), SENTINEL, dtype=torch.int32, device=DEV)
    return buf, buf[64:64 + cells], bad, bad[1:2]


def _guards_untouched(buf, cells, bad):
    h, hb = buf.cpu().numpy(), bad.cpu().numpy()
    assert (h[:64] == SENTINEL).all() and (h[64 + cells:] == SENTINEL).all() and hb[0] == SENTINEL and hb[2] == SENTINEL
    return h[64:64 + cells], int(hb[1])


def test_the_words_around_the_table_stay_untouched():
    from muscle_amd import label_pair_counts, mask_pair_counts
    H, W, A, B = 33, 65, 9, 4
    a, b = _maps(H, W, A, B)
    buf, table, bad3, bad = _guarded((A + 1) * (B + 1))
    label_pair_counts(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), A, B, table, bad)
    t, nb = _guards_untouched(buf, (A + 1) * (B + 1), bad3)               # the table was sentinel-filled: the entry overwrites it
    _same(t.reshape(A + 1, B + 1), R.label_table(a, b, A, B)[0])
    assert nb == 0
    masks = _masks(5, H, W, 1)
    buf, table, bad3, bad = _guarded(6 * (B + 1))
    mask_pair_counts(torch.from_numpy(masks).to(DEV), torch.from_numpy(b).to(DEV), B, table, bad)
    t, nb = _guards_untouched(buf, 6 * (B + 1), bad3)
    _same(t.reshape(6, B + 1), R.mask_table(masks, b, B)[0])
    assert nb == 0


def test_out_of_range_values_are_counted_and_never_index_the_table():
    """a = A+1, a = -1 and b = B+1 in a few pixels: bad equals their number, the in-range counts stay exact, the words around the
    table are untouched and pair_table raises.  No such value ever forms an index, so nothing here can fault."""
    from muscle_amd import label_pair_counts, mask_pair_counts, pair_table
    from muscle_amd.ins_seg import InstanceLabels
    H, W, A, B = 33, 65, 9, 4
    a, b = _maps(H, W, A, B)
    a[0, 0], a[5, 7], a[32, 64], a[10, 10] = A + 1, -1, A + 1, -1
    b[10, 10], b[20, 3], b[32, 63] = B + 1, B + 1, 255                   # (10,10) is bad twice over and counts once
    ref, nbad = R.label_table(a, b, A, B)
    assert nbad == 6 and ref.sum() == H * W - 6
    cells = (A + 1) * (B + 1)
    buf, table, bad3, bad = _guarded(cells)
    label_pair_counts(torch.from_numpy(a).to(DEV), torch.from_numpy(b).to(DEV), A, B, table, bad)
    t, nb = _guards_untouched(buf, cells, bad3)
    _same(t.reshape(A + 1, B + 1), ref)
    assert nb == 6
    masks = _masks(5, H, W, 1)
    masks[:, 10, 10] = True                                              # every mask covers a bad pixel: still counted once
    ref, nbad = R.mask_table(masks, b, B)
    assert nbad == 3
    buf, table, bad3, bad = _guarded(6 * (B + 1))
    mask_pair_counts(torch.from_numpy(masks).to(DEV), torch.from_numpy(b).to(DEV), B, table, bad)
    t, nb = _guards_untouched(buf, 6 * (B + 1), bad3)
    _same(t.reshape(6, B + 1), ref)
    assert nb == 3
    G = torch.from_numpy(b).to(DEV)
    with pytest.raises(ValueError, match="outside"):
        pair_table(masks, G, B)
    ins = InstanceLabels(torch.from_numpy(a).to(DEV), np.zeros(A, np.float32), np.zeros(A, np.int64), np.zeros(A, np.int32))
    with pytest.raises(ValueError, match="outside"):
        pair_table(ins, torch.from_numpy(np.minimum(b, B)).to(DEV), B)


# ---- equivalence and end to end ---------------------------------------------------------------------------------------------
def _instance_labels(seg, score, cls):
    from muscle_amd.ins_seg import InstanceLabels
    area = np.bincount(seg.reshape(-1), minlength=len(score) + 1)[1:].astype(np.int32)
    return InstanceLabels(torch.from_numpy(seg).to(DEV), score, cls, area)


def test_label_form_and_mask_form_agree():
    from muscle_amd import InsSegEval, mask_iou, pair_table, voc_instances
    H, W = 47, 63
    seg, score, cls, cls_png, obj_png = R.synthetic_image(H, W, 11, 5, 0)
    ins = _instance_labels(seg, score, cls)
    G, gt_cls = voc_instances(cls_png, obj_png)
    G_dev = torch.from_numpy(G).to(DEV)
    t_label = pair_table(ins, G_dev, gt_cls.size)
    d = ins.to_irn_dict()
    t_mask = pair_table(d, G_dev, gt_cls.size)
    assert t_label.shape == t_mask.shape == (12, gt_cls.size + 1) and gt_cls.size >= 3
    assert np.array_equal(t_label[1:], t_mask[1:]) and np.array_equal(t_label.sum(0), t_mask[0])
    iou = mask_iou(t_label, False)
    assert np.array_equal(iou, mask_iou(t_mask, True))
    assert np.array_equal(iou, R.iou_from_masks(d["mask"], G, gt_cls.size)) and iou.max() > 0.75
    assert np.array_equal(pair_table(torch.from_numpy(d["mask"]).to(DEV), G_dev), t_mask)       # a device tensor; m found from G
    a, b = InsSegEval(DEV), InsSegEval(DEV)
    a.add(ins, cls_png, obj_png)
    b.add(d, cls_png, obj_png)
    ra, rb = a.result(), b.result()
    assert np.array_equal(ra["ap"], rb["ap"], equal_nan=True) and np.array_equal(ra["map"], rb["map"], equal_nan=True)


def _three_images():
    return [R.synthetic_image(H, W, n, m, seed) for (H, W, n, m, seed) in ((47, 63, 11, 5, 0), (33, 65, 7, 6, 1), (24, 31, 4, 2, 2))]


def test_end_to_end_ap_equals_the_restatement():
    from muscle_amd import InsSegEval
    ev = InsSegEval(DEV, 20, T4)
    ref_in = []
    for seg, score, cls, cls_png, obj_png in _three_images():
        ev.add(_instance_labels(seg, score, cls), cls_png, obj_png)
        G, gt_cls = R.gt_instances(cls_png, obj_png)
        masks = seg[None] == np.arange(1, len(score) + 1)[:, None, None]
        ref_in.append((R.iou_from_masks(masks, G, len(gt_cls)), score, cls, gt_cls))
    got, ref = ev.result(), R.evaluate(ref_in, 20, T4)
    assert np.array_equal(np.isnan(got["ap"]), np.isnan(ref["ap"]))
    d, dm = np.nanmax(np.abs(got["ap"] - ref["ap"])), np.abs(got["map"] - ref["map"]).max()
    print(f"[ins_eval] end to end: max |dAP| = {d:.3g}, max |dmAP| = {dm:.3g}, mAP = {got['map']}")
    assert d <= 1e-12 and dm <= 1e-12
    assert got["map"][0] > got["map"][3] >= 0 and got["map"][0] > 0.2       # the thresholds bite: not a degenerate case


def test_two_runs_give_identical_bits():
    a, b = _maps(375, 500, 300, 40)
    masks = _masks(8, 375, 500, 2)
    r1, r2 = _run_label(a, b, 300, 40), _run_label(a, b, 300, 40)
    assert r1[0].tobytes() == r2[0].tobytes() and r1[1] == r2[1]
    a2, b2 = _maps(375, 500, 30, 5)
    assert _run_label(a2, b2, 30, 5)[0].tobytes() == _run_label(a2, b2, 30, 5)[0].tobytes()
    assert _run_mask(masks, b, 40)[0].tobytes() == _run_mask(masks, b, 40)[0].tobytes()


def test_host_tensors_and_size_mismatches_are_refused():
    from muscle_amd import pair_table
    from muscle_amd._lib import MuscleHipError
    seg, score, cls, cls_png, obj_png = R.synthetic_image(24, 31, 4, 2, 2)
    G_dev = torch.zeros(24, 31, dtype=torch.uint8, device=DEV)
    with pytest.raises(MuscleHipError):
        pair_table(_instance_labels(seg, score, cls), G_dev.cpu(), 2)
    ins = _instance_labels(seg, score, cls)
    ins.seg_map = ins.seg_map.cpu()
    with pytest.raises(MuscleHipError):
        pair_table(ins, G_dev, 2)
    with pytest.raises(MuscleHipError):
        pair_table(torch.zeros(2, 24, 31, dtype=torch.bool), G_dev, 2)
    with pytest.raises(ValueError):
        pair_table(_instance_labels(seg, score, cls), G_dev[:, :30].contiguous(), 2)
    with pytest.raises(ValueError):
        pair_table(np.zeros((2, 24, 30), bool), G_dev, 2)
    with pytest.raises(ValueError):
        pair_table(np.zeros((24, 31), bool), G_dev, 2)


# ---- the scripts ------------------------------------------------------------------------------------------------------------
def test_both_scripts_print_the_same_ap(tmp_path, capsys):
    """infer_irn --ins_eval 1 (from the device seg_map, label-map kernel) and python -m muscle_amd.ins_eval on the files it wrote
    (mask kernel) print the same lines.  A two-image tree with synthetic weights; the ground-truth objects are the two
    halves of each image.  A listed image without a prediction file is named on stderr; a missing object PNG is an error."""
    import PIL.Image
    from muscle_amd import infer_irn as cli, ins_eval, synth
    H, W = 45, 58
    keys = (3, 11)
    root = tmp_path / "VOC2012"
    for d in ("JPEGImages", "SegmentationClass", "SegmentationObject"):
        (root / d).mkdir(parents=True)
    (tmp_path / "cam").mkdir()
    names = ["2007_000001", "2007_000002"]
    for i, name in enumerate(names):
        img = (255 * synth.uniform(3 + i, "ins_script_img", (H, W, 3))).astype(np.uint8)
        PIL.Image.fromarray(img).save(root / "JPEGImages" / f"{name}.jpg", quality=92)
        np.save(tmp_path / "cam" / f"{name}.npy", synth.irn_cam_dict(H, W, 2 + i, classes=keys))
        obj = np.zeros((H, W), np.uint8)
        obj[:, : W // 2], obj[:, W // 2:], obj[0] = 1, 2, 255
        cls_png = np.where(obj == 1, keys[0] + 1, keys[1] + 1).astype(np.uint8)
        cls_png[0] = 255
        PIL.Image.fromarray(obj).save(root / "SegmentationObject" / f"{name}.png")
        PIL.Image.fromarray(cls_png).save(root / "SegmentationClass" / f"{name}.png")
    torch.save({k: torch.from_numpy(np.asarray(v)) for k, v in synth.irn_state_dict(1).items()}, tmp_path / "irn.pth")
    (tmp_path / "list.txt").write_text("".join(n + "\n" for n in names))
    base = ["--irn_weights_name", str(tmp_path / "irn.pth"), "--cam_dir", str(tmp_path / "cam"), "--voc12_root", str(root),
            "--infer_list", str(tmp_path / "list.txt"), "--walk", "stencil", "--sem_seg_out_dir", str(tmp_path / "sem"),
            "--ins_refine_iters", "50"]
    with pytest.raises(SystemExit):
        cli.main(base + ["--ins_eval", "1"])                             # refused without --ins_seg_out_dir
    capsys.readouterr()
    assert cli.main(base + ["--ins_seg_out_dir", str(tmp_path / "ins"), "--ins_eval", "1"]) == 0
    out = capsys.readouterr().out
    first = out[out.index("0.25iou: {"):]                                # after the per-image progress lines
    ev_args = ["--voc12_root", str(root), "--list", str(tmp_path / "list.txt"), "--ins_seg_dir", str(tmp_path / "ins")]
    assert ins_eval.main(ev_args) == 0
    second = capsys.readouterr().out
    print(second)
    assert first == second and [second.count(f"{t}iou: {{'ap': ") for t in T4] == [1, 1, 1, 1]
    ev = ins_eval.InsSegEval(DEV)
    for name in names:
        ev.add(np.load(tmp_path / "ins" / f"{name}.npy", allow_pickle=True).item(), *ins_eval.read_gt_pngs(str(root), name))
    assert "\n".join(ev.lines()) + "\n" == second
    r = ev.result()
    assert ev.n_pos[list(keys)].tolist() == [2, 2] and not np.isnan(r["ap"][:, list(keys)]).any() and not np.isnan(r["map"]).any()
    # a missing prediction file: named, and the image counts as having no predictions; a missing object PNG: an error naming it
    (tmp_path / "ins" / f"{names[1]}.npy").unlink()
    assert ins_eval.main(ev_args) == 0
    assert f"{names[1]}.npy" in capsys.readouterr().err
    (root / "SegmentationObject" / f"{names[0]}.png").unlink()
    with pytest.raises(FileNotFoundError, match=names[0]):
        ins_eval.main(ev_args)
