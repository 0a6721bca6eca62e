"""GPU tests of muscle_amd.irn_sweep: the snapshots of mx_irn_walk_snap against separate walks (bits), and the table of
mx_irn_sweep_confusion against the chain it stands for (integers):

    down  = ops.resize_planar_halfpixel(cam_stack(cam_dict, H, W), h, w)
    rw    = indexing.propagate_to_edge(down, edge, beta=b, exp_times=e, radius=5, method="stencil")
    label = indexing.finish_semseg(rw, H, W, t)
    mx_seg_confusion(label, gt)

No tolerance appears anywhere.  The fields are built so that both ties are really exercised: low-resolution pixel (0,0) has
edge 0 and its three neighbours edge 1, which cuts every path out of it, so its state never changes; the first map is 2 there
and below 1 elsewhere, so that pixel is the maximum, its up-sampling weights are 0 and v = mx / mx = 1 exactly; and a 3x3 block
of edge 1 keeps its state at 0, so the pixels interpolated inside it have v = 0 exactly.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_sweep_ref as SR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")
K = 21
BETAS, EXP_TIMES, THRESHOLDS = (4, 10), (0, 2, 4), (0.0, 0.2, 0.35, 0.9, 1.0)
KEY_ORDER = (17, 3, 9, 0, 19, 12)                                     # inserted unsorted


def make_gt(H, W, seed):
    from muscle_amd import synth
    yy, xx = np.mgrid[0:H, 0:W]
    gt = ((yy // 8 * ((W + 7) // 8) + xx // 8) % K).astype(np.uint8)                  # classes 0..20 in 8x8 blocks
    gt[synth.uniform(seed, "sw_ignore", (H, W)) < 0.05] = 255
    return gt


def make_field(h, w, H, W, nkeys, seed=5):
    """(edge [1,h,w] fp32, cam_dict, gt): see the module docstring for the construction."""
    from muscle_amd import synth
    edge = (synth.uniform(seed, "sw_edge", (1, h, w)) ** 3).astype(np.float32)
    edge[0, 0, 0] = 0.0
    edge[0, 0, 1] = edge[0, 1, 0] = edge[0, 1, 1] = 1.0
    edge[0, 0:3, 3:6] = 1.0
    cams = {}
    for i, k in enumerate(KEY_ORDER[:nkeys]):
        m = (0.9 * synth.uniform(seed, f"sw_cam:{k}", (H, W))).astype(np.float32)
        if i == 0:
            m[:4, :4] = 2.0
        cams[k] = m
    return edge, cams, make_gt(H, W, seed)


def chain_counts(edge, cams, gt, H, W, betas=BETAS, exp_times=EXP_TIMES, thresholds=THRESHOLDS):
    """The defining chain, one grid point at a time -> int64 [B,E,T,K,3] (numpy)."""
    from muscle_amd import indexing, ops
    from muscle_amd._lib import call, ptr, stream
    from muscle_amd.irn import cam_stack
    e = torch.as_tensor(edge).to(DEV)
    g = torch.as_tensor(gt).to(DEV)
    h, w = e.shape[-2:]
    down = ops.resize_planar_halfpixel(cam_stack(cams, H, W, DEV), h, w)
    out = torch.zeros(len(betas), len(exp_times), len(thresholds), K, 3, dtype=torch.int64, device=DEV)
    for bi, b in enumerate(betas):
        for ei, et in enumerate(exp_times):
            rw = indexing.propagate_to_edge(down, e, beta=b, exp_times=et, radius=5, method="stencil")
            for ti, t in enumerate(thresholds):
                label = indexing.finish_semseg(rw, H, W, t)
                call("mx_seg_confusion", ptr(label), ptr(g), K, H, W, ptr(out[bi, ei, ti]), stream())
    return out.cpu().numpy()


def sweep_counts(edge, cams, gt, H, W, betas=BETAS, exp_times=EXP_TIMES, thresholds=THRESHOLDS):
    from muscle_amd.irn_sweep import IrnSweep
    sw = IrnSweep(DEV, betas, exp_times, thresholds)
    sw.add_field(torch.as_tensor(edge).to(DEV), cams, torch.as_tensor(gt).to(DEV), H, W)
    return sw


def kept_walk(edge, cams, H, W, beta, et):
    """(keys, rw of the kept channels [Kp,h,w] numpy, vmax fp32) from the existing entry points."""
    from muscle_amd import indexing, ops
    from muscle_amd.irn import cam_stack
    e = torch.as_tensor(edge).to(DEV)
    h, w = e.shape[-2:]
    down = ops.resize_planar_halfpixel(cam_stack(cams, H, W, DEV), h, w)
    rw = indexing.propagate_to_edge(down, e, beta=beta, exp_times=et, radius=5, method="stencil")
    _, cs = indexing.finish_semseg(rw, H, W, 0.3, soft_output="compact")
    keys = sorted(cams)
    return keys, rw.reshape(-1, h, w)[keys].cpu().numpy(), cs.vmax


# ---- 1. snapshots are bit-equal to separate walks ---------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,C,radius,exact_edges", [(19, 23, 3, 5, False), (19, 23, 3, 5, True), (3, 7, 1, 5, False),
                                                      (1, 9, 2, 5, False), (16, 12, 3, 3, False)],
                         ids=["19x23-two-workgroups", "19x23-edges-0-and-1", "3x7-most-taps-outside", "1x9-one-row", "16x12-radius3"])
def test_snapshots_equal_separate_walks_bit_for_bit(h, w, C, radius, exact_edges):
    from muscle_amd import indexing, synth
    x = torch.from_numpy(synth.uniform(7, "irn_x", (1, C, h, w)).astype(np.float32)).to(DEV)
    edge = torch.from_numpy(synth.uniform(7, "irn_e", (1, h, w)).astype(np.float32)) ** 3
    if exact_edges:
        edge[0, 0, 0] = 1.0
        edge[0, 18, 22] = 0.0
        edge[0, 4, 5:9] = 1.0
        edge[0, 2:6, 15] = 0.0
    edge = edge.to(DEV)
    single = {}
    for ets in ((0,), (0, 1, 3), (2, 5), (8,)):
        multi = indexing.propagate_to_edge_multi(x, edge, radius, 10, ets)
        assert tuple(multi.shape) == (len(ets), C, 1, h, w) and multi.dtype == torch.float32
        for i, et in enumerate(ets):
            if et not in single:
                single[et] = indexing.propagate_to_edge(x, edge, radius=radius, beta=10, exp_times=et, method="stencil")
            assert torch.equal(multi[i], single[et]), (ets, et)
        assert torch.equal(indexing.propagate_to_edge_multi(x, edge, radius, 10, ets), multi), ets          # the same bits again


# ---- 2. counts equal the chain ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,H,W,nkeys,nt", [(9, 13, 35, 50, 3, 5), (19, 23, 76, 92, 6, 5), (3, 7, 9, 25, 1, 5), (9, 13, 35, 50, 6, 64)],
                         ids=["9x13-crop-not-x4-3keys", "19x23-6keys", "3x7-1key", "9x13-64-thresholds"])
def test_counts_equal_the_chain(h, w, H, W, nkeys, nt):
    edge, cams, gt = make_field(h, w, H, W, nkeys)
    thr = THRESHOLDS if nt == 5 else tuple(i / 63 for i in range(64))
    assert thr[0] == 0.0 and thr[-1] == 1.0
    for b in BETAS:                                                   # both ties exist: v == 1 (the maximum) and v == 0
        keys, rw, vmax = kept_walk(edge, cams, H, W, b, EXP_TIMES[-1])
        best = SR.soft_values(rw, H, W, vmax).max(axis=0)
        assert vmax == rw[keys.index(KEY_ORDER[0]), 0, 0] and (best == 1).any() and (best == 0).any() and best[0, 0] == 1
    want = chain_counts(edge, cams, gt, H, W, thresholds=thr)
    sw = sweep_counts(edge, cams, gt, H, W, thresholds=thr)
    got = sw.counts()
    assert got.dtype == np.int64 and got.shape == (2, 3, nt, K, 3)
    assert np.array_equal(got, want)
    assert want[..., 1:, 1].sum() > 0 and (want[:, :, -1, 1:, 1] == 0).all()          # foreground is predicted, and none at t = 1
    m = sw.mious()
    assert m.shape == (2, 3, nt) and abs(m[1, 2, 1] - sw.loglist(1, 2, 1)["mIoU"]) == 0
    assert sw.all_zero_names() == []


def test_counts_equal_the_numpy_restatement():
    """The smallest shape, against tests/irn_sweep_ref.py on the walk results and maxima of the existing entry points."""
    h, w, H, W = 3, 7, 9, 25
    edge, cams, gt = make_field(h, w, H, W, 3)
    got = sweep_counts(edge, cams, gt, H, W).counts()
    for bi, b in enumerate(BETAS):
        for ei, et in enumerate(EXP_TIMES):
            keys, rw, vmax = kept_walk(edge, cams, H, W, b, et)
            want = SR.sweep_counts(rw[None], keys, [vmax], gt, H, W, THRESHOLDS, K)[0]
            assert np.array_equal(got[bi, ei], want), (b, et)


# ---- 3. accumulation --------------------------------------------------------------------------------------------------------
def test_three_images_of_different_sizes_accumulate():
    from muscle_amd.irn_sweep import IrnSweep
    sw = IrnSweep(DEV, BETAS, EXP_TIMES, THRESHOLDS)
    total = 0
    for i, (h, w, H, W, nkeys) in enumerate([(9, 13, 35, 50, 3), (3, 7, 9, 25, 1), (19, 23, 76, 92, 6)]):
        edge, cams, gt = make_field(h, w, H, W, nkeys, seed=11 + i)
        sw.add_field(torch.as_tensor(edge).to(DEV), cams, gt, H, W)               # gt as a numpy array: uploaded
        total = total + chain_counts(edge, cams, gt, H, W)
    assert np.array_equal(sw.counts(), total)
    miou, beta, et, t = sw.best()
    m = sw.mious()
    assert miou == m.max() and (beta, et, t) == tuple(v[i] for v, i in zip((sw.betas, sw.exp_times, sw.thresholds),
                                                                           np.unravel_index(np.argmax(m), m.shape)))


# ---- 4. degenerate inputs ---------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["empty-dict", "all-zero-maps", "edge-one-everywhere"])
def test_degenerate_inputs_predict_background(kind):
    h, w, H, W = 9, 13, 35, 50
    edge, cams, gt = make_field(h, w, H, W, 3)
    if kind == "empty-dict":
        cams = {}
    elif kind == "all-zero-maps":
        cams = {k: np.zeros_like(v) for k, v in cams.items()}
    else:
        edge = np.ones_like(edge)
    want = chain_counts(edge, cams, gt, H, W)
    from muscle_amd.irn_sweep import IrnSweep
    sw = IrnSweep(DEV, BETAS, EXP_TIMES, THRESHOLDS)
    sw.add_field(torch.as_tensor(edge).to(DEV), cams, torch.as_tensor(gt).to(DEV), H, W, name="img")
    got = sw.counts()
    assert np.array_equal(got, want)
    counted = int((gt < 255).sum())
    assert (got[..., 1:, 1] == 0).all() and (got[..., 0, 1] == counted).all()       # every threshold predicts background
    assert (got[..., 1:, 0] == 0).all() and (got[..., 0, 0] == int((gt == 0).sum())).all()
    assert sw.all_zero_names() == ["img"]
    torch.cuda.synchronize()


# ---- 5. the compact route ---------------------------------------------------------------------------------------------------
def test_compact_route_equals_the_grid_sweep():
    from muscle_amd import indexing, ops
    from muscle_amd.irn import cam_stack
    from muscle_amd.irn_sweep import IrnSweep
    from muscle_amd.softlabel import CompactSoft
    h, w, H, W = 9, 13, 35, 50
    edge, cams, gt = make_field(h, w, H, W, 3)
    full = sweep_counts(edge, cams, gt, H, W).counts()
    e = torch.as_tensor(edge).to(DEV)
    down = ops.resize_planar_halfpixel(cam_stack(cams, H, W, DEV), h, w)
    for bi, ei in ((1, 1), (0, 2)):
        rw = indexing.propagate_to_edge(down, e, beta=BETAS[bi], exp_times=EXP_TIMES[ei], radius=5, method="stencil")
        _, cs = indexing.finish_semseg(rw, H, W, 0.35, soft_output="compact")
        assert list(cs.keys) == sorted(cams)
        sw = IrnSweep.thresholds_only(DEV, THRESHOLDS)
        sw.add_compact(cs, gt)
        assert np.array_equal(sw.counts(), full[bi:bi + 1, ei:ei + 1])
    _, zero = indexing.finish_semseg(torch.zeros(20, 1, h, w, device=DEV), H, W, 0.35, soft_output="compact")
    assert zero.vmax == 0
    for cs in (zero, CompactSoft(np.array([3], np.uint8), np.ones((1, h, w), np.float32), (H, W), 0.0, 0.35, 21), None):
        sw = IrnSweep.thresholds_only(DEV, THRESHOLDS)
        sw.add_compact(cs, gt)
        got = sw.counts()
        assert (got[..., 1:, 1] == 0).all() and (got[..., 0, 1] == int((gt < 255).sum())).all()
        assert np.array_equal(got[0, 0], SR.counts_from_values(np.zeros((0, H, W), np.float32), [], gt, THRESHOLDS, K))
    with pytest.raises(ValueError):
        IrnSweep(DEV, BETAS, EXP_TIMES, THRESHOLDS).add_compact(zero, gt)          # B = E = 1 only


def test_script_from_soft(tmp_path, capsys):
    """python -m muscle_amd.irn_sweep --from_soft: one image with a compact label, one without (an all-zero walk result): the table
    it writes equals add_field's at that (beta, exp_times) plus an all-background image, and the best threshold is printed."""
    import PIL.Image
    from muscle_amd import indexing, ops
    from muscle_amd.irn import cam_stack
    from muscle_amd.irn_sweep import IrnSweep, main
    from muscle_amd.softlabel import save_compact
    h, w, H, W = 9, 13, 35, 50
    edge, cams, gt = make_field(h, w, H, W, 3)
    e = torch.as_tensor(edge).to(DEV)
    rw = indexing.propagate_to_edge(ops.resize_planar_halfpixel(cam_stack(cams, H, W, DEV), h, w), e, beta=10, exp_times=2, radius=5,
                                    method="stencil")
    _, cs = indexing.finish_semseg(rw, H, W, 0.35, soft_output="compact")
    (tmp_path / "soft").mkdir()
    (tmp_path / "SegmentationClass").mkdir()
    save_compact(str(tmp_path / "soft" / "a.npz"), cs)
    for n in "ab":
        PIL.Image.fromarray(gt).save(tmp_path / "SegmentationClass" / f"{n}.png")
    (tmp_path / "list.txt").write_text("a\nb\n")
    thr = [str(t) for t in THRESHOLDS]
    assert main(["--from_soft", str(tmp_path / "soft"), "--voc12_root", str(tmp_path), "--infer_list", str(tmp_path / "list.txt"),
                 "--thresholds"] + thr + ["--out_table", str(tmp_path / "t.npy"), "--logfile", str(tmp_path / "log.txt")]) == 0
    want = IrnSweep(DEV, (10,), (2,), THRESHOLDS)
    want.add_field(e, cams, gt, H, W)
    want.add_field(e, {}, gt, H, W)
    assert np.array_equal(np.load(tmp_path / "t.npy"), want.counts())
    out, err = capsys.readouterr()
    assert "best: --sem_seg_bg_thres " + "%g" % want.best()[3] in out and "b: the walk result is all zero" in err
    assert "mIoU" in (tmp_path / "log.txt").read_text()


# ---- 6. the interface -------------------------------------------------------------------------------------------------------
def test_interface():
    from muscle_amd import indexing, ops
    from muscle_amd._lib import MuscleHipError, call, ptr, stream
    from muscle_amd.irn_sweep import IrnSweep
    h, w, H, W = 9, 13, 35, 50
    edge, cams, gt = make_field(h, w, H, W, 3)
    e = torch.as_tensor(edge).to(DEV).reshape(h, w)
    x = torch.rand(2, h, w, device=DEV)
    table = indexing._path_table(5, e.device)
    Wt, cs = ops.irn_walk_weights(e, table, 5, 10)
    for snap in ((1, 4, 2), (2, 2), (0, 1), (1, 4097), tuple(range(1, 15))):      # not ascending, duplicate, < 1, > 4096, ns = 14
        with pytest.raises(MuscleHipError, match="irn_walk_snap"):
            ops.irn_walk_snap(x, e, Wt, cs, table, 5, snap)
    rw = torch.zeros(2, 3, h, w, device=DEV)
    keys = torch.tensor([0, 3, 9], dtype=torch.int32, device=DEV)
    g = torch.as_tensor(gt).to(DEV)
    thr = torch.linspace(0, 1, 65, device=DEV)
    vmax = torch.zeros(2, dtype=torch.int32, device=DEV)
    counts = torch.zeros(2, 5, K, 3, dtype=torch.int64, device=DEV)

    def sweep(rw=rw, nt=5, Kc=K, Hc=H, counts=counts):
        call("mx_irn_sweep_confusion", ptr(rw), 2, 3, ptr(keys), h, w, ptr(g), Hc, W, ptr(thr), nt, Kc, ptr(vmax), ptr(counts), stream())

    for kw in (dict(rw=None), dict(counts=None), dict(nt=65), dict(Kc=25), dict(Hc=4 * h + 1)):
        with pytest.raises(MuscleHipError, match="irn_sweep_confusion"):
            sweep(**kw)
    assert int(counts.sum()) == 0                                               # nothing was launched
    sweep()
    assert int(counts[..., 1].sum()) == 2 * 5 * int((gt < 255).sum())           # a maximum of 0: every pixel predicted once, as background
    assert int(counts[..., 1:, 1].sum()) == 0
    sw = IrnSweep(DEV, BETAS, EXP_TIMES, THRESHOLDS)
    with pytest.raises(MuscleHipError):
        sw.add_field(torch.as_tensor(edge), cams, g, H, W)                      # host edge
    with pytest.raises(MuscleHipError):
        sw.add_field(torch.as_tensor(edge).to(DEV), cams, torch.as_tensor(gt), H, W)      # host gt tensor
    with pytest.raises(MuscleHipError):
        sw.add(None, torch.zeros(2, 3, H, W), cams, g)                          # host image pair
    with pytest.raises(MuscleHipError):
        indexing.propagate_to_edge_multi(torch.zeros(1, 2, h, w), torch.as_tensor(edge), exp_times_list=(0, 1))
    with pytest.raises(ValueError):
        sw.add_field(torch.as_tensor(edge).to(DEV), {20: cams[17]}, g, H, W)    # class key beyond num_cls - 2
    assert int(sw.table.sum()) == 0


# ---- 7. end to end ----------------------------------------------------------------------------------------------------------
def test_sweep_end_to_end_equals_infer_irn_plus_segeval():
    """IrnSweep.add with a randomly initialised EdgeDisplacement on the 64x80 pair of test_infer_irn_stencil_end_to_end: every grid
    point's table equals infer_irn(method="stencil") followed by SegEval."""
    import muscle_amd
    from muscle_amd import synth
    from muscle_amd.evaluation import SegEval
    from muscle_amd.irn import infer_irn
    from muscle_amd.irn_sweep import IrnSweep
    z = np.load(os.path.join(GOLD, "irn_net.npz"))
    crop, H, W, seed = (int(v) for v in z["a_params"])
    sd, x, cam = synth.irn_state_dict(seed), synth.irn_image_pair(H, W, seed), synth.irn_cam_dict(H, W, seed)
    m = muscle_amd.EdgeDisplacement(crop_size=crop)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    pair = torch.from_numpy(x).to(DEV)
    gt = torch.from_numpy(make_gt(H, W, 3)).to(DEV)
    betas, ets, thr = (4, 10), (0, 3), (0.2, 0.35, 0.9)
    sw = IrnSweep(DEV, betas, ets, thr)
    sw.add(m, pair, cam, gt)
    got = sw.counts()
    for bi, b in enumerate(betas):
        for ei, et in enumerate(ets):
            for ti, t in enumerate(thr):
                ev = SegEval(DEV, K)
                ev.add(infer_irn(m, pair, cam, beta=b, exp_times=et, bg_thres=t, method="stencil"), gt)
                assert np.array_equal(got[bi, ei, ti], ev.counts.cpu().numpy()), (b, et, t)
    assert got[..., 1:, 1].sum() > 0
