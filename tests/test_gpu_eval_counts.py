"""The counting rule of src/evaluation.py:27-52, through every entry point that counts a (TP, P, T) table: mx_seg_confusion,
mx_seg_infer_batch (gt / counts), mx_eval_confusion, mx_rapid_eval_lr, mx_camdict_confusion, mx_irn_sweep_confusion.  Each is fed
the same kinds of image and must equal tests/eval_counts_ref.py integer for integer: K in {2, 5, 21, 24}; 1 and 64 thresholds;
images of 1x1, 1x257 (one pixel past a workgroup) and 37x53; ground truth below K, in K..254 (counts towards P only) and 255
(skipped); an image that is all 255 (the table must not move); values that tie with a threshold exactly; a second call (the
table accumulates).  Where an entry point forms its own prediction (mx_seg_infer_batch, mx_rapid_eval_lr,
mx_irn_sweep_confusion) the expected prediction comes from the per-image chain the other tests pin (mx_seg_infer;
mx_upsample_to_nchw -> mx_maxnorm; mx_irn_finish) and is counted with the restatement."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_counts_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SHAPES = ((1, 1), (1, 257), (37, 53))
CASES = pytest.mark.parametrize("K,shape", [(K, s) for K in (2, 5, 21, 24) for s in SHAPES],
                                ids=lambda v: "%dx%d" % v if isinstance(v, tuple) else "K%d" % v)
NTS = (1, 64)


def thresholds(nt):
    """fp32, ascending; the 64 hold 0 and 1 exactly."""
    return np.array([0.25], np.float32) if nt == 1 else (np.arange(64) / 63.0).astype(np.float32)


def pool(nt, negatives=False):
    """Values a map is drawn from: the thresholds themselves (exact ties) and a few others."""
    extra = [0.0, 0.125, 0.25, 0.5, 0.75, 1.0] + ([-0.25, -1.0] if negatives else [])
    return np.concatenate([thresholds(nt), np.array(extra, np.float32)])


def make_gts(K, H, W, rng):
    """uint8 [B,H,W]; every kind of value occurs, and the last image is all 255."""
    if H * W == 1:
        return np.array([K - 1, 0, K, 254, 255], np.uint8).reshape(5, 1, 1)
    gt = rng.randint(0, K, size=(H, W)).astype(np.uint8)
    kind = rng.rand(H, W)
    gt[kind < 0.1] = 255
    gt[(kind >= 0.1) & (kind < 0.2)] = K
    gt[(kind >= 0.2) & (kind < 0.3)] = 254
    gt.flat[:5] = (K - 1, 0, K, 254, 255)
    return np.stack([gt, np.full((H, W), 255, np.uint8)])


def dev(a, dtype=None):
    t = torch.from_numpy(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).to(DEV).contiguous()


def verify(run, want):
    """run(table, idx) adds the images idx to the device table; want[b]: image b's table (numpy)."""
    B, total = len(want), np.sum(want, axis=0)
    assert total[..., 1].sum() > 0 and total[..., 2].sum() > 0 and not want[-1].any()
    table = torch.zeros(*total.shape, dtype=torch.int64, device=DEV)
    run(table, list(range(B)))
    got = table.cpu().numpy()
    assert np.array_equal(got, total), np.argwhere(got != total)[:8]
    run(table, [B - 1])                                              # the image that is all 255
    assert np.array_equal(table.cpu().numpy(), total)
    run(table, list(range(B)))                                       # a second call accumulates
    assert np.array_equal(table.cpu().numpy(), 2 * total)


@CASES
def test_seg_confusion(K, shape):
    from muscle_amd._lib import call, ptr, stream
    H, W = shape
    rng = np.random.RandomState(K * 1000 + W)
    gts = make_gts(K, H, W, rng)
    pred = rng.randint(0, K + 2, size=gts.shape).astype(np.uint8)    # K and K + 1 are predicted too: they count nowhere
    if H * W == 1:
        pred[:, 0, 0] = (K - 1, 1, 0, K, 0)
    d_pred, d_gt = dev(pred), dev(gts)

    def run(table, idx):
        for b in idx:
            call("mx_seg_confusion", ptr(d_pred[b]), ptr(d_gt[b]), K, H, W, ptr(table), stream())

    verify(run, [R.counts(pred[b], gts[b], K) for b in range(len(gts))])


@CASES
def test_seg_infer_batch(K, shape):
    from muscle_amd._lib import call, ptr, stream
    H, W = shape
    h, w, lds, Hs, Ws = 3, 4, 24, 8, 12
    rng = np.random.RandomState(K * 1000 + W + 1)
    gts = make_gts(K, H, W, rng)
    B = len(gts)
    logits = dev((3 * rng.randn(B, h, w, lds)).astype(np.float32))
    d_gt = dev(gts)
    want = []
    for b in range(B):                                               # the per-image launch's prediction
        tab = torch.tensor([[logits[b].data_ptr(), h, w, Hs, Ws, 0, 0, 0]], dtype=torch.int64).to(DEV)
        p = torch.empty(H, W, dtype=torch.uint8, device=DEV)
        call("mx_seg_infer", ptr(tab), 1, lds, K, H, W, None, ptr(p), None, stream())
        want.append(R.counts(p.cpu().numpy(), gts[b], K))

    def run(table, idx):
        tab = torch.tensor([[logits[b].data_ptr(), h, w, Hs, Ws, 0, i, 0] for i, b in enumerate(idx)], dtype=torch.int64).to(DEV)
        pred = torch.empty(len(idx), H, W, dtype=torch.uint8, device=DEV)
        g = d_gt[idx].contiguous()
        call("mx_seg_infer_batch", ptr(tab), len(idx), len(idx), lds, K, H, W, None, ptr(pred), None, ptr(g), ptr(table), stream())
        torch.cuda.synchronize()                                     # tab, pred and g live until the launch has run

    verify(run, want)


@CASES
def test_eval_confusion(K, shape):
    from muscle_amd._lib import call, ptr, stream
    H, W = shape
    rng = np.random.RandomState(K * 1000 + W + 2)
    gts = make_gts(K, H, W, rng)
    B = len(gts)
    label = (rng.rand(B, K) < 0.6).astype(np.float32)
    label[:, 0] = 1
    label[:, 1] = 1
    d_gt, d_label = dev(gts), dev(label)
    for nt in NTS:
        thr = thresholds(nt)
        pred = rng.choice(pool(nt), size=(B, K, H, W)).astype(np.float32)
        half = pred.astype(np.float16).astype(np.float32)
        assert H * W == 1 or any((half[:, 1:] == t).any() for t in thr)          # a value ties with a threshold
        d_pred, d_thr = dev(pred), dev(thr)

        def run(table, idx):
            for b in idx:
                call("mx_eval_confusion", ptr(d_pred[b]), ptr(d_label[b]), ptr(d_gt[b]), ptr(d_thr), nt, K, H, W, ptr(table), stream())

        verify(run, [R.curve_counts(R.half_dict(pred[b], label[b]), gts[b], thr, K) for b in range(B)])


@CASES
def test_rapid_eval_lr(K, shape):
    from muscle_amd import ops
    from muscle_amd._lib import call, lib, ptr, stream
    from muscle_amd.phase2 import cam_maxnorm
    H, W = shape
    h, w, lds = 3, 4, 24
    rng = np.random.RandomState(K * 1000 + W + 3)
    gts = make_gts(K, H, W, rng)
    B = len(gts)
    sgc = rng.randn(B, h, w, lds).astype(np.float32)
    if K > 3:
        sgc[..., 2] = -np.abs(sgc[..., 2]) - 0.1                     # all negative: min = max = 0
    label = (rng.rand(B, K) < 0.6).astype(np.float32)
    label[:, 0] = 1
    label[:, 1] = 1
    label[0, 2:] = 0                                                 # image 0: one live channel, whose minimum normalises to 0
    d_sgc, d_label, d_gt = dev(sgc), dev(label), dev(gts)
    vals = cam_maxnorm(ops.upsample_to_nchw(d_sgc, K, H, W)).cpu().numpy()          # the per-image chain's values
    for nt in NTS:
        thr = thresholds(nt)
        d_thr = dev(thr)

        def run(table, idx):
            n = int(lib().mx_rapid_eval_lr_ws(len(idx), K))
            ws = torch.empty(n, dtype=torch.uint8, device=DEV)
            s, l, g = d_sgc[idx].contiguous(), d_label[idx].contiguous(), d_gt[idx].contiguous()      # held until the launches have run
            call("mx_rapid_eval_lr", ptr(s), ptr(l), ptr(g), ptr(d_thr), nt, len(idx), h, w, lds, K, H, W, ptr(table), ptr(ws), n, stream())
            torch.cuda.synchronize()

        dicts = [R.half_dict(vals[b], label[b]) for b in range(B)]
        if nt == 64 and H * W > 1:
            assert (np.stack(list(dicts[0].values())).max(axis=0) == 0).any()         # ties with the threshold 0
        verify(run, [R.curve_counts(dicts[b], gts[b], thr, K) for b in range(B)])


@CASES
def test_camdict_confusion(K, shape):
    from muscle_amd._lib import call, ptr, stream
    H, W = shape
    rng = np.random.RandomState(K * 1000 + W + 4)
    gts = make_gts(K, H, W, rng)
    B = len(gts)
    keys = sorted(rng.choice(K - 1, size=max(1, (K - 1) // 2), replace=False).tolist())
    d_gt, d_keys = dev(gts), dev(np.array(keys, np.int32))
    for nt in NTS:
        thr = thresholds(nt)
        maps = rng.choice(pool(nt, negatives=True), size=(B, len(keys), H, W)).astype(np.float32)
        low = rng.rand(B, 1, H, W) < 0.15                            # pixels where every map is negative
        low[1] |= H * W == 1
        maps = np.where(low, maps - 2, maps).astype(np.float32)
        best = maps.max(axis=1)
        assert (best < 0).any() and (H * W == 1 or any((best == t).any() for t in thr))
        d_maps, d_thr = dev(maps), dev(thr)

        def run(table, idx):
            for b in idx:
                call("mx_camdict_confusion", ptr(d_maps[b]), ptr(d_keys), len(keys), ptr(d_gt[b]), ptr(d_thr), nt, K, H, W, ptr(table),
                     stream())

        verify(run, [R.curve_counts({k: maps[b, j] for j, k in enumerate(keys)}, gts[b], thr, K) for b in range(B)])


@CASES
def test_irn_sweep_confusion(K, shape):
    from muscle_amd import indexing
    from muscle_amd._lib import call, ptr, stream
    H, W = shape
    h, w, E, C = (H + 3) // 4, (W + 3) // 4, 2, K - 1
    rng = np.random.RandomState(K * 1000 + W + 5)
    gts = make_gts(K, H, W, rng)
    B = len(gts)
    keys = sorted(rng.choice(C, size=max(1, C // 2), replace=False).tolist())
    rw = (rng.rand(B, E, len(keys), h, w) + 0.01).astype(np.float32)
    if w > 3:
        rw[..., :3, :3] = 0                                          # interpolated inside the block: exactly 0, a tie with the threshold 0
    d_gt, d_keys, d_rw = dev(gts), dev(np.array(keys, np.int32)), dev(rw)
    full = torch.zeros(B, E, C, 1, h, w, device=DEV)                 # the stack mx_irn_finish takes: absent channels are zero maps
    full[:, :, keys, 0] = d_rw
    vmax = np.zeros((B, E), np.int32)
    for b in range(B):
        for e in range(E):
            _, cs = indexing.finish_semseg(full[b, e], H, W, 0.3, soft_output="compact")
            vmax[b, e] = np.float32(cs.vmax).view(np.int32)
    d_vmax = dev(vmax)
    for nt in NTS:
        thr = thresholds(nt)
        d_thr = dev(thr)
        want = []
        for b in range(B):
            labels = torch.stack([indexing.finish_semseg(full[b, e], H, W, float(t)) for e in range(E) for t in thr]).cpu().numpy()
            want.append(np.stack([R.counts(lab, gts[b], K) for lab in labels]).reshape(E, nt, K, 3))
        if nt == 64 and w > 3:
            assert want[0][0, 0, 0, 1] > 0                           # background at the threshold 0: the pixels whose value is 0

        def run(table, idx):
            for b in idx:
                call("mx_irn_sweep_confusion", ptr(d_rw[b]), E, len(keys), ptr(d_keys), h, w, ptr(d_gt[b]), H, W, ptr(d_thr), nt, K,
                     ptr(d_vmax[b]), ptr(table), stream())

        verify(run, want)
