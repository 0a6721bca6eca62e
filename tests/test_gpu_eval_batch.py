"""GPU tests of the batched evaluation sweeps: mx_rapid_eval_lr against the per-image chain mx_upsample_to_nchw -> cam_maxnorm ->
mx_eval_confusion (integer tables, exact), mx_seg_infer_batch against mx_seg_infer (bit-equal), the sweep drivers at batch 3
against batch 1 on a synthetic VOC tree of three sizes, and the property all of it rests on: sample b of an eval-mode
batch-8 forward equals the batch-1 forward of that sample bit for bit."""
import os

import numpy as np
import pytest
import torch

DEV = "cuda:0"
K = 21


def _chain_table(sgc, lwb, gt, thresholds, H, W):
    """The existing per-image chain on the same low-resolution maps."""
    from muscle_amd import ops
    from muscle_amd.evaluation import RapidEval
    from muscle_amd.phase2 import cam_maxnorm
    ev = RapidEval(DEV, thresholds=thresholds)
    pred = cam_maxnorm(ops.upsample_to_nchw(sgc, K, H, W))
    for b in range(sgc.shape[0]):
        ev.add_prediction(pred[b], lwb[b], gt[b])
    return ev.counts


def _rapid_lr(sgc, lwb, gt, thresholds, H, W, counts=None):
    from muscle_amd._lib import call, lib, ptr, stream
    B, h, w, lds = sgc.shape
    thr = torch.tensor(thresholds, dtype=torch.float32, device=DEV)
    if counts is None:
        counts = torch.zeros(len(thresholds), K, 3, dtype=torch.int64, device=DEV)
    n = int(lib().mx_rapid_eval_lr_ws(B, K))
    assert n == B * K * 2 * 4
    ws = torch.empty(n, dtype=torch.uint8, device=DEV)
    call("mx_rapid_eval_lr", ptr(sgc), ptr(lwb), ptr(gt), ptr(thr), len(thresholds), B, h, w, lds, K, H, W, ptr(counts), ptr(ws), n,
         stream())
    return counts


def _kernel_case(h, w, H, W):
    g = torch.Generator().manual_seed(100 * h + W)
    sgc = torch.randn(3, h, w, 24, generator=g)
    sgc[..., 5] = -sgc[..., 5].abs() - 0.1               # all negative: min = max = 0, the +1e-6 denominators
    sgc[..., 7] = sgc[..., 3]                            # identical maps: an exact tie, channel 3 must win
    lab = torch.zeros(3, K)
    lab[:, 0] = 1
    lab[0, [3, 5, 7, 9, 12]] = 1
    lab[1, [1, 3, 7, 20]] = 1                            # image 2: no foreground label at all
    gt = torch.randint(0, K, (3, H, W), generator=g).to(torch.uint8)      # class 19 is in gt and never predicted (label 0)
    gt[torch.rand(3, H, W, generator=g) < 0.1] = 255
    assert (gt == 255).any() and (gt == 19).any()
    return sgc.to(DEV).contiguous(), lab.to(DEV).contiguous(), gt.to(DEV).contiguous()


@pytest.mark.gpu
@pytest.mark.parametrize("shape", [(5, 4, 37, 29), (1, 1, 16, 16)], ids=["5x4to37x29", "1x1to16x16"])
@pytest.mark.parametrize("nt", [16, 1])
def test_rapid_eval_lr_equals_the_per_image_chain(shape, nt):
    from muscle_amd.evaluation import RAPID_THRESHOLDS
    h, w, H, W = shape
    thresholds = RAPID_THRESHOLDS if nt == 16 else (0.3,)
    assert len(thresholds) == nt
    sgc, lwb, gt = _kernel_case(h, w, H, W)
    want = _chain_table(sgc, lwb, gt, thresholds, H, W)
    got = _rapid_lr(sgc, lwb, gt, thresholds, H, W)
    valid = int((gt < 255).sum())
    assert int(want[0, :, 1].sum()) == valid             # every counted pixel has one prediction: nothing is excluded
    assert got.dtype == torch.int64 and torch.equal(got, want)
    if nt == 16 and h > 1:
        assert int(want[0, 3, 1]) > 0 and int(want[:, 7, 1].sum()) == 0       # the tie went to the first channel
        assert int(want[:, 5, 1].sum()) == 0 and int(want[0, 19, 2]) > 0      # the all-negative channel; the absent class
    again = _rapid_lr(sgc, lwb, gt, thresholds, H, W)
    assert torch.equal(again, got)                       # the same bits run to run
    twice = _rapid_lr(sgc, lwb, gt, thresholds, H, W, counts=got.clone())
    assert torch.equal(twice, 2 * want)                  # accumulated across calls


@pytest.mark.gpu
def test_rapid_eval_lr_refuses_bad_arguments():
    from muscle_amd._lib import lib, ptr
    L = lib()
    sgc, lwb, gt = _kernel_case(5, 4, 37, 29)
    thr = torch.tensor([0.3], device=DEV)
    counts = torch.zeros(1, K, 3, dtype=torch.int64, device=DEV)
    ws = torch.empty(3 * K * 8, dtype=torch.uint8, device=DEV)
    good = [ptr(sgc), ptr(lwb), ptr(gt), ptr(thr), 1, 3, 5, 4, 24, K, 37, 29, ptr(counts), ptr(ws), ws.numel(), None]
    for i, v in ((0, None), (12, None), (13, None), (4, 0), (4, 65), (5, 0), (8, 22), (9, 25), (9, 1), (14, ws.numel() - 1)):
        args = list(good)
        args[i] = v
        assert L.mx_rapid_eval_lr(*args) < 0, (i, v)
    assert L.mx_rapid_eval_lr_ws(0, K) == 0
    assert int(counts.abs().sum()) == 0


@pytest.mark.gpu
def test_seg_infer_batch_equals_seg_infer_per_image():
    from muscle_amd._lib import call, ptr, stream
    B, h, w, lds, H, W, Hs, Ws = 3, 5, 4, 24, 37, 29, 40, 32
    g = torch.Generator().manual_seed(3)
    logits = (3 * torch.randn(B, h, w, lds, generator=g)).to(DEV).contiguous()
    cls = torch.rand(B, K, generator=g).to(DEV).contiguous()
    gt = torch.randint(0, K, (B, H, W), generator=g).to(torch.uint8)
    gt[torch.rand(B, H, W, generator=g) < 0.1] = 255
    gt = gt.to(DEV).contiguous()
    for c in (None, cls):
        preds, probs = [], []
        want_counts = torch.zeros(K, 3, dtype=torch.int64, device=DEV)
        for b in range(B):
            tab = torch.tensor([[logits[b].data_ptr(), h, w, Hs, Ws, 0, 0, 0]], dtype=torch.int64).to(DEV)
            p, q = torch.empty(H, W, dtype=torch.uint8, device=DEV), torch.empty(K, H, W, device=DEV)
            call("mx_seg_infer", ptr(tab), 1, lds, K, H, W, ptr(c[b]) if c is not None else None, ptr(p), ptr(q), stream())
            call("mx_seg_confusion", ptr(p), ptr(gt[b]), K, H, W, ptr(want_counts), stream())
            preds.append(p)
            probs.append(q)
        tab = torch.tensor([[logits[b].data_ptr(), h, w, Hs, Ws, 0, b, 0] for b in range(B)], dtype=torch.int64).to(DEV)
        pred, prob = torch.empty(B, H, W, dtype=torch.uint8, device=DEV), torch.empty(B, K, H, W, device=DEV)
        counts = torch.zeros(K, 3, dtype=torch.int64, device=DEV)
        call("mx_seg_infer_batch", ptr(tab), B, B, lds, K, H, W, ptr(c), ptr(pred), ptr(prob), ptr(gt), ptr(counts), stream())
        assert torch.equal(pred, torch.stack(preds)) and torch.equal(prob, torch.stack(probs))
        assert torch.equal(counts, want_counts) and int(counts[:, 2].sum()) == int((gt < 255).sum())
        pred2 = torch.empty_like(pred)                    # without prob, gt and counts
        call("mx_seg_infer_batch", ptr(tab), B, B, lds, K, H, W, ptr(c), ptr(pred2), None, None, None, stream())
        assert torch.equal(pred2, pred)
    # two rows per image (a pass and its flip), interleaved: per image the rows are summed in table order
    rows = [[logits[b].data_ptr(), h, w, Hs, Ws, f, b, 0] for f in (0, 1) for b in range(B)]
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    pred, prob = torch.empty(B, H, W, dtype=torch.uint8, device=DEV), torch.empty(B, K, H, W, device=DEV)
    call("mx_seg_infer_batch", ptr(tab), 2 * B, B, lds, K, H, W, None, ptr(pred), ptr(prob), None, None, stream())
    for b in range(B):
        t1 = torch.tensor([[logits[b].data_ptr(), h, w, Hs, Ws, f, 0, 0] for f in (0, 1)], dtype=torch.int64).to(DEV)
        p, q = torch.empty(H, W, dtype=torch.uint8, device=DEV), torch.empty(K, H, W, device=DEV)
        call("mx_seg_infer", ptr(t1), 2, lds, K, H, W, None, ptr(p), ptr(q), stream())
        assert torch.equal(pred[b], p) and torch.equal(prob[b], q)


# ---- model level ------------------------------------------------------------------------------------------------------------
SIZES = ((40, 56), (56, 40), (40, 56), (33, 47), (56, 40), (40, 56))      # three of 40x56, two of 56x40, one of 33x47


def _tree(tmp_path):
    import PIL.Image
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    g = np.random.default_rng(11)
    names, labels = [f"2008_{i:06d}" for i in range(len(SIZES))], {}
    for i, (nm, (h, w)) in enumerate(zip(names, SIZES)):
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        img = np.stack([127 + 100 * np.sin(xx / (4.0 + c) + i) * np.cos(yy / (6.0 - c)) for c in range(3)], -1) + g.normal(0, 12, (h, w, 3))
        PIL.Image.fromarray(np.clip(img, 0, 255).astype(np.uint8), "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=92)
        cls = [2 * i + 1, 2 * i + 2]
        lab = np.zeros(20, np.float32)
        lab[cls] = 1
        labels[nm] = lab
        gt = g.choice([0, cls[0] + 1, cls[1] + 1, 255], size=(h // 4 + 1, w // 4 + 1), p=[0.5, 0.25, 0.2, 0.05]).astype(np.uint8)
        PIL.Image.fromarray(np.ascontiguousarray(np.kron(gt, np.ones((4, 4), np.uint8))[:h, :w]), "L").save(
            root / "SegmentationClass" / f"{nm}.png")
    return str(root), names, labels


@pytest.fixture(scope="module")
def enc_model():
    import muscle_amd
    from muscle_amd import synth
    from muscle_amd.arch import net_cfg
    # the seeded synthetic weights of the parity tests (default initialisation gives an all-background prediction)
    sd = {k: torch.from_numpy(np.asarray(v)) for k, v in synth.synth_state_dict(net_cfg("efficientnet-b0", False), 31).items()}
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=False)
    model.load_state_dict(sd, strict=False)
    return model.to(DEV).eval()


@pytest.fixture(scope="module")
def dec_model():
    import muscle_amd
    torch.manual_seed(1)
    return muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=True, mode="dec").to(DEV).eval()


@pytest.mark.gpu
@pytest.mark.both_arith
def test_eval_forward_is_per_sample_up_to_batch_8(enc_model, dec_model):
    from muscle_amd.evaluation import MAX_EVAL_BATCH
    assert MAX_EVAL_BATCH == 8
    x = torch.randn(8, 3, 40, 56, generator=torch.Generator().manual_seed(9)).to(DEV)
    with torch.no_grad():
        cam, sgc, _, _ = enc_model(x, cam="cam_lr")
        seg = dec_model(x, cam="seg_lr")
        cam, sgc, seg = cam.clone(), sgc.clone(), seg.clone()
        for b in range(8):
            c1, s1, _, _ = enc_model(x[b:b + 1], cam="cam_lr")
            assert torch.equal(c1[0], cam[b]) and torch.equal(s1[0], sgc[b]), b
            assert torch.equal(dec_model(x[b:b + 1], cam="seg_lr")[0], seg[b]), b
        for B in (3, 5):
            c, s, _, _ = enc_model(x[:B], cam="cam_lr")
            assert torch.equal(c, cam[:B]) and torch.equal(s, sgc[:B]), B
            assert torch.equal(dec_model(x[:B], cam="seg_lr"), seg[:B]), B


@pytest.mark.gpu
@pytest.mark.both_arith
def test_rapid_eval_sweep_batch_equals_per_image(tmp_path, enc_model):
    from muscle_amd.evaluation import rapid_eval_sweep
    root, names, labels = _tree(tmp_path)
    dev = torch.device(DEV)
    one = rapid_eval_sweep(enc_model, names, root, labels, dev, batch=1)
    three = rapid_eval_sweep(enc_model, names, root, labels, dev, batch=3)        # a full batch, a remainder of two, a singleton
    assert int(one.counts[:, :, 1].sum()) > 0 and int((one.counts[:, 1:, 1] > 0).sum()) > 0
    assert torch.equal(three.counts, one.counts)
    assert three.best() == one.best()
    with pytest.raises(ValueError, match="batch"):
        rapid_eval_sweep(enc_model, names, root, labels, dev, batch=9)


@pytest.mark.gpu
@pytest.mark.both_arith
@pytest.mark.parametrize("variant", ["plain", "cls", "crf"])
def test_seg_validation_batch_equals_per_image(tmp_path, dec_model, variant):
    import PIL.Image
    from muscle_amd.evaluation import SegValidation, validate_seg
    root, names, _ = _tree(tmp_path)
    dev = torch.device(DEV)
    names = [n for n, s in zip(names, SIZES) if s == (40, 56)]
    cls_dir = None
    if variant == "cls":
        cls_dir = tmp_path / "cls"
        cls_dir.mkdir()
        for i, nm in enumerate(names):
            np.save(cls_dir / f"{nm}.npy", np.linspace(0.2, 1.0, 21, dtype=np.float32)[None] ** (i + 1))
        cls_dir = str(cls_dir)
    a = SegValidation(dev, 21, cls_dir=cls_dir, crf=variant == "crf")
    b = SegValidation(dev, 21, cls_dir=cls_dir, crf=variant == "crf")
    imgs = [PIL.Image.open(os.path.join(root, "JPEGImages", n + ".jpg")).convert("RGB") for n in names]
    gts = [np.array(PIL.Image.open(os.path.join(root, "SegmentationClass", n + ".png"))) for n in names]
    with torch.no_grad():
        want = torch.stack([a.add(dec_model, im, gt, n) for im, gt, n in zip(imgs, gts, names)])
        got = b.add_batch(dec_model, imgs, gts, names)
    assert got.dtype == torch.uint8 and torch.equal(got, want)
    assert int(a.table.counts.sum()) > 0 and torch.equal(b.table.counts, a.table.counts)
    if variant != "crf":
        assert validate_seg(dec_model, names, root, dev, 21, cls_dir=cls_dir, batch=3) == a.miou() == \
            validate_seg(dec_model, names, root, dev, 21, cls_dir=cls_dir, batch=1)
