"""GPU parity of segmentation inference (infer_seg.py:88-133 without the CRF): the eval-mode decoder on ragged sizes with
non-trivial BatchNorm running statistics against the oracle, the low-resolution cam='seg_lr' forward, the fused
post-processing kernel mx_seg_infer against fp64 / numpy restatements of the script, end to end against the oracle, the
device confusion table against src/evaluation.py's arithmetic, run-to-run bits and the command-line entry point.
As in test_gpu_infer.py, cv2.resize is restated as F.interpolate(align_corners=False) (same sampling rule)."""
import os
import re
import subprocess
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from muscle_amd import synth
from muscle_amd.arch import net_cfg
from test_gpu_model import close

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


def _sd(name, seed):
    """Synthetic decoder weights whose BatchNorm running statistics are NOT the identity (synth writes mean 0 / var 1)."""
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


def _img_list(seed, H, W, scales):
    """VOC12ClsDatasetMSF order: for each scale the resized image, then its horizontal flip."""
    base = T(synth.normal(seed, "img", (1, 3, H, W)).astype(np.float32))
    out = []
    for s in scales:
        im = F.interpolate(base, size=(int(round(H * s)), int(round(W * s))), mode="bilinear", align_corners=False)
        out += [im, torch.flip(im, dims=[3])]
    return out


def _post(seg_maps, H, W, cls=None):
    """infer_seg.py:104-125 in fp64 on per-pass logits [1,K,Hs,Ws]: softmax, resize to (H, W), un-flip, mean, class scale."""
    acc = []
    for n, s in enumerate(seg_maps):
        p = F.interpolate(torch.softmax(s.double(), dim=1), size=(H, W), mode="bilinear", align_corners=False)[0]
        acc.append(torch.flip(p, dims=[2]) if n % 2 else p)
    m = torch.stack(acc).mean(0)
    if cls is not None:
        m[1:] *= torch.as_tensor(np.asarray(cls, dtype=np.float64))[1:, None, None]
    return m


def _upsample_lr(lr, K, Hs, Ws):
    """cam='seg' from cam='seg_lr' in fp64: [h,w,lds] -> [1,K,Hs,Ws] (align_corners=True, MuSCLe.py:244-245)."""
    return F.interpolate(lr[..., :K].permute(2, 0, 1)[None].double().cpu(), size=(Hs, Ws), mode="bilinear", align_corners=True)


def _margin(m):
    top = torch.topk(m, 2, dim=0).values
    return (top[0] - top[1]).numpy()


def _run_kernel(maps, meta, K, H, W, cls=None, prob=True, lds=24):
    """maps: device tensors [h,w,lds] (one per pass); meta: (Hs, Ws, flip) per pass."""
    from muscle_amd._lib import call, ptr, stream
    rows = [[m.data_ptr(), m.shape[0], m.shape[1], hs, ws, fl, 0, 0] for m, (hs, ws, fl) in zip(maps, meta)]
    tab = torch.tensor(rows, dtype=torch.int64).to(DEV)
    c = None if cls is None else torch.as_tensor(np.asarray(cls, dtype=np.float32)).to(DEV)
    pred = torch.full((H, W), 77, dtype=torch.uint8, device=DEV)
    pr = torch.full((K, H, W), -1.0, device=DEV) if prob else None
    call("mx_seg_infer", ptr(tab), len(rows), lds, K, H, W, ptr(c), ptr(pred), ptr(pr), stream())
    torch.cuda.synchronize()
    return pred.cpu(), (pr.cpu() if prob else None)


_ORACLE = {}


@pytest.mark.both_arith
@pytest.mark.parametrize("name", ["efficientnet-b0", "efficientnet-b3"])
def test_eval_decoder_vs_oracle(name):
    """Eval-mode cam='seg' (BiFPN BatchNorms on running statistics, level joins at odd sizes) against the oracle, with and
    without the folded backbone BatchNorms; cam='seg_lr' upsampled is cam='seg''s seg_map bit for bit."""
    from oracle import mcl_oracle as O
    from muscle_amd import ops
    seed, H, W = 41, 75, 100
    sd = _sd(name, seed)
    model = _model(name, sd)
    imgs = _img_list(seed, H, W, (0.5, 1.0, 1.25))[::2]                # 38x50, 75x100, 94x125
    for x in imgs:
        key = (name, tuple(x.shape))
        if key not in _ORACLE:
            net = O.OracleDecNet(name, sd).eval()
            with torch.no_grad():
                _ORACLE[key] = net.forward_seg(x)
        rseg, rft = _ORACLE[key]
        Hs, Ws = x.shape[2:]
        for fold in (False, True):
            model.train()
            model.eval()
            if fold:
                model.fold_eval_bn()
            with torch.no_grad():
                seg, ft = model(x.to(DEV), cam="seg")
                lr = model(x.to(DEV), cam="seg_lr")
            assert seg.shape == rseg.shape and ft.shape == rft.shape
            close(seg, rseg, 5e-4)
            close(ft, rft, 5e-4)
            assert lr.shape[0] == 1 and lr.shape[3] == 24 and lr.shape[1] < Hs and lr.shape[2] < Ws
            assert torch.equal(ops.upsample_to_nchw(lr, 21, Hs, Ws), seg)


def test_seg_lr_is_no_grad_only():
    model = _model("efficientnet-b0", _sd("efficientnet-b0", 3))
    x = torch.zeros(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="no_grad"):
        model(x, cam="seg_lr")


def _b0_passes(seed, H, W, scales):
    model = _model("efficientnet-b0", _sd("efficientnet-b0", seed))
    imgs = [im.to(DEV) for im in _img_list(seed, H, W, scales)]
    with torch.no_grad():
        lrs = [model(im, cam="seg_lr")[0] for im in imgs]
    return model, imgs, lrs


@pytest.mark.both_arith
def test_fused_post_vs_fp64():
    """mx_seg_infer on the model's own low-res logits against the fp64 restatement, scales below and above 1."""
    seed, H, W, K = 43, 75, 100, 21
    _, imgs, lrs = _b0_passes(seed, H, W, (0.5, 1.0, 1.75))
    meta = [(im.shape[2], im.shape[3], n % 2) for n, im in enumerate(imgs)]
    cls = np.concatenate([[1.0], np.linspace(0.05, 1.0, K - 1)]).astype(np.float32)
    for c in (None, cls):
        pred, prob = _run_kernel(lrs, meta, K, H, W, cls=c)
        ref = _post([_upsample_lr(lr, K, hs, ws) for lr, (hs, ws, _) in zip(lrs, meta)], H, W, c)
        err = float((prob.double() - ref).abs().max())
        assert err <= 2e-6, err
        ok = _margin(ref) > 1e-5
        assert ok.mean() > 0.9
        assert np.array_equal(pred.numpy()[ok], ref.argmax(0).numpy()[ok])


@pytest.mark.both_arith
def test_infer_seg_end_to_end_vs_oracle():
    from oracle import mcl_oracle as O
    from muscle_amd.infer import infer_seg
    seed, H, W, K = 47, 75, 100, 21
    sd = _sd("efficientnet-b0", seed)
    model = _model("efficientnet-b0", sd)
    imgs = _img_list(seed, H, W, (0.5, 1.0))
    net = O.OracleDecNet("efficientnet-b0", sd).eval()
    with torch.no_grad():
        ref = _post([net.forward_seg(im)[0] for im in imgs], H, W)
    pred, prob = infer_seg(model, [im.to(DEV) for im in imgs], H, W, return_prob=True)
    assert pred.dtype == torch.uint8 and pred.shape == (H, W) and prob.shape == (K, H, W)
    err = float((prob.cpu().double() - ref).abs().max())
    assert err <= 1e-3, err
    p, r = pred.cpu().numpy(), ref.argmax(0).numpy()
    bad = p != r
    assert bad.mean() <= 5e-3, bad.mean()
    assert np.all(_margin(ref)[bad] <= 1e-3)


def test_cls_label_scale():
    """Channel 0 is untouched, the others are scaled after the mean; a class scaled to 0 never wins, unless every channel
    is 0 (np.argmax's tie rule: 0)."""
    K, H, W = 21, 23, 31
    g = torch.Generator().manual_seed(5)
    maps = [(torch.randn(7, 9, 24, generator=g) * 3).to(DEV), (torch.randn(7, 9, 24, generator=g) * 3).to(DEV)]
    meta = [(20, 26, 0), (20, 26, 1)]
    cls = np.zeros(K, np.float32)
    cls[0] = 0.0                      # entry 0 is not used
    cls[[3, 8, 15]] = [1.0, 0.5, 2.0]
    p0, r0 = _run_kernel(maps, meta, K, H, W)
    p1, r1 = _run_kernel(maps, meta, K, H, W, cls=cls)
    assert torch.equal(r1[0], r0[0])
    for k in range(1, K):
        assert torch.equal(r1[k], r0[k] * float(cls[k])), k
    assert set(np.unique(p1.numpy())) <= {0, 3, 8, 15}
    assert np.array_equal(p1.numpy(), r1.numpy().argmax(0))
    # background probability underflows to exactly 0 and every other class is scaled to 0: all channels 0 -> class 0
    m = torch.zeros(3, 4, 24)
    m[..., 0] = -300.0
    m[..., 1:21] = torch.randn(3, 4, 20, generator=g)
    p2, r2 = _run_kernel([m.to(DEV)], [(6, 8, 0)], K, 5, 7, cls=np.zeros(K, np.float32))
    assert float(r2.abs().max()) == 0.0 and int(p2.max()) == 0


def _np_coords(n_out, n_in, align_corners):
    d = np.arange(n_out, dtype=np.float64)
    if align_corners:
        s = d * ((n_in - 1) / (n_out - 1) if n_out > 1 else 0.0)
    else:
        s = np.maximum((d + 0.5) * n_in / n_out - 0.5, 0.0)
    i0 = np.minimum(np.floor(s).astype(np.int64), n_in - 1)
    i1 = np.minimum(i0 + 1, n_in - 1)
    return i0, i1, s - i0


def _np_resize(a, Ho, Wo, align_corners):          # a [h,w,K]
    y0, y1, wy = _np_coords(Ho, a.shape[0], align_corners)
    x0, x1, wx = _np_coords(Wo, a.shape[1], align_corners)
    r = a[y0] * (1 - wy)[:, None, None] + a[y1] * wy[:, None, None]
    return r[:, x0] * (1 - wx)[None, :, None] + r[:, x1] * wx[None, :, None]


def _np_seg(maps, meta, K, H, W, cls=None):
    """infer_seg.py:101-133 in numpy fp64 (explicit align_corners / cv2 half-pixel coordinates)."""
    acc = []
    for n, (m, (hs, ws, fl)) in enumerate(zip(maps, meta)):
        up = _np_resize(m[..., :K].astype(np.float64), hs, ws, True)
        e = np.exp(up - up.max(-1, keepdims=True))
        v = _np_resize(e / e.sum(-1, keepdims=True), H, W, False)
        acc.append(v[:, ::-1] if fl else v)
    m = np.mean(acc, axis=0).transpose(2, 0, 1)
    if cls is not None:
        m[1:] = m[1:] * np.asarray(cls, np.float64)[1:, None, None]
    return m


@pytest.mark.parametrize("case", ["1x1", "down_up", "w1_flip", "single", "k3_lds4"])
def test_kernel_edge_cases(case):
    g = np.random.default_rng(11)
    K, lds = 21, 24
    if case == "1x1":
        shapes, meta, H, W = [(1, 1)], [(5, 7, 1)], 9, 6
    elif case == "down_up":                                  # Hs, Ws below and above H, W (scales 0.5 and 1.75)
        shapes, meta, H, W = [(3, 4), (3, 4), (8, 11), (8, 11)], [(10, 13, 0), (10, 13, 1), (35, 46, 0), (35, 46, 1)], 20, 26
    elif case == "w1_flip":
        shapes, meta, H, W = [(2, 1), (2, 1)], [(9, 1, 0), (9, 1, 1)], 17, 1
    elif case == "single":
        shapes, meta, H, W = [(4, 5)], [(30, 38, 0)], 25, 31
    else:
        K, lds = 3, 4
        shapes, meta, H, W = [(5, 6), (5, 6)], [(11, 13, 0), (11, 13, 1)], 12, 15
    maps = [(g.standard_normal((h, w, lds)) * 4).astype(np.float32) for h, w in shapes]
    pred, prob = _run_kernel([T(m).to(DEV) for m in maps], meta, K, H, W, lds=lds)
    ref = _np_seg(maps, meta, K, H, W)
    assert prob.shape == (K, H, W)
    assert float(np.abs(prob.double().numpy() - ref).max()) <= 2e-6
    ok = (np.sort(ref, 0)[-1] - np.sort(ref, 0)[-2]) > 1e-5
    assert np.array_equal(pred.numpy()[ok], ref.argmax(0)[ok])
    p2, _ = _run_kernel([T(m).to(DEV) for m in maps], meta, K, H, W, lds=lds, prob=False)   # prob = NULL: pred alone
    assert torch.equal(p2, pred)


def test_kernel_bad_args():
    from muscle_amd._lib import lib, ptr
    L = lib()
    m = torch.zeros(2, 2, 24, device=DEV)
    tab = torch.tensor([[m.data_ptr(), 2, 2, 4, 4, 0, 0, 0]], dtype=torch.int64, device=DEV)
    pred = torch.empty(4, 4, dtype=torch.uint8, device=DEV)
    for args in ((None, 1, 24, 21, 4, 4), (ptr(tab), 0, 24, 21, 4, 4), (ptr(tab), -1, 24, 21, 4, 4),
                 (ptr(tab), 1, 20, 21, 4, 4), (ptr(tab), 1, 22, 21, 4, 4), (ptr(tab), 1, 28, 25, 4, 4),
                 (ptr(tab), 1, 24, 0, 4, 4), (ptr(tab), 1, 24, 21, 0, 4)):
        assert L.mx_seg_infer(*args, None, ptr(pred), None, None) < 0, args
        assert b"seg_infer" in L.mx_last_error()
    assert L.mx_seg_infer(ptr(tab), 1, 24, 21, 4, 4, None, None, None, None) < 0      # pred NULL
    counts = torch.zeros(21, 3, dtype=torch.int64, device=DEV)
    assert L.mx_seg_confusion(None, ptr(pred), 21, 4, 4, ptr(counts), None) < 0
    assert L.mx_seg_confusion(ptr(pred), ptr(pred), 21, 4, 4, None, None) < 0
    assert L.mx_seg_confusion(ptr(pred), ptr(pred), 0, 4, 4, ptr(counts), None) < 0
    assert b"seg_confusion" in L.mx_last_error()
    torch.cuda.synchronize()


def _np_counts(pred, gt, num_cls):
    """src/evaluation.py:36-50 for one image."""
    cal = gt < 255
    mask = (pred == gt) * cal
    return np.array([[np.sum((gt == i) * mask), np.sum((pred == i) * cal), np.sum((gt == i) * cal)] for i in range(num_cls)],
                    dtype=np.int64)


def test_seg_eval_vs_numpy():
    from muscle_amd.evaluation import SegEval, miou_loglist
    g = np.random.default_rng(3)
    ev = SegEval(DEV)
    ref = np.zeros((21, 3), np.int64)
    for H, W in ((37, 53), (120, 91), (1, 1)):
        pred = g.choice([0, 2, 5, 9, 15, 22], size=(H, W)).astype(np.uint8)       # 22 >= K: never counted (as :41-42)
        gt = g.choice([0, 2, 5, 7, 15, 255], size=(H, W)).astype(np.uint8)        # 255 = ignore; 7 only in gt
        ev.add(T(pred).to(DEV), T(gt).to(DEV))
        ref += _np_counts(pred, gt, 21)
    got = ev.counts.cpu().numpy()
    assert np.array_equal(got, ref)
    assert got[3].sum() == 0 and got[7, 1] == 0
    a, b = ev.loglist(), miou_loglist(ref)
    assert a == b and set(a) >= {"background", "tvmonitor", "mIoU"}
    big = np.full((600, 700), 4, np.uint8)                                          # more pixels than one workgroup pass
    ev2 = SegEval(DEV)
    ev2.add(T(big).to(DEV), T(big).to(DEV))
    assert ev2.counts.cpu().numpy()[4].tolist() == [600 * 700] * 3


def test_infer_seg_bits_repeat():
    from muscle_amd.infer import infer_seg
    seed, H, W = 53, 75, 100
    model = _model("efficientnet-b0", _sd("efficientnet-b0", seed))
    imgs = [im.to(DEV) for im in _img_list(seed, H, W, (0.5, 1.0, 1.25))]
    cls = np.linspace(0.0, 1.0, 21).astype(np.float32)
    a = infer_seg(model, imgs, H, W, cls_label=cls, return_prob=True)
    b = infer_seg(model, imgs, H, W, cls_label=cls, return_prob=True)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    c, none = infer_seg(model, imgs, H, W, cls_label=cls)
    assert none is None and torch.equal(c, a[0])


def test_cli_end_to_end(tmp_path):
    """python -m muscle_amd.infer_seg in a fresh process on a VOC-shaped tree: one PNG per image equal to infer_seg's
    pred, and the printed mIoU equal to SegEval's."""
    import PIL.Image
    from muscle_amd.data import MSFStager
    from muscle_amd.evaluation import SegEval
    from muscle_amd.infer import infer_seg
    from muscle_amd.infer_seg import DEFAULT_SCALES
    seed = 59
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    (root / "SegmentationClass").mkdir()
    g = np.random.default_rng(seed)
    names = ["2007_000032", "2007_000039"]
    sizes = [(72, 96), (80, 72)]                     # smallest pass 36 x 36: above the backbone's static-padding minimum
    for nm, (h, w) in zip(names, sizes):
        PIL.Image.fromarray(g.integers(0, 256, (h, w, 3), dtype=np.uint8), "RGB").save(root / "JPEGImages" / f"{nm}.jpg")
        PIL.Image.fromarray(g.choice([0, 1, 4, 255], size=(h, w)).astype(np.uint8), "L").save(root / "SegmentationClass" / f"{nm}.png")
    (tmp_path / "val.txt").write_text("".join(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n" for nm in names))
    np.save(tmp_path / "cls_labels.npy", {nm: np.eye(20, dtype=np.float32)[i] for i, nm in enumerate(names)})
    sd = _sd("efficientnet-b0", seed)
    torch.save({k: T(v) for k, v in sd.items()}, tmp_path / "w.pth")
    out = tmp_path / "seg"
    env = dict(os.environ, PYTHONPATH=ROOT)
    r = subprocess.run([sys.executable, "-m", "muscle_amd.infer_seg", "--weights", str(tmp_path / "w.pth"),
                        "--infer_list", str(tmp_path / "val.txt"), "--voc12_root", str(root), "--num_classes", "21",
                        "--bifpn", "3", "--pretrained", "b0", "--out_seg", str(out), "--gt_dir", str(root / "SegmentationClass")],
                       cwd=str(tmp_path), env=env, capture_output=True, text=True, timeout=170)
    assert r.returncode == 0, r.stderr[-3000:]
    model = _model("efficientnet-b0", sd)
    stager = MSFStager(DEV)
    ev = SegEval(DEV)
    for nm in names:
        img = PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB")
        pred, _ = infer_seg(model, stager(img, DEFAULT_SCALES), img.size[1], img.size[0])
        png = PIL.Image.open(out / f"{nm}.png")
        assert png.mode == "L"
        assert np.array_equal(np.array(png), pred.cpu().numpy()), nm
        ev.add(pred, T(np.array(PIL.Image.open(root / "SegmentationClass" / f"{nm}.png"))).to(DEV))
    m = re.search(r"mIoU:\s*([0-9.]+)%", r.stdout)
    assert m, r.stdout[-2000:]
    assert m.group(1) == "%.3f" % ev.loglist()["mIoU"]
