"""GPU parity of pixel-adaptive mask refinement (muscle_amd.pamr; mx_pamr_affinity / mx_pamr_step / mx_pamr) against the numpy
restatement of its model in pamr_ref.py, and its wiring into infer.infer_seg / infer.infer_cam_fused.

Shapes are the smallest at which the kernels can still go wrong: 5x7 and 1x9 are smaller than every large dilation (both clamps
hit), 37x53 is ragged against the 64 x 4 tile, 65x129 crosses a tile and a wave boundary in both directions.

Tolerance: e32 = max|float32-numpy - fp64| is computed for the same input (what fp32 rounding alone does to the model, reference
arithmetic on the CPU) and the kernel must stay within 4 * e32 + 1e-7 of the fp64 result.  The factor covers the hardware exp and
reciprocal, a few ulp against numpy's, and a different but fixed order of the 9 D-term variance; the ratios observed are printed and
listed in profiles/pamr_bench.txt."""
import functools
import os
import subprocess
import sys

import numpy as np
import pytest
import torch

import pamr_ref as R
from muscle_amd import synth
from muscle_amd.arch import net_cfg

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
T = lambda a: torch.from_numpy(np.ascontiguousarray(a))  # noqa: E731
F_TOL = 4.0
DIL = R.DEFAULT_DILATIONS


def _one_image(kind, H, W, g):
    if kind == "noise":
        return g.integers(0, 256, (H, W, 3), dtype=np.uint8)
    if kind == "ramp":
        y, x = np.mgrid[0:H, 0:W]
        return np.stack([(3 * x + y) % 256, (2 * y + 5) % 256, (x + 2 * y) % 256], axis=-1).astype(np.uint8)
    if kind == "blocks":                                    # 8x8 constant blocks: std = 0 in their interiors at dilation 1
        b = g.integers(0, 256, ((H + 7) // 8, (W + 7) // 8, 3), dtype=np.uint8)
        return np.ascontiguousarray(np.repeat(np.repeat(b, 8, axis=0), 8, axis=1)[:H, :W])
    raise KeyError(kind)


#         name            image     N  C   H   W    dilations
CASES = {"tiny_5x7":     ("noise",  1, 1,  5,  7,   DIL),
         "row_1x9":      ("ramp",   1, 4,  1,  9,   DIL),
         "ragged_37x53": ("blocks", 1, 21, 37, 53,  DIL),
         "blocks_d1":    ("blocks", 1, 4,  37, 53,  (1,)),
         "ramp_d1":      ("ramp",   1, 1,  5,  7,   (1,)),
         "tiles_65x129": ("noise",  1, 25, 65, 129, DIL),         # C = 25: no 24-class cap
         "batch2":       ("noise",  2, 4,  19, 23,  DIL)}         # two different images and masks: batch strides


@functools.lru_cache(maxsize=None)
def _case(name):
    """(img uint8 [N,H,W,3], mask fp32 [N,C,H,W] in [0,1], dilations, w64, out64 after 10 iterations, e32 of w, e32 of out)."""
    kind, N, C, H, W, dil = CASES[name]
    g = np.random.default_rng(sorted(CASES).index(name) + 11)
    img = np.stack([_one_image(kind, H, W, g) for _ in range(N)])
    mask = g.random((N, C, H, W)).astype(np.float32)
    out64, w64 = R.pamr(img, mask, 10, dil)
    out32, w32 = R.pamr(img, mask, 10, dil, dtype=np.float32)
    for a in (img, mask, w64, out64):
        a.setflags(write=False)
    return img, mask, dil, w64, out64, float(np.abs(w32 - w64).max()), float(np.abs(out32 - out64).max())


def _within(tag, got, ref64, e32):
    err = float(np.abs(got.astype(np.float64) - ref64).max())
    print(f"{tag}: max|gpu - fp64| {err:.3e}, e32 {e32:.3e}, ratio {err / e32 if e32 > 0 else float('nan'):.2f}")
    assert np.isfinite(got).all()
    assert err <= F_TOL * e32 + 1e-7, (tag, err, e32)


@pytest.mark.parametrize("name", sorted(CASES))
def test_affinity_against_fp64(name):
    from muscle_amd import pamr_affinity
    img, _, dil, w64, _, e32, _ = _case(name)
    w = pamr_affinity(T(img).to(DEV), dil)
    assert w.shape == w64.shape and w.dtype == torch.float32 and w.is_cuda
    _within(f"{name} w", w.cpu().numpy(), w64, e32)
    assert float((w.sum(dim=1) - 1).abs().max()) <= 1e-5 and float(w.min()) >= 0
    # the two image layouts holding the same integer values: the same bits; a second run: the same bits
    planar = T(img.transpose(0, 3, 1, 2)).float().to(DEV)
    assert torch.equal(pamr_affinity(planar, dil), w)
    assert torch.equal(pamr_affinity(T(img).to(DEV), dil), w)
    if img.shape[0] == 1:                                   # unbatched inputs; a numpy image is uploaded
        assert torch.equal(pamr_affinity(img[0], dil), w[0]) and torch.equal(pamr_affinity(planar[0], dil), w[0])


@pytest.mark.parametrize("name", sorted(CASES))
def test_pamr_against_fp64(name):
    from muscle_amd import PAMR, pamr_affinity, pamr_apply
    img, mask, dil, _, out64, _, e32 = _case(name)
    m = T(mask).to(DEV)
    keep = m.clone()
    pamr = PAMR(10, dil)
    out = pamr(T(img).to(DEV), m)
    assert out.shape == m.shape and out.dtype == torch.float32 and out.is_cuda
    _within(f"{name} out", out.cpu().numpy(), out64, e32)
    assert torch.equal(m, keep)                              # mask is untouched
    lo, hi = float(mask.min()), float(mask.max())
    assert lo * (1 - 1e-5) <= float(out.min()) and float(out.max()) <= hi * (1 + 1e-5)
    assert torch.equal(pamr(T(img).to(DEV), m), out)         # two runs, the same bits
    # mx_pamr = mx_pamr_affinity + num_iter x mx_pamr_step, bit for bit
    assert torch.equal(pamr_apply(pamr_affinity(T(img).to(DEV), dil), m, 10, dil), out)
    assert torch.equal(m, keep)
    if img.shape[0] == 1:
        assert torch.equal(pamr(img[0], m[0]), out[0])       # unbatched, numpy image


@pytest.mark.parametrize("num_iter", [0, 1, 2, 10])
def test_iteration_counts(num_iter):
    """Both parities of the ping-pong; 0 returns the input bits."""
    from muscle_amd import PAMR, pamr_affinity, pamr_apply
    img, mask, dil, _, _, _, _ = _case("ragged_37x53")
    m = T(mask).to(DEV)
    out = PAMR(num_iter, dil)(T(img).to(DEV), m)
    assert out.data_ptr() != m.data_ptr()
    stepwise = pamr_apply(pamr_affinity(T(img).to(DEV), dil), m, num_iter, dil)
    assert torch.equal(out, stepwise) and stepwise.data_ptr() != m.data_ptr()
    if num_iter == 0:
        assert torch.equal(out, m)
        return
    ref64, _ = R.pamr(img, mask, num_iter, dil)
    ref32, _ = R.pamr(img, mask, num_iter, dil, dtype=np.float32)
    _within(f"ragged_37x53 num_iter {num_iter}", out.cpu().numpy(), ref64, float(np.abs(ref32 - ref64).max()))


def test_noncontiguous_mask_and_raw_entries():
    """A non-contiguous mask is made contiguous; the C entries called directly: mx_pamr with the workspace of mx_pamr_ws for an even and
    an odd count lands in `out`, equal to the steps called one by one."""
    import ctypes
    from muscle_amd import PAMR
    from muscle_amd._lib import call, lib, ptr, stream
    img, mask, dil, _, _, _, _ = _case("batch2")
    N, C, H, W = mask.shape
    im = T(img).to(DEV)
    m = T(mask).to(DEV)
    nc = T(mask.transpose(0, 1, 3, 2)).to(DEV).transpose(2, 3)
    assert not nc.is_contiguous()
    want = PAMR(3, dil)(im, m)
    assert torch.equal(PAMR(3, dil)(im, nc), want)
    d = (ctypes.c_int * len(dil))(*dil)
    nbytes = lib().mx_pamr_ws(N, C, H, W, len(dil))
    assert nbytes >= (N * 8 * len(dil) * H * W + N * C * H * W) * 4
    ws = torch.empty(nbytes // 4, dtype=torch.float32, device=DEV)
    w = torch.empty(N, 8 * len(dil), H, W, device=DEV)
    call("mx_pamr_affinity", ptr(im), 0, N, H, W, d, len(dil), ptr(w), stream())
    for it in (2, 3):
        out = torch.full_like(m, -1.0)
        call("mx_pamr", ptr(im), 0, ptr(m), ptr(out), N, C, H, W, d, len(dil), it, ptr(ws), nbytes, stream())
        a, b = m, None
        for _ in range(it):
            b = torch.empty_like(m)
            call("mx_pamr_step", ptr(w), ptr(a), ptr(b), N, C, H, W, d, len(dil), stream())
            a = b
        assert torch.equal(out, a), it
    assert torch.equal(out, want) and torch.equal(m, T(mask).to(DEV))


def test_constant_mask_and_constant_image():
    from muscle_amd import PAMR, pamr_affinity
    img, mask, dil, _, _, _, _ = _case("tiles_65x129")
    const = torch.full((1, 3, 65, 129), 0.375, device=DEV)
    const[0, 1] = 0.0
    const[0, 2] = 1.0
    out = PAMR(10, dil)(T(img).to(DEV), const)
    assert float((out - const).abs().max()) <= 1e-6          # a convex combination of equal values
    flat = np.full((33, 70, 3), 77, np.uint8)
    w = pamr_affinity(flat, dil)
    assert torch.equal(w, torch.full_like(w, 1.0 / 48))      # std = 0: every a_p is 0
    bimg, _, _, _, _, _, _ = _case("blocks_d1")
    wb = pamr_affinity(bimg[0], (1,))
    inner = torch.stack([wb[:, by * 8 + 1:by * 8 + 7, bx * 8 + 1:bx * 8 + 7] for by in range(4) for bx in range(6)])
    assert torch.equal(inner, torch.full_like(inner, 0.125))


def test_planar_argmax_first_maximum_wins():
    from muscle_amd.pamr import planar_argmax
    g = np.random.default_rng(5)
    m = g.integers(0, 4, (2, 25, 37, 53)).astype(np.float32)          # many ties
    pred = planar_argmax(T(m).to(DEV))
    assert pred.dtype == torch.uint8 and np.array_equal(pred.cpu().numpy(), m.argmax(1).astype(np.uint8))
    assert np.array_equal(planar_argmax(T(m[1]).to(DEV)).cpu().numpy(), m[1].argmax(0).astype(np.uint8))


# ---- the wiring into inference -----------------------------------------------------------------------------------------------------
def _dec_sd(name, seed):
    """Synthetic decoder weights with non-identity BatchNorm running statistics (as tests/test_gpu_crf.py builds them)."""
    sd = synth.synth_state_dict(net_cfg(name, True), seed, mode="dec", layers=3)
    rng = np.random.default_rng(seed + 1000)
    for k in sorted(sd):
        if k.endswith("running_mean"):
            sd[k] = rng.normal(0.0, 0.5, sd[k].shape).astype(np.float32)
        elif k.endswith("running_var"):
            sd[k] = rng.uniform(0.5, 2.0, sd[k].shape).astype(np.float32)
    return sd


def _dec_model(name, sd):
    import muscle_amd
    m = muscle_amd.MuSCLe(21, name, layers=3, last_pooling=True, mode="dec")
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return m.to(DEV).eval()


def _photo(seed, H, W):
    """A blocky noisy image."""
    g = np.random.default_rng(seed)
    img = np.zeros((H, W, 3))
    img[:, :W // 3] = [200, 30, 30]
    img[H // 4:3 * H // 4, W // 3:4 * W // 5] = [20, 180, 60]
    img[:, 4 * W // 5:] = [30, 40, 200]
    return np.clip(img + g.normal(0, 12, img.shape), 0, 255).astype(np.uint8)


def test_infer_seg_with_pamr():
    """pamr=None is the call without the argument, bit for bit; with PAMR(2) the map is pamr(img, the plain map) bit for bit and
    pred its first-maximum argmax; together with a CRF it is refused."""
    import PIL.Image as PI
    from muscle_amd import PAMR
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    seed, H, W, K = 61, 72, 96, 21
    model = _dec_model("efficientnet-b0", _dec_sd("efficientnet-b0", seed))
    img = _photo(seed, H, W)
    imgs = MSFStager(DEV)(PI.fromarray(img, "RGB"), (0.5, 1.0))
    pred0, prob0 = infer_seg(model, imgs, H, W, return_prob=True)
    pred0b, prob0b = infer_seg(model, imgs, H, W, return_prob=True, pamr=None, pamr_img=None)
    assert torch.equal(pred0, pred0b) and torch.equal(prob0, prob0b)
    pamr = PAMR(2)
    pred, prob = infer_seg(model, imgs, H, W, return_prob=True, pamr=pamr, pamr_img=img)
    want = pamr(img, prob0)
    assert torch.equal(prob, want)
    assert np.array_equal(pred.cpu().numpy(), want.cpu().numpy().argmax(0).astype(np.uint8)) and pred.dtype == torch.uint8
    assert float((prob.sum(0) - 1).abs().max()) <= 1e-5      # every row of w sums to 1: still a distribution
    assert not torch.equal(prob, prob0)
    pred2, none = infer_seg(model, imgs, H, W, pamr=pamr, pamr_img=T(img).to(DEV))
    assert none is None and torch.equal(pred2, pred)
    with pytest.raises(ValueError, match="one of them"):
        infer_seg(model, imgs, H, W, crf_img=img, pamr=pamr, pamr_img=img)


def test_infer_cam_fused_with_pamr():
    """pamr=None is the call without the argument, bit for bit; with PAMR(2) every map is mx_infer_norm(pamr(img, the plain map)),
    bit for bit, for both maps from one affinity."""
    import muscle_amd
    from muscle_amd import PAMR, infer
    from muscle_amd._lib import call, ptr, stream
    seed, H, W = 31, 75, 100
    sd = synth.synth_state_dict(net_cfg("efficientnet-b0", False), seed)
    model = muscle_amd.MuSCLe(21, "efficientnet-b0", layers=3, last_pooling=False)
    model.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    model = model.to(DEV)
    base = T(synth.normal(seed, "img", (1, 3, H, W)).astype(np.float32))
    imgs = []
    for s in (1.0, 1.5):
        im = torch.nn.functional.interpolate(base, size=(int(round(H * s)), int(round(W * s))), mode="bilinear", align_corners=False)
        imgs += [im.to(DEV), torch.flip(im, dims=[3]).to(DEV)]
    classes = [2, 7, 14]
    label = torch.zeros(1, 20)
    label[0, classes] = 1.0
    img = _photo(seed, H, W)
    cam0, sgc0, score0 = infer.infer_cam_fused(model, imgs, label, H, W)
    cam0b, sgc0b, score0b = infer.infer_cam_fused(model, imgs, label, H, W, pamr=None, pamr_img=None)
    assert torch.equal(score0, score0b)
    assert all(np.array_equal(cam0[k], cam0b[k]) and np.array_equal(sgc0[k], sgc0b[k]) for k in classes)
    pamr = PAMR(2)
    cam, sgc, score = infer.infer_cam_fused(model, imgs, label, H, W, pamr=pamr, pamr_img=img)
    assert torch.equal(score, score0) and sorted(cam) == sorted(sgc) == classes
    for got, plain in ((cam, cam0), (sgc, sgc0)):
        want = pamr(img, T(np.stack([plain[k] for k in classes])).to(DEV))
        call("mx_infer_norm", ptr(want), len(classes), H * W, stream())
        want = want.cpu().numpy()
        for j, k in enumerate(classes):
            assert got[k].dtype == np.float32 and np.array_equal(got[k], want[j]), k
            assert not np.array_equal(got[k], plain[k])
            assert abs(float(got[k].max()) - 1.0) <= 1e-4      # normalised once more: the maximum is 1 again
    only, none, _ = infer.infer_cam_fused(model, imgs, label, H, W, want_sgc=False, pamr=pamr, pamr_img=img)
    assert none == {} and all(np.array_equal(only[k], cam[k]) for k in classes)


def test_cli_infer_seg_pamr(tmp_path):
    """python -m muscle_amd.infer_seg --pamr_iters 2 in a fresh process: the PNG equals infer_seg(pamr=PAMR(2))'s pred."""
    import PIL.Image
    import muscle_amd
    from muscle_amd import PAMR
    from muscle_amd.data import MSFStager
    from muscle_amd.infer import infer_seg
    from muscle_amd.infer_seg import DEFAULT_SCALES
    seed, nm = 67, "2007_000033"
    root = tmp_path / "VOC2012"
    (root / "JPEGImages").mkdir(parents=True)
    PIL.Image.fromarray(_photo(seed, 72, 96), "RGB").save(root / "JPEGImages" / f"{nm}.jpg", quality=95)
    (tmp_path / "val.txt").write_text(f"/JPEGImages/{nm}.jpg /SegmentationClassAug/{nm}.png\n")
    sd = _dec_sd("efficientnet-b0", seed)
    torch.save({k: T(v) for k, v in sd.items()}, tmp_path / "w.pth")
    r = subprocess.run([sys.executable, "-m", "muscle_amd.infer_seg", "--weights", str(tmp_path / "w.pth"), "--infer_list",
                        str(tmp_path / "val.txt"), "--voc12_root", str(root), "--pretrained", "b0", "--out_seg", str(tmp_path / "seg"),
                        "--pamr_iters", "2", "--pamr_dilations", "1", "2", "4"],
                       cwd=str(tmp_path), env=dict(os.environ, PYTHONPATH=ROOT), capture_output=True, text=True, timeout=80)
    assert r.returncode == 0, r.stderr[-3000:]
    before = muscle_amd.get_gemm_mode()
    muscle_amd.set_gemm_mode(1)                               # a fresh process runs the library's default arithmetic
    try:
        model = _dec_model("efficientnet-b0", sd)
        img = PIL.Image.open(root / "JPEGImages" / f"{nm}.jpg").convert("RGB")
        pred, _ = infer_seg(model, MSFStager(DEV)(img, DEFAULT_SCALES), img.size[1], img.size[0], pamr=PAMR(2, (1, 2, 4)),
                            pamr_img=np.asarray(img))
    finally:
        muscle_amd.set_gemm_mode(before)
    assert np.array_equal(np.array(PIL.Image.open(tmp_path / "seg" / f"{nm}.png")), pred.cpu().numpy())
