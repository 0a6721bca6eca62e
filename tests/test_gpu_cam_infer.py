"""GPU tests of the one-launch CAM post-processing (mx_cam_infer, infer.infer_cam_fused): bit equality with the per-pass
path (infer.infer_cam: mx_infer_accum per pass and map over all 20 channels), parity with the CPU oracle, the want_cam /
empty-label switches, the kernel's edge cases and its argument checks."""
import numpy as np
import pytest
import torch

from muscle_amd import synth
from muscle_amd.arch import net_cfg

pytestmark = [pytest.mark.gpu, pytest.mark.both_arith]
DEV = "cuda:0"
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731
CASES = [("efficientnet-b0", 75, 100, (0.5, 1.0, 1.5, 2.0)), ("efficientnet-b3", 64, 48, (1.0, 1.5))]
LABEL_SETS = {1: [11], 3: [2, 7, 14], 20: list(range(20))}


def _build(name, seed):
    import muscle_amd
    cfg = net_cfg(name, False)
    sd = synth.synth_state_dict(cfg, seed)
    m = muscle_amd.MuSCLe(21, name, layers=3, last_pooling=False)
    m.load_state_dict({k: T(v) for k, v in sd.items()}, strict=True)
    return cfg, sd, m.to(DEV)


def _img_list(seed, H, W, scales):
    """VOC12ClsDatasetMSF order: for each scale the resized image, then its horizontal flip."""
    base = T(synth.normal(seed, "img", (1, 3, H, W)).astype(np.float32))
    out = []
    for s in scales:
        hs, ws = int(round(H * s)), int(round(W * s))
        im = torch.nn.functional.interpolate(base, size=(hs, ws), mode="bilinear", align_corners=False)
        out += [im, torch.flip(im, dims=[3])]
    return out


def _label(classes):
    label = torch.zeros(1, 20)
    label[0, classes] = 1.0
    return label


@pytest.mark.parametrize("name,H,W,scales", CASES)
def test_fused_equals_per_pass_path(name, H, W, scales):
    """Same helpers, same order, sum from 0.f: the dicts are np.array_equal to infer_cam's and the scores are equal."""
    from muscle_amd import infer
    _, _, model = _build(name, 31)
    imgs = [im.to(DEV) for im in _img_list(31, H, W, scales)]
    for n, classes in LABEL_SETS.items():
        label = _label(classes)
        rcam, rsgc, rscore = infer.infer_cam(model, imgs, label, H, W)
        gcam, gsgc, gscore = infer.infer_cam_fused(model, imgs, label, H, W)
        assert sorted(gcam) == sorted(gsgc) == sorted(rcam) == classes
        for got, ref in ((gcam, rcam), (gsgc, rsgc)):
            for k in classes:
                assert got[k].dtype == np.float32 and got[k].shape == (H, W)
                ne = int((got[k] != ref[k]).sum())
                print(f"{name} nkeep={n} class {k}: {ne} differing pixels, max |d| {float(np.abs(got[k] - ref[k]).max()):.3e}")
                assert np.array_equal(got[k], ref[k]), (n, k, ne)
        assert torch.equal(gscore, rscore)
        # want_cam=False: the CAM map is neither read nor computed; the SGC dict is the same
        ncam, nsgc, nscore = infer.infer_cam_fused(model, imgs, label, H, W, want_cam=False)
        assert ncam == {} and sorted(nsgc) == classes and all(np.array_equal(nsgc[k], gsgc[k]) for k in classes)
        assert torch.equal(nscore, rscore)
        ocam, osgc, _ = infer.infer_cam_fused(model, imgs, label, H, W, want_sgc=False)
        assert osgc == {} and all(np.array_equal(ocam[k], gcam[k]) for k in classes)


@pytest.mark.parametrize("name,H,W,scales", CASES)
def test_fused_matches_oracle(name, H, W, scales):
    """The comparison of test_gpu_infer.py::test_infer_cam_matches_oracle against O.infer_cam: 1e-3, except pixels that sit
    within fp32 round-off of the channel minimum (the script's `norm[norm < min + 1e-6] = 0` is discontinuous there), whose
    share is at most 5e-3."""
    from oracle import mcl_oracle as O
    from muscle_amd import infer
    seed = 31
    _, sd, model = _build(name, seed)
    imgs = _img_list(seed, H, W, scales)
    label = _label([2, 7, 14])
    ocam, osgc, oscore = O.infer_cam(O.OracleNet(name, sd), imgs, label, H, W)
    gcam, gsgc, gscore = infer.infer_cam_fused(model, [im.to(DEV) for im in imgs], label, H, W)
    assert sorted(gcam) == sorted(ocam) == [2, 7, 14] and sorted(gsgc) == sorted(osgc)
    for d_got, d_ref in ((gcam, ocam), (gsgc, osgc)):
        for k in d_ref:
            a, b = d_got[k], d_ref[k]
            assert a.dtype == np.float32 and a.shape == (H, W)
            bad = np.abs(a - b) > 1e-3
            print(f"{name} class {k}: max |d| {float(np.abs(a - b).max()):.3e}, share beyond 1e-3 {float(bad.mean()):.3e}")
            if bad.any():
                lo = float(b.min())
                flip = bad & (np.maximum(a, b) <= 2e-3) & (np.minimum(a, b) >= lo - 1e-3)
                assert np.array_equal(bad, flip), (k, float(np.abs(a - b).max()))
                assert bad.mean() <= 5e-3, (k, float(bad.mean()))
    assert float((gscore.cpu() - oscore).abs().max()) <= 1e-5


def test_image_without_labels_gives_empty_dicts():
    from muscle_amd import infer
    _, _, model = _build("efficientnet-b0", 5)
    imgs = [im.to(DEV) for im in _img_list(5, 48, 64, (1.0,))]
    cam, sgc, score = infer.infer_cam_fused(model, imgs, torch.zeros(1, 20), 48, 64)
    assert cam == {} and sgc == {} and score.shape == (20,)
    _, _, rscore = infer.infer_cam(model, imgs, torch.zeros(1, 20), 48, 64)
    assert torch.equal(score, rscore)


def test_cam_infer_kernel_edge_cases():
    """As test_gpu_infer.py::test_infer_kernels_edge_cases: flip, a single-pixel low-res map, an all-negative channel
    (normalises to the reference's -1e-6/1e-6 quirk); plus two passes, a keep list that does not start at 0, and one
    output NULL."""
    from muscle_amd._lib import call, ptr, stream
    K, H, W = 21, 9, 7
    cam = torch.full((1, 1, 24), -3.0, device=DEV)
    cam[..., 5] = 2.0
    sgc = torch.full((1, 1, 24), 0.5, device=DEV)
    tab = torch.tensor([[cam.data_ptr(), sgc.data_ptr(), 1, 1, 16, 16, 1, 0],
                        [cam.data_ptr(), sgc.data_ptr(), 1, 1, 8, 24, 0, 0]], dtype=torch.int64, device=DEV)
    keep = torch.tensor([0, 4], dtype=torch.int32, device=DEV)
    oc = torch.full((2, H, W), 7.0, device=DEV)          # fully overwritten: the old content must not show
    os_ = torch.full((2, H, W), 7.0, device=DEV)
    call("mx_cam_infer", ptr(tab), 2, 24, K, H, W, ptr(keep), 2, ptr(oc), ptr(os_), stream())
    assert torch.allclose(oc[0], torch.full((H, W), -6.0, device=DEV)) and torch.allclose(oc[1], torch.full((H, W), 4.0, device=DEV))
    assert torch.allclose(os_, torch.full((2, H, W), 1.0, device=DEV))
    only = torch.full((2, H, W), 7.0, device=DEV)
    call("mx_cam_infer", ptr(tab), 2, 24, K, H, W, ptr(keep), 2, None, ptr(only), stream())
    assert torch.equal(only, os_)
    call("mx_cam_infer", ptr(tab), 2, 24, K, H, W, ptr(keep), 2, ptr(only), None, stream())
    assert torch.equal(only, oc)
    # against the per-pass kernel, one flipped pass of a 3 x 2 map that is not constant
    src = T(synth.normal(2, "lr", (3, 2, 24)).astype(np.float32)).to(DEV)
    acc = torch.zeros(K - 1, H, W, device=DEV)
    call("mx_infer_accum", ptr(src), ptr(acc), 3, 2, 24, K, 40, 30, H, W, 1, stream())
    tab1 = torch.tensor([[src.data_ptr(), src.data_ptr(), 3, 2, 40, 30, 1, 0]], dtype=torch.int64, device=DEV)
    all20 = torch.arange(20, dtype=torch.int32, device=DEV)
    o20 = torch.empty(20, H, W, device=DEV)
    call("mx_cam_infer", ptr(tab1), 1, 24, K, H, W, ptr(all20), 20, ptr(o20), None, stream())
    assert torch.equal(o20, acc)
    # the case of test_infer_kernels_edge_cases itself (one flipped pass of the 1 x 1 map), then the normalisation
    acc = torch.zeros(K - 1, H, W, device=DEV)
    call("mx_infer_accum", ptr(cam), ptr(acc), 1, 1, 24, K, 16, 16, H, W, 1, stream())
    one = torch.empty(2, H, W, device=DEV)
    call("mx_cam_infer", ptr(tab), 1, 24, K, H, W, ptr(keep), 2, ptr(one), None, stream())
    assert torch.equal(one, acc[[0, 4]])
    assert torch.allclose(one[1], torch.full((H, W), 2.0, device=DEV)) and torch.allclose(one[0], torch.full((H, W), -3.0, device=DEV))
    call("mx_infer_norm", ptr(one), 2, H * W, stream())
    call("mx_infer_norm", ptr(acc), K - 1, H * W, stream())
    assert torch.equal(one, acc[[0, 4]])
    ref = np.full((H, W), 2.0, np.float32)
    mn, mx = ref.min(), ref.max()
    ref[ref < mn + 1e-6] = 0
    ref = (ref - mn - 1e-6) / (mx - mn + 1e-6)
    assert np.allclose(one[1].cpu().numpy(), ref, rtol=1e-5)
    assert np.allclose(one[0].cpu().numpy(), -1.0, rtol=1e-5)    # negative channel -> clamped to 0 -> (0 - 0 - 1e-6)/1e-6


def test_cam_infer_argument_errors():
    from muscle_amd._lib import lib, ptr
    L = lib()
    m = torch.zeros(2, 2, 24, device=DEV)
    tab = torch.tensor([[m.data_ptr(), m.data_ptr(), 2, 2, 4, 4, 0, 0]], dtype=torch.int64, device=DEV)
    keep = torch.tensor([0, 1], dtype=torch.int32, device=DEV)
    out = torch.empty(2, 4, 4, device=DEV)
    good = (ptr(tab), 1, 24, 21, 4, 4, ptr(keep), 2, ptr(out), ptr(out))
    for i, v in ((0, None), (6, None), (1, 0), (2, 22), (2, 20), (3, 1), (3, 25), (4, 0), (5, 0), (7, 0), (7, 21), (7, -1)):
        args = list(good)
        args[i] = v
        assert L.mx_cam_infer(*args, None) < 0, (i, v)
        assert b"cam_infer" in L.mx_last_error()
    args = list(good)
    args[8] = args[9] = None                                        # both outputs NULL
    assert L.mx_cam_infer(*args, None) < 0
    torch.cuda.synchronize()
