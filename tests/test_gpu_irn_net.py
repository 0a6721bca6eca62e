"""GPU parity of the IRN edge / displacement network (muscle_amd/irn.py, csrc/irn_net.hip) and of infer_irn end to end.

Yardstick: the fp64 restatement tests/irn_net_ref.py on the CPU.  err(t) = max|t - t64| / max|t64|; e32 is that error for
the fp32 torch-CPU restatement (the arithmetic the reference's fixture was made with), eHIP for the HIP path.  Required per
tensor: eHIP <= 2 e32 + 2e-7, in exact-fp32 and in split arithmetic (the form of tests/test_gpu_split.py; the factor is 2
because the partner is another library's summation order).  Against the reference's fixture (fp32 against fp32) the bound
is that plus e32, by the triangle inequality.  Every figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_net_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_net.npz")
NAMES = ["x1", "x2", "x3", "x4", "x5", "edge_cat", "dp_cat1", "dp_cat2"]


def err(t, t64):
    return float((t.detach().cpu().double() - t64).abs().max()) / max(float(t64.abs().max()), 1e-30)


def check(name, hip, t32, t64):
    e_hip, e32 = err(hip, t64), err(t32, t64)
    print(f"[irn_net] {name}: eHIP {e_hip:.3e}  e32 {e32:.3e}  bound {2 * e32 + 2e-7:.3e}")
    assert e_hip <= 2 * e32 + 2e-7, (name, e_hip, e32)
    return e_hip, e32


def nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous()


def nchw(t):
    return t.permute(0, 3, 1, 2).contiguous()


def rnd(seed, name, shape, scale=1.0):
    from muscle_amd import synth
    return torch.from_numpy(synth.normal(seed, name, shape) * scale)


# ---- 1. the 3x3 convolution ------------------------------------------------------------------------------------------
CONV_SHAPES = [  # N, H, W, Ci, Co, stride, bias, relu
    (2, 128, 128, 64, 64, 1, True, True), (2, 128, 128, 128, 128, 2, True, True), (2, 64, 64, 128, 128, 1, True, True),
    (2, 64, 64, 256, 256, 2, True, True), (2, 32, 32, 256, 256, 1, True, True), (2, 32, 32, 512, 512, 1, True, True),
    (1, 13, 21, 64, 128, 1, True, False), (3, 17, 30, 32, 48, 2, False, True), (1, 9, 50, 20, 12, 1, False, False),
    (3, 7, 5, 8, 72, 2, True, True), (1, 33, 19, 36, 64, 2, False, False), (2, 16, 47, 48, 36, 1, True, True),
]


@pytest.mark.parametrize("shape", CONV_SHAPES, ids=lambda s: "x".join(str(v) for v in s))
def test_conv3x3_vs_fp64(shape):
    from muscle_amd import ops
    N, H, W, Ci, Co, stride, bias, relu = shape
    x = rnd(11, f"cx{shape}", (N, Ci, H, W))
    w = rnd(11, f"cw{shape}", (Co, Ci, 3, 3), (2.0 / (9 * Ci)) ** 0.5)
    s = 0.5 + torch.from_numpy(__import__("muscle_amd").synth.uniform(11, f"cs{shape}", (Co,)))
    b = rnd(11, f"cb{shape}", (Co,), 0.3) if bias else None

    def ref(dt):
        o = F.conv2d(x.to(dt), (w * s.view(-1, 1, 1, 1)).to(dt), None if b is None else b.to(dt), stride=stride, padding=1)
        return F.relu(o) if relu else o
    wp = ops.conv3x3_pack(w.float().to(DEV), s.float().to(DEV))
    y = ops.conv3x3(nhwc(x.float()).to(DEV), wp, bias=None if b is None else b.float().to(DEV), stride=stride, relu=relu)
    t64 = ref(torch.float64)
    assert tuple(y.shape) == (N, t64.shape[2], t64.shape[3], Co)
    # the partner rounds the scaled weight to fp32 exactly as the pack kernel does (one multiplication)
    t32 = F.conv2d(x.float(), (w.float() * s.float().view(-1, 1, 1, 1)), None if b is None else b.float(), stride=stride, padding=1)
    t32 = F.relu(t32) if relu else t32
    check(f"conv3x3 {shape}", nchw(y), t32, t64)


# ---- 2. the small kernels --------------------------------------------------------------------------------------------
def test_stem_maxpool_vs_fp64():
    from muscle_amd import ops
    N, H, W, S = 2, 45, 61, 64                                   # image smaller than the 64 x 64 frame: the pad bites
    x = rnd(12, "sx", (N, 3, H, W))
    w = rnd(12, "sw", (64, 3, 7, 7), (2.0 / 147) ** 0.5)
    b = rnd(12, "sb", (64,), 0.2)

    def ref(dt):
        xp = F.pad(x.to(dt), [0, S - W, 0, S - H])
        return F.max_pool2d(F.relu(F.conv2d(xp, w.to(dt), b.to(dt), stride=2, padding=3)), 3, 2, 1)
    H1 = (S - 1) // 2 + 1
    wp = torch.cat([w.float().reshape(64, 147), torch.zeros(64, 1)], dim=1).contiguous().to(DEV)
    a = ops.pw_fwd(ops.stem7_im2col(x.float().to(DEV), H1, H1), wp, 64, bias=b.float().to(DEV), relu=True).view(N, H1, H1, 64)
    y = ops.maxpool3s2(a)
    check("stem+maxpool", nchw(y), ref(torch.float32), ref(torch.float64))


@pytest.mark.parametrize("scale,crop", [(1, (12, 10)), (2, (23, 19)), (4, (45, 37)), (4, (48, 40))])
def test_gn_resize_slice_vs_fp64(scale, crop):
    from muscle_amd import ops
    N, Hs, Ws, C, G, ldd, coff = 2, 12, 10, 32, 4, 72, 24
    Hd, Wd = crop
    x = rnd(13, "gx", (N, C, Hs, Ws)) * 2 + 0.7
    ga, be = rnd(13, "gg", (C,)) * 0.3 + 1, rnd(13, "gb", (C,)) * 0.2

    def ref(dt):
        o = F.group_norm(x.to(dt), G, ga.to(dt), be.to(dt), 1e-5)
        if scale > 1:
            o = F.interpolate(o, scale_factor=scale, mode="bilinear", align_corners=False)
        return F.relu(o[..., :Hd, :Wd])
    guard = 7.25
    buf = torch.full((N * Hd * Wd * ldd + 64,), guard, dtype=torch.float32, device=DEV)          # guard rows after the buffer
    dst = buf[:N * Hd * Wd * ldd].view(N, Hd, Wd, ldd)
    xd = nhwc(x.float()).to(DEV)
    ops.gn_resize(xd, ops.gn_stats(xd, G), ga.float().to(DEV), be.float().to(DEV), dst, coff, scale)
    check(f"gn_resize x{scale} {crop}", nchw(dst[..., coff:coff + C]), ref(torch.float32), ref(torch.float64))
    assert bool((dst[..., :coff] == guard).all()) and bool((dst[..., coff + C:] == guard).all()) and bool((buf[-64:] == guard).all())


def test_gather_camdown_finish_vs_fp64():
    from muscle_amd import ops
    x = rnd(14, "ax", (3, 11, 15, 24)).float()
    assert torch.equal(ops.gather_s2(x.to(DEV)).cpu(), x[:, ::2, ::2].contiguous())
    cams = rnd(14, "cam", (20, 93, 125)).abs()
    d = ops.resize_planar_halfpixel(cams.float().to(DEV), 24, 32)
    ref = lambda dt: F.interpolate(cams.to(dt)[None], size=(24, 32), mode="bilinear", align_corners=False)[0]
    check("cam down-scale", d, ref(torch.float32), ref(torch.float64))
    Hf, Wf, h, w = 16, 20, 13, 17
    e, dp, mean = rnd(14, "fe", (2, Hf, Wf, 4)) * 2, rnd(14, "fd", (2, Hf, Wf, 4)), rnd(14, "fm", (2,))
    ge, gd = ops.irn_net_finish(e.float().to(DEV), dp.float().to(DEV), mean.float().to(DEV), h, w)

    def fin(dt):
        ee, dd = e.to(dt)[:, :h, :w, 0], dp.to(dt)[0, :h, :w, :2].permute(2, 0, 1)
        return torch.sigmoid(ee[0] / 2 + ee[1].flip(-1) / 2)[None], dd - mean.to(dt).view(2, 1, 1)
    (e32, d32), (e64, d64) = fin(torch.float32), fin(torch.float64)
    check("finish edge", ge, e32, e64)
    check("finish dp", gd, d32, d64)


# ---- 3. the whole network ---------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def refs():
    """Both fixture cases through the restatement in fp32 and fp64, once per session (the 512 x 512 fp64 pass is the cost)."""
    from muscle_amd import synth
    z = np.load(GOLD)
    out = {}
    for tag in ("a", "b"):
        crop, H, W, seed = (int(v) for v in z[f"{tag}_params"])
        sd = synth.irn_state_dict(seed)
        x = synth.irn_image_pair(H, W, seed)
        r = {"crop": crop, "x": x, "sd": sd}
        for nm, dt in (("f32", torch.float32), ("f64", torch.float64)):
            with torch.no_grad():
                e, d, named = R.edge_displacement(R.to_dtype(sd, dt), torch.from_numpy(x).to(dt), crop, want_named=True)
            r[nm] = dict(named, edge=e, dp=d)
        out[tag] = r
    return z, out


def build_model(r):
    import muscle_amd
    m = muscle_amd.EdgeDisplacement(crop_size=r["crop"])
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in r["sd"].items()}, strict=True)
    return m.to(DEV).eval()


@pytest.mark.both_arith
@pytest.mark.parametrize("tag", ["a", "b"])
def test_network_vs_fixture_and_fp64(refs, tag):
    from muscle_amd import synth
    z, rr = refs
    r = rr[tag]
    m = build_model(r)
    x = torch.from_numpy(r["x"]).to(DEV)
    edge, dp = m(x)
    with torch.no_grad():
        xs, ecat, cat1, cat2 = m.features(x)
    got = dict(zip(NAMES, [nchw(t) for t in xs] + [nchw(ecat), nchw(cat1), nchw(cat2)]), edge=edge, dp=dp)
    summ = z[f"{tag}_summary"]
    for i, k in enumerate(NAMES + ["edge", "dp"]):
        e_hip, e32 = check(f"net {tag} {k}", got[k], r["f32"][k], r["f64"][k])
        bound = (2 * e32 + 2e-7) + e32                                 # against the fp32 fixture: triangle inequality
        t64 = r["f64"][k]
        scale = float(t64.abs().max())
        if k in ("edge", "dp"):
            fix = torch.from_numpy(z[f"{tag}_{k}"]).double()
            e_fix = float((got[k].cpu().double() - fix).abs().max()) / scale
            print(f"[irn_net] net {tag} {k}: vs fixture {e_fix:.3e}  bound {bound:.3e}")
            assert tuple(got[k].shape) == tuple(fix.shape) and e_fix <= bound, (k, e_fix, bound)
        else:
            # [l2, probe-dot] of the fixture: |l2 - l2'| <= ||d||_2 <= sqrt(n) max|d|, |<p,d>| <= ||p||_1 max|d|
            a = got[k].cpu().double().numpy().ravel()
            pr = synth.normal(123, k, a.shape)
            mine = np.array([np.sqrt((a * a).sum()), (a * pr).sum()])
            lim = bound * scale * np.array([np.sqrt(a.size), np.abs(pr).sum()])
            print(f"[irn_net] net {tag} {k}: summary diff {np.abs(mine - summ[i])} limit {lim}")
            assert (np.abs(mine - summ[i]) <= lim).all(), (k, mine, summ[i], lim)


# ---- 4. infer_irn end to end --------------------------------------------------------------------------------------------
def test_infer_irn_end_to_end(refs):
    from muscle_amd import synth
    from muscle_amd.irn import infer_irn
    z, rr = refs
    r = rr["a"]
    crop, H, W, seed = (int(v) for v in z["a_params"])
    beta, times = (int(v) for v in z["e2e_params"])
    bg = float(z["e2e_bg_thres"])
    cam = synth.irn_cam_dict(H, W, seed)
    m = build_model(r)
    label, soft = infer_irn(m, torch.from_numpy(r["x"]).to(DEV), cam, beta=beta, exp_times=times, bg_thres=bg, soft_output=True)
    label, soft = label.cpu().numpy(), soft.cpu().numpy()
    assert label.dtype == np.uint8 and label.shape == (H, W) and soft.dtype == np.float16 and soft.shape == (H, W, 21)
    lab64, soft64, _ = R.infer_irn(R.to_dtype(r["sd"], torch.float64), torch.from_numpy(r["x"]).double(), cam, beta, times, bg, crop)
    for nm, lab_ref, soft_ref in (("fp64 restatement", lab64, soft64), ("fixture", z["e2e_label"], z["e2e_soft"])):
        diff = float((label != lab_ref).mean())
        sdiff = float(np.abs(soft.astype(np.float32) - soft_ref.astype(np.float32)).max())
        print(f"[irn_net] infer_irn vs {nm}: label share differing {diff:.3e}  soft max diff {sdiff:.3e}")
        assert diff <= 2e-3, (nm, diff)
        assert sdiff <= 1e-3, (nm, sdiff)


# ---- 5. the same bits every run -----------------------------------------------------------------------------------------
def test_forward_is_bit_reproducible(refs):
    _z, rr = refs
    r = rr["a"]
    m = build_model(r)
    x = torch.from_numpy(r["x"]).to(DEV)
    e1, d1 = m(x)
    e2, d2 = m(x)
    assert torch.equal(e1, e2) and torch.equal(d1, d2)
    m2 = build_model(r)                                               # a second prepare(): the same packed weights, the same bits
    e3, d3 = m2(x)
    assert torch.equal(e1, e3) and torch.equal(d1, d3)
