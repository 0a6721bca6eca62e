"""tests/dec_ref.py against independent statements of the same operations (torch's own operators and autograd, the oracle's
FieldLoss pieces), the input conditions that tests/test_gpu_dec_kernels.py and tests/test_gpu_head_kernels.py rely on - for the
very seeds and shapes they run, taken from the same tables - and the argument refusals of the entries (nothing is launched)."""
import ctypes
import os

import pytest
import torch
import torch.nn.functional as F

import dec_ref as R
from dec_ref import F32, F64, U

from muscle_amd import _lib
from oracle import mcl_oracle as O


def _close(a, b, tol=1e-12):
    scale = max(1.0, float(b.abs().max()))
    assert float((a - b).abs().max()) <= tol * scale


# ---- restatements ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 1, 1, 4), (2, 2, 3, 4), (1, 5, 4, 8), (2, 7, 7, 36)])
def test_avgpool_matches_torch(shape):
    x = torch.randn(shape, dtype=F64, requires_grad=True)
    y = F.avg_pool2d(x.permute(0, 3, 1, 2), 3, 2, 1, count_include_pad=True).permute(0, 2, 3, 1)
    _close(R.avgpool3s2(x.detach())[0], y.detach())
    g = torch.randn(y.shape, dtype=F64)
    y.backward(g)
    _close(R.avgpool3s2_bwd(g, shape[1], shape[2])[0], x.grad)
    xi = torch.randint(-2 ** 19, 2 ** 19, shape).float()
    # the exact-regime value: the integer sum times float32(1/9), rounded once: within 2U of the float64 quotient
    assert bool(((R.avgpool3s2_exact(xi).double() - R.avgpool3s2(xi)[0]).abs() <= 2 * U * R.avgpool3s2(xi)[0].abs()).all())


@pytest.mark.parametrize("size", R.RESIZE_SIZES, ids=lambda s: "x".join(map(str, s)))
def test_bilinear_matches_interpolate(size):
    Hs, Ws, Hd, Wd = size
    x = torch.randn(2, Hs, Ws, 4, dtype=F64, requires_grad=True)
    y = F.interpolate(x.permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=True)
    _close(R.resize_nhwc(x.detach(), Hd, Wd)[0], y.detach().permute(0, 2, 3, 1))
    _close(R.resize_nhwc(x.detach(), Hd, Wd, relu=True)[0], y.detach().permute(0, 2, 3, 1).clamp_min(0))
    g = torch.randn(y.shape, dtype=F64)
    y.backward(g)
    _close(R.resize_nhwc_bwd(g.permute(0, 2, 3, 1), Hs, Ws)[0], x.grad)
    src = torch.randn(2, Hs, Ws, 8, dtype=F64)
    up = F.interpolate(src[..., :5].permute(0, 3, 1, 2), size=(Hd, Wd), mode="bilinear", align_corners=True)
    _close(R.upsample_to_nchw(src, 5, Hd, Wd)[0], up)
    _close(R.upsample_to_nchw_bwd(g, Hs, Ws)[0], x.grad)
    W = R.bil_matrix(Hs, Hd)
    assert float((W.sum(1) - 1).abs().max()) < 1e-14 and float(W.min()) >= 0
    if Hs == Hd:
        assert torch.equal(W, torch.eye(Hs, dtype=F64))


def test_ce_matches_torch_and_first_maximum_wins():
    gen = torch.Generator().manual_seed(1)
    seg = torch.randn(2, 5, 33, generator=gen, dtype=F64, requires_grad=True)
    mask = torch.rand(2, 5, 33, generator=gen)                       # tie-free
    loss = F.cross_entropy(seg, mask.argmax(1))
    got, _, t = R.ce_argmax(seg.detach(), mask)
    assert abs(float(got) - float(loss.detach())) < 1e-13 and torch.equal(t, mask.argmax(1))
    (loss * 0.37).backward()
    _close(R.ce_argmax_bwd(seg.detach(), mask, 0.37)[0], seg.grad)
    tie = torch.tensor([[[0.0, 0.5, 0.25], [0.0, 0.5, 0.75], [0.0, 0.25, 0.75], [0.0, 0.5, 0.75]]])      # [1,4,3]
    assert R.ce_argmax(torch.zeros(1, 4, 3), tie)[2].tolist() == [[0, 0, 1]]
    for shape in R.CE_SHAPES[:3]:
        for kind in ("spread", "confident"):
            seg, mask = R.ce_inputs(shape, kind)
            top = mask.max(1, keepdim=True).values
            ntop = (mask == top).sum(1)
            if shape[2] > 100:
                assert bool((top == 0).any()) and bool((ntop == 2).any()) and bool((ntop >= 3).any())
            if kind == "spread" and shape[2] > 100:
                assert float(seg.max()) > 35 and float(seg.min()) < -35
            elif kind == "confident":
                assert float(R.ce_argmax(seg, mask)[0]) < 1e-3                     # near zero


def test_clip_matches_oracle():
    for n, mx in ((1001, 9.0), (1001, 1e3), (255, 0.5)):
        x = torch.randn(n, dtype=F64)
        p = torch.nn.Parameter(torch.zeros(n, dtype=F64))
        p.grad = x.clone()
        total = O.clip_grad_norm([p], mx)
        norm, v, _ = R.clip_grad_norm(x, mx)
        assert abs(float(total) - float(norm)) < 1e-12 * float(norm)
        _close(v, p.grad)
    norm, v, _ = R.clip_grad_norm(torch.zeros(7), 9.0)
    assert float(norm) == 0 and torch.equal(v, torch.zeros(7, dtype=F64))


def test_field_edges_match_oracle():
    N, K, H, W = 2, 5, 12, 13
    seg = R.smooth_field(3, (N, K, H, W)).double()
    lab = torch.tensor([[1.0, 0.0, 0.5, 1.0], [0.0, 0.0, 0.0, 0.0]], dtype=F64)
    ref = R.field_edges(seg, lab, 2.0)
    assert float((R.sobel5(F32) - O.sobel5_kernels()).abs().max()) == 0
    p = torch.softmax(seg * 2.0, 1)[:, 1:]
    e = F.conv2d(p.reshape(N * 4, 1, H, W), O.sobel5_kernels(F64), padding=2).view(N, 4, 2, H, W) * lab.view(N, 4, 1, 1, 1)
    mag, q = O.quantize_orient(e[:, :, 0], e[:, :, 1])
    _close(ref["mag"], mag, 1e-9)
    near = R.boundary_distance(ref["ang"]) < 1e-5          # the oracle's boundaries are float64 k*3.1416/8, ours the fp32 constants
    lb = ref["labelled"]                                   # (an unlabelled plane is -0 * lab in the oracle: angle pi, never used)
    assert bool(((ref["orient"].double() == q) | near)[lb].all()) and float(near[lb].double().mean()) < 0.01
    _close(ref["edge_fg"], mag.sum(1), 1e-9)
    assert bool((ref["mx"][lab == 0] == 0).all())
    _close(ref["mx"][lab != 0], mag.flatten(2).max(-1).values[lab != 0], 1e-9)
    assert bool((ref["orient"][~ref["labelled"]] == 7).all())
    assert float((ref["mag"][~ref["labelled"]] - 1e-4).abs().max()) < 1e-12
    assert abs(R.M_ZERO - 1e-4) < 1e-11


@pytest.mark.parametrize("hw", R.SELECT_HW, ids=lambda s: f"{s[0]}x{s[1]}")
@pytest.mark.parametrize("step", R.SELECT_STEPS)
def test_field_select_matches_oracle(hw, step):
    H, W = hw
    mag, orient, mx, slots = R.select_inputs(H, W)
    outs, ins, counts = R.field_select(mag.numpy(), orient.numpy(), mx.numpy(), slots, step, H, W)
    for s, (n, f) in enumerate(slots):
        m = mx[n, f]
        pos = ((mag[n, f] >= torch.tensor(0.8, dtype=F32) * m) & (m > 1)).view(H, W)
        o, i = O.field_points(orient[n, f].view(H, W).long() + 1, pos, step, H, W)
        assert outs[s].tolist() == o.tolist() and ins[s].tolist() == i.tolist()
        assert counts[s].tolist() == [len(o), len(i), int(pos.sum())]
    # the input conditions of the GPU cases: no positives, all positive, every sector, unsorted slots
    by = {sl: c for sl, c in zip(slots, counts)}
    assert by[(0, 1)][2] == 0 and by[(1, 2)][2] == H * W and slots != sorted(slots)
    if H * W >= 8:
        assert set(orient[0, 0].tolist()) == set(range(8))


def test_field_gather_and_scatter_match_autograd():
    gen = torch.Generator().manual_seed(5)
    N, CH, H, W, h, w, K, ML = 2, 7, 9, 11, 3, 4, 5, 8
    pts = R.field_points_for(N, H, W, 20, gen)
    mask = torch.randn(N, K, H, W, generator=gen)
    for mode, dense in ((0, torch.randn(N, CH, H, W, generator=gen)), (1, torch.randn(N, h, w, CH, generator=gen))):
        feat, mf = R.field_gather(dense, mode, mask, pts, K, ML, H, W)
        if mode == 1:
            up = F.interpolate(dense.double().permute(0, 3, 1, 2), size=(H, W), mode="bilinear", align_corners=True)
        else:
            up = dense.double()
        n, p = pts[:, 0].long(), pts[:, 1].long()
        _close(feat, torch.softmax(up, 1)[n, :, p // W, p % W])
        _close(mf[:, :K], torch.softmax(mask.double(), 1)[n, :, p // W, p % W])
        assert float(mf[:, K:].abs().max()) == 0
        gfeat = torch.randn(20, CH, generator=gen)
        got, mag = R.field_scatter(feat, gfeat, pts, mode, dense.shape, 0.37, H, W)
        _close(got, R.field_scatter_autograd(dense, gfeat, pts, mode, 0.37, H, W))
        assert bool((mag >= got.abs() - 1e-15).all())


def test_field_terms_match_oracle():
    sim, simm = R.terms_inputs(8, 2)
    ref = R.field_terms(sim, simm, 0.5)
    s64 = sim.double().requires_grad_(True)
    total = 0
    for s in range(2):
        l = 0
        for dim in (1, 0):
            l = l + O._field_terms(simm[s].double().mean(dim) > simm[s].double().mean(), (s64[s].mean(dim) > s64[s].mean()).detach(), s64[s], dim)
        assert abs(float(l.detach()) * 0.5 - float(ref["slot_loss"][s])) < 1e-14
        total = total + l * 0.5
    total.backward()
    _close(ref["gsim"], s64.grad)


def test_head_restatements():
    gen = torch.Generator().manual_seed(9)
    x = torch.randn(6, 21, generator=gen, dtype=F64, requires_grad=True)
    eps = 1e-5
    y = x / (x.norm(dim=1, keepdim=True) + eps)
    ry, rn, _ = R.row_l2norm(x.detach(), eps)
    _close(ry, y.detach())
    gy = torch.randn(6, 21, generator=gen, dtype=F64)
    y.backward(gy)
    _close(R.row_l2norm_bwd(x.detach(), rn, gy, eps)[0], x.grad, 1e-11)
    z = torch.zeros(2, 5)
    assert float(R.row_l2norm(z, eps)[0].abs().max()) == 0
    assert torch.equal(R.row_l2norm_bwd(z, torch.zeros(2), torch.ones(2, 5), eps)[0], torch.full((2, 5), 1.0 / eps, dtype=F64))
    T = (torch.rand(9, 24, generator=gen, dtype=F64) + 0.5).requires_grad_(True)
    for K in (20, 21, 23):
        T.grad = None
        rv = T[:, :K] / (T[:, K] + eps)[:, None]
        out = R.pcm_norm(T.detach(), K, eps)[0]
        _close(out[:, :K], rv.detach())
        assert float(out[:, K:].abs().max()) == 0
        g = torch.randn(9, 24, generator=gen, dtype=F64)
        rv.backward(g[:, :K])
        _close(R.pcm_norm_bwd(T.detach(), g, K, eps)[0], T.grad, 1e-11)
    gaff, aff = torch.randn(2, 5, 8, generator=gen), torch.randn(2, 5, 8, generator=gen)
    f = torch.randn(2, 5, 3, generator=gen, dtype=F64, requires_grad=True)
    a = f @ f.transpose(1, 2)
    torch.relu(a).backward(gaff[:, :, :5].double())
    G2 = R.sym_relu_grad(gaff, F.pad(a.detach(), (0, 3)), 5)
    _close(torch.bmm(G2[:, :, :5], f.detach()), f.grad, 1e-11)
    assert float(G2[:, :, 5:].abs().max()) == 0
    a1, b1 = torch.randn(9, generator=gen), torch.randn(9, generator=gen)
    yv = torch.tensor([1.0, 0.0, -0.0, -1.0, 2.0, 0.0, 3.0, -2.0, 1e-30])
    _close(R.ew(0, a1, alpha=-1.5)[0], -1.5 * a1.double())
    _close(R.ew(1, a1, b1, alpha=0.3)[0], a1.double() + 0.3 * b1.double())
    _close(R.ew(2, a1, b1, yv)[0], (a1.double() + b1.double()) * (yv > 0))
    _close(R.ew(2, a1, None, yv)[0], a1.double() * (yv > 0))
    X, v = torch.randn(7, 4, generator=gen), torch.randn(3, 4, generator=gen)
    _close(R.bcast_add(X, v, -0.5, 3)[0], X.double() - 0.5 * v.double().repeat_interleave(3, 0)[:7])


# ---- the input conditions of the GPU cases ------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", [c for c in R.RESIZE_CASES if c != R.RESIZE_FWD_ONLY], ids=lambda c: "-".join(map(str, c)))
def test_resize_adjoint_condition(case):
    """The sum rule's allowance stays below a tenth of the share of one destination row or column."""
    N, C, Hs, Ws, Hd, Wd = case
    _, g, _ = R.resize_inputs(case)
    _, _, e_ref, rel, share = R.adjoint_rule(g, Hs, Ws)
    assert rel < 0.1 * share, (e_ref / U, rel, share)


@pytest.mark.parametrize("case", [c for c in R.UPSAMPLE_CASES if c != R.UPSAMPLE_FWD_ONLY], ids=lambda c: "-".join(map(str, c)))
def test_upsample_adjoint_condition(case):
    N, K, lds, Hs, Ws, Hd, Wd = case
    _, g, _ = R.upsample_inputs(case)
    _, _, e_ref, rel, share = R.adjoint_rule(g.permute(0, 2, 3, 1), Hs, Ws)
    assert rel < 0.1 * share, (e_ref / U, rel, share)


def test_grid_cap_cases_are_above_the_cap():
    cap = R.GRID_CAP
    assert 129 * 129 * 128 > cap and 257 * 257 * 128 > cap                        # avgpool (1,257,257,512), both directions
    N, C, Hs, Ws, Hd, Wd = R.RESIZE_CASES[-2]
    assert N * Hd * Wd * C // 4 > cap
    N, C, Hs, Ws, Hd, Wd = R.RESIZE_CASES[-1]
    assert N * Hs * Ws * C // 4 > cap
    N, K, lds, Hs, Ws, Hd, Wd = R.UPSAMPLE_CASES[-1]
    assert N * K * Hd * Wd > cap
    assert 448 * 28 * 4 > 48 * 1024 > 250 * 40 * 4
    assert R.CE_SHAPES[-1][0] * R.CE_SHAPES[-1][2] > cap and R.EDGE_SHAPES[4][2] * R.EDGE_SHAPES[4][3] > cap
    assert R.CLIP_N[-2] > 2048 * 256 and R.CLIP_N[-1] > 4096 * 256
    HW = R.EDGE_SHAPES[4][2] * R.EDGE_SHAPES[4][3]
    assert (HW - cap) % 256 != 0 and (HW - cap) // 256 + 1 < 8192             # second sweep: one partly idle workgroup, idle ones after it
    assert R.EDGE_SHAPES[0][2] * R.EDGE_SHAPES[0][3] * 2 < 256 < R.EDGE_SHAPES[5][0] * 99 and R.EDGE_SHAPES[3][1] - 1 == 65


@pytest.mark.parametrize("beta", R.EDGE_BETAS)
@pytest.mark.parametrize("shape", R.EDGE_SHAPES[:4] + R.EDGE_SHAPES[5:], ids=lambda s: "x".join(map(str, s)))
def test_orient_compared_share(shape, beta):
    """At least 95 % of the labelled pixels (beta = 2), or of those above the magnitude floor (beta = 100), lie farther from every
    sector boundary than 4 x the fp32 restatement's angle error (the larger of the case's own and the calibration draw's)."""
    seg, lab = R.edge_inputs(shape, beta)
    ref = R.field_edges(seg, lab, beta)
    err = max(R.edge_calib(beta)[3], R.angle_error(seg, lab, beta, ref))
    cmp_, floor = R.orient_compare_mask(ref, err)
    base = int(ref["labelled"].sum()) if beta < 10 else int(floor.sum())
    assert base > 0 and int(cmp_.sum()) >= 0.95 * base, (err, int(cmp_.sum()), base)
    assert bool((lab == 0.5).any()) and bool((lab == 0).any()) and bool((lab == 1).any())
    if shape[0] > 1:
        assert float(lab[R.edge_empty_sample(shape[0])].abs().sum()) == 0 and bool((lab.abs().sum(1) > 0)[-1])


@pytest.mark.parametrize("k", R.TERMS_K)
@pytest.mark.parametrize("S", R.TERMS_S)
def test_terms_margins(k, S):
    """Every decision margin exceeds 4 x the fp32 restatement's error in the means; all four classes occur in slot 0 along both
    dimensions; slot 1 has two empty classes."""
    sim, simm = R.terms_inputs(k, S)
    ref = R.field_terms(sim, simm, 0.5)
    for t in (sim, simm):
        t64 = t.double()
        e = 0.0
        for dim in (1, 2):
            e = max(e, float((t.mean(dim).double() - t64.mean(dim)).abs().max()))
        e += float((t.mean((1, 2)).double() - t64.mean((1, 2))).abs().max())
        which = 0 if t is sim else 1
        assert float(ref["margins"][:, :, which].min()) > 4.0 * max(e, U), (e, float(ref["margins"][:, :, which].min()))
    assert bool((ref["counts"][0] > 0).all())
    if S > 1:
        assert ref["counts"][1, :, 0].tolist() == [0, 0] and ref["counts"][1, :, 1].tolist() == [0, 0]


@pytest.mark.parametrize("mode,hw,ch", [(1, hw, ch) for hw in range(4) for ch in range(5)] + [(0, hw, ch) for hw in range(4) for ch in range(2)])
def test_scatter_point_condition(mode, hw, ch):
    """field_scatter: the allowance (with the atomics' roundings in mode 0) stays below a tenth of the smallest share of a point;
    the point with corners in four tiles has them there; sample 1 has no point."""
    (h, w), CH = R.SCATTER_HW[hw], R.SCATTER_CH[ch]
    c = R.scatter_rule(h, w, CH, mode, R.scatter_gup(hw, ch, mode))
    assert c["rel"] + c["atomics"] < 0.1 * c["share"], (c["e_ref"] / U, c["rel"], c["share"])
    assert not bool((c["pts"][:, 0] == 1).any()) and int((c["pts"][:, 1] == 0).sum()) >= 8
    if mode == 1 and h > 8 and w > 8:
        Wy, Wx = R.bil_matrix(h, c["H"])[int(c["pts"][16, 1]) // c["W"]], R.bil_matrix(w, c["W"])[int(c["pts"][16, 1]) % c["W"]]
        assert Wy[7] > 0 and Wy[8] > 0 and Wx[7] > 0 and Wx[8] > 0
    assert 64 * R.SCATTER_CH[3] * 4 > 64 * 1024 and R.SCATTER_CH[3] > 256


def test_sum_conditions_of_ce_clip_and_rows():
    """Where a sum has at most 100 000 terms its allowance is below a tenth of one term's share (the norms: a twentieth, the square
    root halves it); the longer sums have their exact regimes, whose expected values are what float64 gives."""
    for shape in R.CE_SHAPES:
        n = shape[0] * shape[2]
        for kind in ("spread", "confident"):
            if n <= 100000:
                assert R.ce_fwd_rule(*R.ce_inputs(shape, kind))[3] < 1.0 / (10.0 * n), (shape, kind)
        if n <= 300000:
            seg, mask, want = R.ce_exact_inputs(shape)
            ref = float(R.ce_argmax(seg, mask)[0])
            assert abs(float(want) - ref) <= 2 * U * ref and 20 <= ref <= 27      # log(1 + exp(-20)) is 2e-9: far below fp32
    for n in R.CLIP_N:
        for sc in R.CLIP_SCENARIOS:
            if n <= 100000:
                assert R.clip_rule(*R.clip_inputs(n, sc))[3] < 1.0 / (20.0 * n), (n, sc)
        x, want = R.clip_exact_inputs(n)
        assert abs(float(want) - float(R.clip_grad_norm(x, 1e9)[0])) <= U * float(want) and bool((x.abs() == 4).all())
    for Rn in R.ROW_R:
        for C in R.ROW_C:
            x, gy = R.row_inputs(Rn, C)
            assert R.row_norm_rule(x)[1] < 1.0 / (20.0 * C) and R.row_dot_rule(x, gy)[1] < 1.0 / (10.0 * C), (Rn, C)
            assert Rn < 3 or bool((x == 0).all(1).any())
    assert R.ROW_R[-1] > 8192 * 4


def test_calibration_draws():
    """The fixed draws the exp / atan2 paths are judged by give finite, non-trivial figures (what the committed profile records)."""
    for kind in ("spread", "confident"):
        assert 1.0 < R.ce_bwd_units(kind) < 1e3
    for beta in R.EDGE_BETAS:
        up, um, ue, ang = R.edge_calib(beta)
        assert 1.0 < up < 1e3 and 1.0 < um < 1e3 and 1.0 < ue < 1e3 and 0 < ang < 1e-3
    for mode in (0, 1):
        assert all(1.0 < u < 1e3 for u in R.gather_calib(mode))
    geos = {g[0] for g in R.GATHER_GEO}
    assert geos == {0, 1} and max(R.GATHER_CH) == 1024 and (24, 24) in R.GATHER_KML


# ---- argument refusals --------------------------------------------------------------------------------------------------------
def test_bad_arguments_before_any_launch():
    """MX_EARG (-1) with the entry's name in mx_last_error(); the pointers are host memory and are never dereferenced."""
    if not os.path.exists(_lib.LIB_PATH):
        from muscle_amd import _build
        _build.build(verbose=False)
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    st = None
    cases = [
        ("avgpool3s2", (p, p, 1, 4, 4, 6, 0, st)),
        ("resize_nhwc", (p, p, 1, 3, 3, 6, 6, 6, 8, 0, 0, st)),
        ("resize_nhwc", (p, p, 1, 3, 3, 8, 6, 6, 8, 4, 0, st)),                      # coff + C > ldd
        ("bcast_add", (p, p, 1.0, 4, 6, 2, st)),
        ("resize_nhwc_bwd", (p + 4, p, 1, 3, 3, 4, 6, 6, st)),
        ("resize_nhwc_bwd", (p, p + 8, 1, 3, 3, 4, 6, 6, st)),
        ("upsample_to_nchw_bwd", (p, p, 1, 4, 41, 1, 1, 1000, 8, 0, st)),            # 1000 * 41 * 4 = 164 000 > 163 840
        ("ce_argmax", (p, p, None, p, None, 1, 2, 4, 0, None, 0, st)),
        ("ce_argmax", (p, p, None, p, None, 1, 2, 4, 0, p, 4, st)),
        ("field_select", (p, p, p, p, 1, 7, p, p, p, 3, 5, 2, st)),
        ("field_gather", (p, 0, 0, 0, p, p, 4, p, p, 1025, 21, 24, 8, 8, st)),
        ("field_gather", (p, 0, 0, 0, p, p, 4, p, p, 64, 65, 64, 8, 8, st)),
        ("field_gather", (p, 0, 0, 0, p, p, 4, p, p, 64, 21, 20, 8, 8, st)),
        ("field_terms", (p, p, 1, 257, 1.0, p, p, p, st)),
        ("field_scatter", (p, p, p, 4, 1, 3, 3, None, p, None, 1, 64, 21, 21, st)),
        ("field_scatter", (p, p, p, 4, 1, 3, 3, None, p, p, 1, 644, 21, 21, st)),      # 64 * 644 * 4 = 164 864 > 163 840
        ("pcm_norm", (p, None, p, 4, 24, 24, 1e-5, 0, st)),
        ("pcm_norm", (p, None, p, 4, 24, 25, 1e-5, 0, st)),
        ("ew", (1, p, None, None, 1.0, p, 4, st)),
        ("ew", (2, p, p, None, 1.0, p, 4, st)),
    ]
    assert 1000 * 41 * 4 > 160 * 1024 and 64 * 644 * 4 > 160 * 1024
    for name, args in cases:
        assert getattr(L, "mx_" + name)(*args) == -1, (name, args)
        assert name.encode() in L.mx_last_error(), (name, L.mx_last_error())
