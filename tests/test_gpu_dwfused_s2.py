"""The fused stride-2 depthwise backward (mx_dwconv_bwd_fused_s2: BN1 data gradient formed while the output-resolution tile is
staged, weight + data gradients from the one staged tile with the taps chosen by pixel parity, swish'(bn0) and the BN0 backward sums
in the epilogue; reference model.py:76-90 backward with Conv2dStaticSamePadding, utils.py:122-145) against float64 autograd of the
same chain: even and odd images, both pad_lo of each kernel size, images smaller than a tile or than the kernel, channel counts that
are not a multiple of the 32-channel chunk, several workgroups per chunk, and (MULTI) several tiles per workgroup: groups that run
from one sample into the next, and groups that the tile sequence does not reach."""
import pytest
import torch
import torch.nn.functional as F

import dw_geom

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _swish_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


CASES = [
    (2, 56, 56, 32, 3),                                        # several tiles, even size, pad_lo 0
    (2, 28, 28, 24, 5),                                        # ragged channel chunk, pad_lo 1
    (2, 21, 37, 20, 3), (1, 15, 15, 40, 5),                    # odd sizes, pad_lo 1 / 2, ragged tiles, two chunks
    (3, 9, 9, 32, 5), (2, 2, 2, 8, 3), (1, 1, 1, 4, 5),        # image smaller than a tile or than the kernel
    (4, 64, 64, 36, 3),                                        # more than one workgroup per chunk
]


def _same_pad(H, W, K):
    """(Ho, Wo, pad_lo, (left, right, top, bottom)) of the TF 'same' padding of a stride-2 K x K kernel, as
    test_depthwise_forward_matches_float64 builds it."""
    Ho, Wo = (H + 1) // 2, (W + 1) // 2
    pt_h, pt_w = max((Ho - 1) * 2 + K - H, 0), max((Wo - 1) * 2 + K - W, 0)
    assert pt_h // 2 == pt_w // 2
    return Ho, Wo, pt_h // 2, (pt_w // 2, pt_w - pt_w // 2, pt_h // 2, pt_h - pt_h // 2)


def _reference(dA, D, gate, add, st1, c1, X, st0, W, pads):
    """tests/test_gpu_dwfused.py::_reference with F.pad + stride 2."""
    d = lambda t: t.double()
    dA, D, gate, add, X, W, c1 = map(d, (dA, D, gate, add, X, W, c1))
    a1, b1 = d(st1.scale), d(st1.shift)
    dd = c1[0] * ((dA * gate[:, None, None, :] + add[:, None, None, :]) * _swish_grad(a1 * D + b1)) + c1[1] * D + c1[2]
    x = X.clone().requires_grad_()
    w = W.clone().requires_grad_()
    act = F.silu(d(st0.scale) * x + d(st0.shift))
    y = F.conv2d(F.pad(act.permute(0, 3, 1, 2), pads), w, stride=2, groups=X.shape[3])
    (y * dd.permute(0, 3, 1, 2)).sum().backward()
    gX = x.grad / d(st0.scale)       # the kernel returns dL/d(a0*x + b0): the BatchNorm-0 backward that follows carries the scale
    part = torch.stack([gX.sum((0, 1, 2)), (gX * X).sum((0, 1, 2))])
    return gX, w.grad, part


def _inputs(N, H, W, C, K):
    from muscle_amd import ops
    Ho, Wo, pad_lo, pads = _same_pad(H, W, K)
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + H * 10 + C + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    dA, D, X = rn(N, Ho, Wo, C), rn(N, Ho, Wo, C), rn(N, H, W, C)
    gate, add = torch.sigmoid(rn(N, C)), rn(N, C) * 0.1
    mk = lambda: ops.BNState(torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1, rn(C) * 0.1, torch.rand(C, device=DEV, generator=g) + 0.5)
    st1, st0 = mk(), mk()
    c1 = rn(3, C) * 0.3
    Wt = rn(C, 1, K, K) * 0.3
    return (dA, D, gate, add, st1, c1, X, st0, Wt), pad_lo, pads


def _case(N, H, W, C, K):
    from muscle_amd import ops
    (dA, D, gate, add, st1, c1, X, st0, Wt), pad_lo, pads = _inputs(N, H, W, C, K)
    want_gx, want_dw, want_part = _reference(dA, D, gate, add, st1, c1, X, st0, Wt, pads)
    outs = []
    for _ in range(2):
        dW = torch.zeros_like(Wt)
        gX, part = ops.dwconv_bwd_fused_s2(dA, D, gate, add, st1, c1, X, st0, Wt, dW, K, pad_lo)
        outs.append((gX, dW, part))
    (gX, dW, part), (gX2, dW2, part2) = outs
    assert part.shape == (ops.lib().mx_dwconv_bwd_fused_s2_parts(N, H, W, C, K), 2, C)
    err_gx = float((gX.double() - want_gx).abs().max())
    err_dw = float((dW.double() - want_dw).abs().max())
    err_part = float((part.double().sum(0) - want_part).abs().max())
    print(f"gX {err_gx:.3e} / max {float(want_gx.abs().max()):.3e}  dW {err_dw:.3e} / max {float(want_dw.abs().max()):.3e}  "
          f"part {err_part:.3e} / max {float(want_part.abs().max()):.3e}  rows {part.shape[0]}")
    assert torch.equal(gX, gX2) and torch.equal(dW, dW2) and torch.equal(part, part2)      # same bits every run (no atomics)
    assert err_gx <= 2e-5 * float(want_gx.abs().max()) + 1e-6                              # every element
    assert err_dw <= 5e-5 * float(want_dw.abs().max()) + 1e-5
    assert err_part <= 5e-5 * float(want_part.abs().max()) + 1e-5
    return part, pad_lo


@pytest.mark.parametrize("N,H,W,C,K", CASES)
def test_fused_s2_depthwise_backward_matches_float64(N, H, W, C, K):
    _case(N, H, W, C, K)


# 32 channel chunks leave 4096 / 32 = 128 groups (3x3) or 2048 / 32 = 64 (5x5) for 5 x 33 tiles of the unshifted tiling
MULTI = [
    (5, 88, 96, 1024, 3, 0, 33, 2, 83, 83),        # pad_lo 0: the launch's tiling is the counted one, 2 tiles per group
    (5, 88, 96, 1024, 5, 1, 48, 5, 55, 48),        # pad_lo 1: origins at -1, so 4 x 12 tiles per sample where 3 x 11 were counted; 5 per group, 7 groups never reached
]


@pytest.mark.parametrize("N,H,W,C,K,pad_lo,ntile,tpb,groups,reached", MULTI)
def test_fused_s2_multi_tile_groups(N, H, W, C, K, pad_lo, ntile, tpb, groups, reached):
    from muscle_amd import ops
    geo = dw_geom.fused_s2_geom(N, H, W, C, K, pad_lo)
    assert (geo.ntile, geo.tpb, geo.groups) == (ntile, tpb, groups)
    assert geo.groups == ops.lib().mx_dwconv_bwd_fused_s2_parts(N, H, W, C, K)
    dw_geom.assert_multi_tile(geo)
    assert dw_geom.cdiv(N * geo.ntile, geo.tpb) == reached
    part, got_pad = _case(N, H, W, C, K)
    assert got_pad == pad_lo
    # a group past the end of the (sample, tile) sequence writes rows of zeros (the finalise adds every row)
    assert int(part[reached:].count_nonzero()) == 0
    assert all(int(part[r].count_nonzero()) > 0 for r in (0, reached - 1))


def test_fused_s2_model_padding_on_odd_image():
    """The model freezes its pads at the nominal (even) size: an odd feature map then keeps pad_lo = (K-1)/2 - 1 and
    Ho = floor(H/2) (arch.static_same_pad / BlockCfg.out_size), which the kernel takes like any other static padding."""
    from muscle_amd import ops
    N, H, W, C, K = 2, 21, 37, 20, 5
    pad_lo, pad_hi = 1, 2
    Ho, Wo = (H + pad_lo + pad_hi - K) // 2 + 1, (W + pad_lo + pad_hi - K) // 2 + 1
    g = torch.Generator(device=DEV).manual_seed(7)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    mk = lambda: ops.BNState(torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1, rn(C) * 0.1, torch.rand(C, device=DEV, generator=g) + 0.5)
    dA, D, X, gate, add = rn(N, Ho, Wo, C), rn(N, Ho, Wo, C), rn(N, H, W, C), torch.sigmoid(rn(N, C)), rn(N, C) * 0.1
    st1, st0, c1, Wt = mk(), mk(), rn(3, C) * 0.3, rn(C, 1, K, K) * 0.3
    want_gx, want_dw, want_part = _reference(dA, D, gate, add, st1, c1, X, st0, Wt, (pad_lo, pad_hi, pad_lo, pad_hi))
    dW = torch.zeros_like(Wt)
    gX, part = ops.dwconv_bwd_fused_s2(dA, D, gate, add, st1, c1, X, st0, Wt, dW, K, pad_lo)
    assert float((gX.double() - want_gx).abs().max()) <= 2e-5 * float(want_gx.abs().max()) + 1e-6
    assert float((dW.double() - want_dw).abs().max()) <= 5e-5 * float(want_dw.abs().max()) + 1e-5
    assert float((part.double().sum(0) - want_part).abs().max()) <= 5e-5 * float(want_part.abs().max()) + 1e-5


def test_fused_s2_defer_hands_over_the_weight_gradient():
    from muscle_amd import ops
    N, H, W, C, K = 2, 28, 28, 24, 5
    (dA, D, gate, add, st1, c1, X, st0, Wt), pad_lo, _ = _inputs(N, H, W, C, K)
    dW_now = torch.zeros_like(Wt)
    gX_now, part_now = ops.dwconv_bwd_fused_s2(dA, D, gate, add, st1, c1, X, st0, Wt, dW_now, K, pad_lo)
    handed = []
    dW = torch.full_like(Wt, 3.0)
    gX, part = ops.dwconv_bwd_fused_s2(dA, D, gate, add, st1, c1, X, st0, Wt, dW, K, pad_lo, defer=lambda s, w: handed.append((s, w)))
    torch.cuda.synchronize()
    assert len(handed) == 1 and handed[0][1] is dW
    assert handed[0][0].shape == (part.shape[0], C * K * K)
    assert torch.equal(dW, torch.full_like(Wt, 3.0))                       # untouched until the rows are added
    ops.dw_parts_reduce(*handed[0])
    assert torch.equal(dW, dW_now + 3.0)
    assert torch.equal(gX, gX_now) and torch.equal(part, part_now)


def test_fused_s2_parts_fit_the_one_launch_finalise():
    """B7's three stride-2 blocks and the decoder configuration's fourth at batch 32 / 448 px, and the same at the 224 px views."""
    from muscle_amd import ops
    L = ops.lib()
    for N, H, C, K in [(32, 224, 192, 3), (32, 112, 288, 5), (32, 56, 480, 3), (32, 28, 1344, 5),
                       (32, 112, 192, 3), (32, 56, 288, 5), (32, 28, 480, 3), (32, 14, 1344, 5)]:
        p = L.mx_dwconv_bwd_fused_s2_parts(N, H, H, C, K)
        assert 1 <= p <= 1024, (N, H, C, K, p)
