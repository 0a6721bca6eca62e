"""The fused stride-1 depthwise backward (mx_dwconv_bwd_fused: BN1 data gradient formed while the tile is staged, weight + data
gradients from the one staged tile, swish'(bn0) and the BN0 backward sums in the epilogue; reference model.py:76-90 backward)
against float64 autograd of the same chain, on every tile shape the kernel has (14 x 28 and 8 x 16, 3x3 and 5x5), ragged images,
channel counts that are not a multiple of the 32-channel chunk, with and without BN0 / residual; and the depthwise forward
(mx_dwconv_fwd) against float64 on both paddings the model meets.

The *_MULTI cases put each kernel on its several-tiles-per-workgroup loop (tests/dw_geom.py restates the launch geometry and every
such case asserts it against the library first): a workgroup's partial sums then run over a tile sequence that crosses from one sample
into the next, with the gate / add of the SE block re-staged per tile, and the last group is short."""
import pytest
import torch
import torch.nn.functional as F

import dw_geom

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _swish_grad(z):
    s = torch.sigmoid(z)
    return s * (1 + z * (1 - s))


def _reference(dA, D, gate, add, st1, c1, X, st0, W, K, residual):
    d = lambda t: t.double()
    dA, D, gate, add, X, W, c1 = map(d, (dA, D, gate, add, X, W, c1))
    a1, b1 = d(st1.scale), d(st1.shift)
    dd = c1[0] * ((dA * gate[:, None, None, :] + add[:, None, None, :]) * _swish_grad(a1 * D + b1)) + c1[1] * D + c1[2]
    x = X.clone().requires_grad_()
    w = W.clone().requires_grad_()
    act = F.silu(d(st0.scale) * x + d(st0.shift)) if st0 is not None else x
    y = F.conv2d(act.permute(0, 3, 1, 2), w, padding=(K - 1) // 2, groups=X.shape[3])
    (y * dd.permute(0, 3, 1, 2)).sum().backward()
    gX = x.grad
    part = None
    if st0 is not None:
        gX = gX / d(st0.scale)       # the kernel returns dL/d(a0*x + b0): the BatchNorm-0 backward that follows carries the scale
        part = torch.stack([gX.sum((0, 1, 2)), (gX * X).sum((0, 1, 2))])
    elif residual is not None:
        gX = gX + residual.double()
    return gX, w.grad, part


def _fused_case(N, H, W, C, K, bn0, res):
    from muscle_amd import ops
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + H * 10 + C + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    dA, D, X = rn(N, H, W, C), rn(N, H, W, C), rn(N, H, W, C)
    gate, add = torch.sigmoid(rn(N, C)), rn(N, C) * 0.1
    mk = lambda: ops.BNState(torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1, rn(C) * 0.1, torch.rand(C, device=DEV, generator=g) + 0.5)
    st1, st0 = mk(), (mk() if bn0 else None)
    c1 = rn(3, C) * 0.3
    Wt = rn(C, 1, K, K) * 0.3
    residual = rn(N, H, W, C) if res else None
    want_gx, want_dw, want_part = _reference(dA, D, gate, add, st1, c1, X, st0, Wt, K, residual)
    outs = []
    for _ in range(2):
        dW = torch.zeros_like(Wt)
        gX, part = ops.dwconv_bwd_fused(dA, D, gate, add, st1, c1, X, st0, Wt, dW, K, (K - 1) // 2, residual=residual)
        outs.append((gX, dW, part))
    (gX, dW, part), (gX2, dW2, part2) = outs
    assert torch.equal(gX, gX2) and torch.equal(dW, dW2)                    # same bits every run (ordered partial rows, no atomics)
    assert float((gX.double() - want_gx).abs().max()) <= 2e-5 * float(want_gx.abs().max()) + 1e-6
    assert float((dW.double() - want_dw).abs().max()) <= 5e-5 * float(want_dw.abs().max()) + 1e-5
    if bn0:
        assert torch.equal(part, part2)
        got = part.double().sum(0)
        assert float((got - want_part).abs().max()) <= 5e-5 * float(want_part.abs().max()) + 1e-5
    else:
        assert part is None
    return part


@pytest.mark.parametrize("N,H,W,C,K,bn0,res", [
    (2, 28, 28, 64, 5, True, False), (2, 28, 28, 40, 3, True, False),       # 14 x 28 tiles (B7's 28 x 28 stages), ragged channels
    (3, 56, 56, 36, 5, True, False), (2, 56, 56, 32, 3, False, True),       # several tiles per plane; the plain-input (stage 1) form
    (2, 14, 28, 32, 5, True, False), (1, 42, 84, 16, 3, True, False),
    (2, 20, 37, 48, 5, True, False), (2, 20, 37, 20, 3, True, False),       # 8 x 16 tiles, image not a multiple of the tile
    (3, 9, 9, 32, 5, False, True), (2, 16, 16, 64, 3, False, False),
    (4, 112, 112, 32, 3, True, False), (2, 112, 112, 24, 5, True, False)])
def test_fused_depthwise_backward_matches_float64(N, H, W, C, K, bn0, res):
    _fused_case(N, H, W, C, K, bn0, res)


# 32 channel chunks leave 4096 / 32 = 128 groups (3x3), 1024 / 32 = 32 (5x5 on 8 x 16) or 512 / 32 = 16 (14 x 28) for the tile sequence
FUSED_MULTI = [
    (3, 72, 80, 1024, 3, True, False, 0, 45, 2),       # 8 x 16 / 3x3: 45 tiles per sample, 2 per group
    (3, 40, 40, 1024, 5, True, False, 0, 15, 2),       # 8 x 16 / 5x5
    (3, 40, 40, 1024, 5, False, True, 0, 15, 2),       # ... the plain-input + residual form (no BN0 rows)
    (3, 120, 84, 1024, 3, True, False, 3, 45, 2),      # 8 x 28 / 3x3, row-staged
    (5, 56, 56, 1024, 5, True, False, 1, 8, 3),        # 14 x 28 / 5x5: 8 tiles per sample, 3 per group
]


@pytest.mark.parametrize("N,H,W,C,K,bn0,res,shape,ntile,tpb", FUSED_MULTI)
def test_fused_depthwise_backward_multi_tile_groups(N, H, W, C, K, bn0, res, shape, ntile, tpb):
    from muscle_amd import ops
    geo = dw_geom.fused_geom(N, H, W, C, K)
    assert dw_geom.fused_shape(H, W, K) == shape and (geo.ntile, geo.tpb) == (ntile, tpb)
    assert geo.groups == ops.lib().mx_dwconv_bwd_fused_parts(N, H, W, C, K)
    dw_geom.assert_multi_tile(geo)
    part = _fused_case(N, H, W, C, K, bn0, res)
    if bn0:
        assert part.shape == (geo.groups, 2, C)


def _block_cfg(K, S, lo, hi):
    from muscle_amd.arch import BlockCfg
    return BlockCfg(index=1, cin=4, cexp=4, cout=4, kernel=K, stride=S, se=1, expand=True, skip=False, pad_lo=lo, pad_hi=hi, drop_rate=0.0)


def _forward_case(N, H, W, C, K, S, act, pads, Ho, Wo, multi=None):
    """pads: F.pad's (left, right, top, bottom) of the activated tensor; left == top is the kernel's pad_lo.
    multi: None | "stats" | "pooled" - the form whose several-tiles-per-workgroup geometry the case is built for."""
    from muscle_amd import ops
    L = ops.lib()
    pad_lo = pads[0]
    assert pads[2] == pad_lo
    if multi == "stats":
        geo = dw_geom.fwd_geom(N, Ho, Wo, C, S)
        assert geo.groups == L.mx_dwconv_fwd_parts(N, Ho, Wo, C, S)
        dw_geom.assert_multi_tile(geo)
    elif multi == "pooled":
        geo = dw_geom.fwd_geom(N, Ho, Wo, C, S, pooled=True)
        ws = L.mx_dwconv_fwd_ws(N, Ho, Wo, C, S)
        assert geo.gpp > 1 and geo.gpp * 4 * N * C == ws - dw_geom.WS_COUNTER_BYTES
        dw_geom.assert_multi_tile(geo)
    g = torch.Generator(device=DEV).manual_seed(N * 1000 + H * 10 + C + K + S)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    X = rn(N, H, W, C)
    Wt = rn(C, 1, K, K) * 0.3
    st = ops.BNState(torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1, rn(C) * 0.1, torch.rand(C, device=DEV, generator=g) + 0.5) if act else None
    x64 = X.double()
    if act:
        x64 = F.silu(st.scale.double() * x64 + st.shift.double())
    xp = F.pad(x64.permute(0, 3, 1, 2), pads)
    want = F.conv2d(xp, Wt.double(), stride=S, groups=C).permute(0, 2, 3, 1)
    assert want.shape == (N, Ho, Wo, C)
    outs = [ops.dwconv_fwd(X, Wt, K, S, pad_lo, Ho, Wo, st=st, want_stats=True) for _ in range(2)]
    (Y, stats), (Y2, stats2) = outs
    assert torch.equal(Y, Y2) and torch.equal(stats, stats2)
    assert float((Y.double() - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 1e-6
    ssum = stats.double().sum(0)
    assert float((ssum[0] - want.sum((0, 1, 2))).abs().max()) <= 2e-5 * float(want.abs().sum((0, 1, 2)).max()) + 1e-5
    assert float((ssum[1] - (want * want).sum((0, 1, 2))).abs().max()) <= 2e-5 * float((want * want).sum((0, 1, 2)).max()) + 1e-5
    # inference form: no statistics, the squeeze sums of swish(ps * y + pb) per sample instead
    ps, pb = torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1
    Yp, pooled = ops.dwconv_fwd(X, Wt, K, S, pad_lo, Ho, Wo, st=st, pool=(ps, pb))
    assert float((Yp.double() - want).abs().max()) <= 2e-6 * float(want.abs().max()) + 1e-6
    want_pool = F.silu(ps.double() * want + pb.double()).sum((1, 2))
    assert float((pooled.double() - want_pool).abs().max()) <= 2e-5 * float(want_pool.abs().max()) + 1e-5
    if multi == "pooled":
        # the groups of a sample are joined in group order by the last to arrive: the same bits every run, and every arrival
        # counter is left at zero for the next launch
        Yp2, pooled2 = ops.dwconv_fwd(X, Wt, K, S, pad_lo, Ho, Wo, st=st, pool=(ps, pb))
        assert torch.equal(Yp, Yp2) and torch.equal(pooled, pooled2)
        torch.cuda.synchronize()
        bufs = list(ops._scratch_bufs.values())
        assert bufs and all(int(b[:dw_geom.WS_COUNTER_BYTES].count_nonzero()) == 0 for b in bufs)


@pytest.mark.parametrize("N,H,W,C,K,S,act", [
    (2, 28, 28, 64, 5, 1, True), (2, 28, 28, 40, 3, 1, True), (3, 56, 56, 36, 5, 1, True), (2, 112, 112, 32, 3, 1, False),     # 8 x 28 row-staged tiles
    (1, 30, 84, 16, 5, 1, True), (2, 12, 28, 32, 3, 1, True),                                                                  # ... ragged rows
    (2, 20, 37, 48, 5, 1, True), (2, 16, 16, 20, 3, 1, False),                                                                 # 8 x 16 tiles
    (2, 56, 56, 32, 3, 2, True), (2, 28, 28, 24, 5, 2, True),                                                                  # stride 2 (TF 'same' padding)
    (2, 21, 37, 20, 5, 2, True), (2, 15, 15, 40, 3, 2, False)])                                                                # ... on an odd image: pad_lo (K-1)/2
def test_depthwise_forward_matches_float64(N, H, W, C, K, S, act):
    """mx_dwconv_fwd (model.py:76-79: BN0 + SiLU of the expand output applied while the tile is staged, depthwise convolution with
    TensorFlow 'same' padding, the BatchNorm-1 statistics as partial rows; eval mode: the SE squeeze sums instead) against float64, on
    both stride-1 tile shapes, stride 2, ragged images and channel counts."""
    Ho, Wo = (H + S - 1) // S, (W + S - 1) // S
    pt_h, pt_w = max((Ho - 1) * S + K - H, 0), max((Wo - 1) * S + K - W, 0)
    assert pt_h // 2 == pt_w // 2
    _forward_case(N, H, W, C, K, S, act, (pt_w // 2, pt_w - pt_w // 2, pt_h // 2, pt_h - pt_h // 2), Ho, Wo)


@pytest.mark.parametrize("K", [3, 5])
@pytest.mark.parametrize("N,H,W,C,act", [(3, 2, 2, 4, True), (2, 3, 2, 20, False), (2, 15, 15, 40, True), (2, 21, 37, 20, True),
                                         (1, 38, 50, 40, False), (3, 19, 25, 4, True)])
def test_depthwise_forward_stride2_model_padding(N, H, W, C, act, K):
    """The model freezes its pads at the nominal (even) size (arch.static_same_pad): multi-scale inference then feeds odd maps, and maps
    smaller than the kernel, with pad_lo = (K-1)/2 - 1 and Ho = floor(H/2) (BlockCfg.out_size)."""
    from muscle_amd.arch import static_same_pad
    lo, hi = static_same_pad(K, 2, 224)
    assert lo == (K - 1) // 2 - 1
    b = _block_cfg(K, 2, lo, hi)
    _forward_case(N, H, W, C, K, 2, act, (lo, hi, lo, hi), b.out_size(H), b.out_size(W))


def _tf_same(H, W, K, S):
    Ho, Wo = (H + S - 1) // S, (W + S - 1) // S
    pt_h, pt_w = max((Ho - 1) * S + K - H, 0), max((Wo - 1) * S + K - W, 0)
    assert pt_h // 2 == pt_w // 2
    return (pt_w // 2, pt_w - pt_w // 2, pt_h // 2, pt_h - pt_h // 2), Ho, Wo


@pytest.mark.parametrize("N,H,W,C,K,S,multi", [
    (3, 72, 80, 1024, 3, 1, "stats"),          # 16-wide tiles: 45 per sample, 2 per group
    (3, 120, 84, 1024, 5, 1, "stats"),         # 28-wide row-staged tiles: 45 per sample, 2 per group
    (3, 112, 112, 1024, 5, 2, "stats"),        # stride 2: 49 per sample, 2 per group
    (32, 80, 112, 128, 3, 2, "pooled"),        # groups do not straddle samples here: 35 tiles in 18 groups of 2, the last one short
    (32, 56, 80, 128, 5, 1, "pooled"),         # 16-wide: 35 tiles, 18 groups
    (32, 88, 84, 128, 3, 1, "pooled")])        # 28-wide: 33 tiles, 17 groups
def test_depthwise_forward_multi_tile_groups(N, H, W, C, K, S, multi):
    pads, Ho, Wo = _tf_same(H, W, K, S)
    _forward_case(N, H, W, C, K, S, True, pads, Ho, Wo, multi=multi)


@pytest.mark.parametrize("H,W", [(64, 64), (75, 101)])
@pytest.mark.parametrize("pad_lo", [0, 1])
def test_stem_im2col_is_unfold_of_the_padded_image(H, W, pad_lo):
    """mx_stem_im2col: rows (n, oy, ox), columns ci * 9 + ky * 3 + kx of the statically padded image, column 27 zero - copies only, so
    exact."""
    from muscle_amd import ops
    N, pad_hi = 2, 1                          # arch.static_same_pad(3, 2, nominal): (0, 1) at an even nominal size, (1, 1) at an odd one
    Ho, Wo = (H + pad_lo + pad_hi - 3) // 2 + 1, (W + pad_lo + pad_hi - 3) // 2 + 1
    g = torch.Generator(device=DEV).manual_seed(H + pad_lo)
    img = torch.randn(N, 3, H, W, device=DEV, generator=g)
    cols = ops.stem_im2col(img, Ho, Wo, pad_lo)
    want = F.unfold(F.pad(img, (pad_lo, pad_hi, pad_lo, pad_hi)), 3, stride=2)          # [N, 27, Ho * Wo]
    want = want.permute(0, 2, 1).reshape(N * Ho * Wo, 27)
    assert cols.shape == (N * Ho * Wo, 28)
    assert torch.equal(cols[:, :27], want)
    assert int(cols[:, 27].count_nonzero()) == 0
