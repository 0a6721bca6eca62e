"""The unfused depthwise backward pair (mx_dwconv_bwd_data: dX = dwconv^T(dY) [+ residual], the gradient at the ACTIVATED input;
mx_dwconv_bwd_weight: dW += sum dY * act(X), act = silu(a0*X + b0) or identity) against float64 autograd of
F.conv2d(F.pad(act(X)), W, stride=S, groups=C): all four (K, S) instantiations of each kernel, ragged / several / exact tiles, both
pad_lo of each kernel size at stride 2, images smaller than the kernel, ragged and multiple channel chunks.  engine.block_route takes
this pair for a stride-2 block only with engine.DW_S2_FUSED off (tests/test_gpu_backbone.py runs that route end to end); the last test
here holds it against the fused stride-2 kernel that replaced it."""
import pytest
import torch
import torch.nn.functional as F

import dw_geom
from test_gpu_dwfused_s2 import CASES as S2_CASES, _inputs as s2_inputs, _reference as s2_reference, _swish_grad

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _geometry(kind, H, W, K):
    """(S, pad_lo, F.pad's (left, right, top, bottom), Ho, Wo)."""
    if kind == "s1":
        p = (K - 1) // 2
        return 1, p, (p, p, p, p), H, W
    if kind == "model":                 # the pads frozen at the nominal (even) size, whatever the map's own size
        from muscle_amd.arch import BlockCfg, static_same_pad
        lo, hi = static_same_pad(K, 2, 224)
        b = BlockCfg(index=1, cin=4, cexp=4, cout=4, kernel=K, stride=2, se=1, expand=True, skip=False, pad_lo=lo, pad_hi=hi, drop_rate=0.0)
        return 2, lo, (lo, hi, lo, hi), b.out_size(H), b.out_size(W)
    Ho, Wo = (H + 1) // 2, (W + 1) // 2                        # "tf": TensorFlow 'same' at the map's own (odd) size, the other pad_lo
    pt_h, pt_w = max((Ho - 1) * 2 + K - H, 0), max((Wo - 1) * 2 + K - W, 0)
    assert pt_h // 2 == pt_w // 2 == (K - 1) // 2
    return 2, pt_h // 2, (pt_w // 2, pt_w - pt_w // 2, pt_h // 2, pt_h - pt_h // 2), Ho, Wo


def _make(N, H, W, C, K, kind, seed=0):
    from muscle_amd import ops
    S, pad_lo, pads, Ho, Wo = _geometry(kind, H, W, K)
    g = torch.Generator(device=DEV).manual_seed(seed + N * 1000 + H * 10 + W + C + K)
    rn = lambda *s: torch.randn(*s, device=DEV, generator=g)
    X, dY, Wt, res = rn(N, H, W, C), rn(N, Ho, Wo, C), rn(C, 1, K, K) * 0.3, rn(N, H, W, C)
    st = ops.BNState(torch.rand(C, device=DEV, generator=g) + 0.5, rn(C) * 0.1, rn(C) * 0.1, torch.rand(C, device=DEV, generator=g) + 0.5)
    return (X, dY, Wt, res, st), (S, pad_lo, pads, Ho, Wo)


def _reference(X, dY, Wt, st, pads, S):
    """(gradient at the activated input, dW) in float64."""
    x = X.double()
    if st is not None:
        x = F.silu(st.scale.double() * x + st.shift.double())
    a = x.clone().requires_grad_()
    w = Wt.double().clone().requires_grad_()
    y = F.conv2d(F.pad(a.permute(0, 3, 1, 2), pads), w, stride=S, groups=X.shape[3])
    assert y.shape[2:] == dY.shape[1:3]
    (y * dY.double().permute(0, 3, 1, 2)).sum().backward()
    return a.grad, w.grad


def _check_weight(X, dY, Wt, st, K, S, pad_lo, pads):
    """dW += : a pre-filled dW keeps its values and takes the increment; two runs give the same bits (partial rows added in order)."""
    from muscle_amd import ops
    _, want_dw = _reference(X, dY, Wt, st, pads, S)
    g = torch.Generator(device=DEV).manual_seed(5)
    base = torch.randn(Wt.shape, device=DEV, generator=g)
    outs = []
    for _ in range(2):
        dW = base.clone()
        ops.dwconv_bwd_weight(X, dY, dW, K, S, pad_lo, st=st)
        outs.append(dW)
    assert torch.equal(outs[0], outs[1])
    err = float((outs[0].double() - base.double() - want_dw).abs().max())
    print(f"dW {err:.3e} / max {float(want_dw.abs().max()):.3e}")
    assert err <= 5e-5 * float(want_dw.abs().max()) + 1e-5


SIZES = [("s1", 9, 9), ("s1", 20, 37), ("s1", 16, 16),                                         # one ragged 8 x 16 input tile, several, exact
         ("model", 2, 2), ("model", 3, 2), ("model", 15, 15), ("model", 21, 37), ("model", 56, 56),
         ("tf", 15, 15), ("tf", 21, 37)]
# channels 4 / 20 (ragged chunk) / 40 (two chunks) and N = 1..3 go round over the cases, so that every (K, S) meets all of them
UNIT = [(1 + (i + j) % 3, H, W, (4, 20, 40)[(i + 2 * j) % 3], K, kind) for i, (kind, H, W) in enumerate(SIZES) for j, K in enumerate((3, 5))]


@pytest.mark.parametrize("N,H,W,C,K,kind", UNIT)
def test_unfused_backward_matches_float64(N, H, W, C, K, kind):
    from muscle_amd import ops
    (X, dY, Wt, res, st), (S, pad_lo, pads, Ho, Wo) = _make(N, H, W, C, K, kind)
    want_dx, _ = _reference(X, dY, Wt, None, pads, S)          # (linear in the activated input: the same with and without the prologue)
    for residual in (None, res):
        dX = ops.dwconv_bwd_data(dY, Wt, K, S, pad_lo, H, W, residual=residual)
        want = want_dx if residual is None else want_dx + residual.double()
        err = float((dX.double() - want).abs().max())
        print(f"dX {err:.3e} / max {float(want.abs().max()):.3e}")
        assert err <= 2e-5 * float(want.abs().max()) + 1e-6
    for prologue in (None, st):
        _check_weight(X, dY, Wt, prologue, K, S, pad_lo, pads)


@pytest.mark.parametrize("N,H,W,C,K,kind", [(2, 20, 37, 20, 3, "s1"), (2, 20, 37, 40, 5, "s1"), (3, 21, 37, 20, 3, "model"), (2, 21, 37, 40, 5, "model")])
def test_unfused_weight_gradient_stays_inside_its_scratch(N, H, W, C, K, kind):
    """The C entry with a scratch of exactly mx_dwconv_bwd_weight_parts rows: every row is written (a NaN left behind would reach dW)
    and nothing behind the last one is."""
    from muscle_amd import ops
    from muscle_amd._lib import call, ptr, stream
    (X, dY, Wt, _, st), (S, pad_lo, pads, Ho, Wo) = _make(N, H, W, C, K, kind, seed=1)
    rows = ops.lib().mx_dwconv_bwd_weight_parts(N, Ho, Wo, C, S)
    assert rows == dw_geom.bww_geom(N, Ho, Wo, C, S).groups
    n, guard = C * K * K, 3
    buf = torch.full((rows + guard, n), float("nan"), device=DEV)
    buf[rows:] = 12345.0
    dW = torch.zeros_like(Wt)
    call("mx_dwconv_bwd_weight", ptr(X), ptr(st.scale), ptr(st.shift), ptr(dY), ptr(dW), ptr(buf), N, H, W, C, K, S, pad_lo, Ho, Wo, stream())
    assert bool(torch.isfinite(dW).all()) and bool(torch.isfinite(buf[:rows]).all())
    assert bool((buf[rows:] == 12345.0).all())
    _, want_dw = _reference(X, dY, Wt, st, pads, S)
    assert float((dW.double() - want_dw).abs().max()) <= 5e-5 * float(want_dw.abs().max()) + 1e-5


# 2048 / 32 channel chunks = 64 groups for the (sample, tile) sequence
@pytest.mark.parametrize("N,H,W,C,K,kind,ntile,tpb", [
    (3, 56, 80, 1024, 3, "s1", 35, 2), (3, 56, 80, 1024, 5, "s1", 35, 2),                # 8 x 16 output tiles: 35 per sample, 2 per group
    (3, 112, 112, 1024, 3, "model", 49, 3), (3, 112, 112, 1024, 5, "model", 49, 3)])     # 8 x 8 output tiles of the 56 x 56 output: 49, 3 per group
def test_unfused_weight_gradient_multi_tile_groups(N, H, W, C, K, kind, ntile, tpb):
    """Several tiles per workgroup, a group running from one sample into the next, a short last group."""
    from muscle_amd import ops
    (X, dY, Wt, _, st), (S, pad_lo, pads, Ho, Wo) = _make(N, H, W, C, K, kind)
    geo = dw_geom.bww_geom(N, Ho, Wo, C, S)
    assert (geo.ntile, geo.tpb) == (ntile, tpb)
    assert geo.groups == ops.lib().mx_dwconv_bwd_weight_parts(N, Ho, Wo, C, S)
    dw_geom.assert_multi_tile(geo)
    _check_weight(X, dY, Wt, st, K, S, pad_lo, pads)


@pytest.mark.parametrize("N,H,W,C,K", S2_CASES)
def test_unfused_route_agrees_with_the_fused_stride2_kernel(N, H, W, C, K):
    """bn_backward_from_coeffs -> dwconv_bwd_weight(st=st0) + dwconv_bwd_data, times swish'(a0*X + b0), is what
    dwconv_bwd_fused_s2 computes in one pass: the two routes differ by no more than the sum of their own float64 bounds."""
    from muscle_amd import ops
    (dA, D, gate, add, st1, c1, X, st0, Wt), pad_lo, pads = s2_inputs(N, H, W, C, K)
    want_gx, want_dw, _ = s2_reference(dA, D, gate, add, st1, c1, X, st0, Wt, pads)
    Ho, Wo = D.shape[1:3]
    dW_f = torch.zeros_like(Wt)
    gX_f, _ = ops.dwconv_bwd_fused_s2(dA, D, gate, add, st1, c1, X, st0, Wt, dW_f, K, pad_lo)
    dd = ops.bn_backward_from_coeffs(dA.view(-1, C), D.view(-1, C), st1, c1, gate=gate, gate_add=add, rows_per_sample=Ho * Wo,
                                     out=torch.empty(N * Ho * Wo, C, device=DEV)).view(N, Ho, Wo, C)
    dW_u = torch.zeros_like(Wt)
    ops.dwconv_bwd_weight(X, dd, dW_u, K, 2, pad_lo, st=st0)
    gX_u = ops.dwconv_bwd_data(dd, Wt, K, 2, pad_lo, H, W).double() * _swish_grad(st0.scale.double() * X.double() + st0.shift.double())
    bound_gx = 2e-5 * float(want_gx.abs().max()) + 1e-6
    bound_dw = 5e-5 * float(want_dw.abs().max()) + 1e-5
    assert float((gX_u - gX_f.double()).abs().max()) <= 2 * bound_gx         # each route is held to `bound` against float64 on its own
    assert float((dW_u.double() - dW_f.double()).abs().max()) <= 2 * bound_dw
