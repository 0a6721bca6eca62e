"""The fused backward of the small expand convs (ops.pw_bwd_fused / mx_pw_bwd_small_fused: dW += dZ^T X and dX = dZ W (+ residual) from one
pass over G and G2) against float64, beside the unfused pair in exact-fp32 arithmetic (bn_bwd_apply_plain, pw_dgrad, pw_wgrad on the same
inputs) under the project's rule e_got <= 1.5 e_ref + 3e-7 scale; every operand a row view with a leading dimension larger than its width,
dW pre-filled, guard rows behind dX, bit-identical from run to run, and dW bit for bit what pw_wgrad_bnbwd gives where the two kernels
cut the rows into the same groups (below 131 072 rows)."""
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.25
SHAPES = [(288, 48), (192, 32)]
ROWS = [1, 21, 64, 199, 4133]      # less than a slab, a ragged slab, one whole group, several groups with a ragged last one, many groups


def _view(rows, width, pad, g, fill=None):
    """[rows, width] view into a [rows, width + pad] buffer"""
    buf = torch.randn(rows, width + pad, device=DEV, generator=g) if fill is None else torch.full((rows, width + pad), fill, device=DEV)
    return buf, buf[:, :width]


def _inputs(R, Co, Ci, fold, res, seed):
    g = torch.Generator(device=DEV).manual_seed(seed)
    gbuf = torch.randn(2, R, Co + 8, device=DEV, generator=g)           # G and G2 share a leading dimension
    G, G2 = gbuf[0, :, :Co], (gbuf[1, :, :Co] if fold else None)
    coef = torch.stack([torch.rand(Co, device=DEV, generator=g) + 0.5, torch.randn(Co, device=DEV, generator=g) * 0.3,
                        torch.randn(Co, device=DEV, generator=g) * 0.1]).contiguous() if fold else None
    _, X = _view(R, Ci, 4, g)
    W = torch.randn(Co, Ci, device=DEV, generator=g) * (Co ** -0.5)
    dW0 = torch.randn(Co, Ci, device=DEV, generator=g)
    resbuf = torch.randn(R, Ci + 12, device=DEV, generator=g)
    return G, G2, coef, X, W, dW0, (resbuf[:, :Ci] if res else None)


def _run(G, G2, coef, X, W, dW0, res, **kw):
    from muscle_amd import ops
    R, Ci = X.shape
    buf = torch.full((R + 3, Ci + 12), SENTINEL, device=DEV)              # three guard rows and twelve guard columns of a sentinel
    dW = dW0.clone()
    dX = ops.pw_bwd_fused(G, G2, coef, X, W, dW, residual=res, out=buf[:R, :Ci], **kw)
    assert dX.data_ptr() == buf.data_ptr()
    return buf, dW


@pytest.mark.parametrize("fold,res", [(True, True), (True, False), (False, True), (False, False)])
@pytest.mark.parametrize("R", ROWS)
@pytest.mark.parametrize("Co,Ci", SHAPES)
def test_fused_backward_matches_fp64(Co, Ci, R, fold, res):
    import muscle_amd
    from muscle_amd import ops
    G, G2, coef, X, W, dW0, resv = _inputs(R, Co, Ci, fold, res, 1000 * Co + R + 2 * fold + res)
    dz64 = (coef[0].double() * G.double() + coef[1].double() * G2.double() + coef[2].double()) if fold else G.double()
    want_dx = dz64 @ W.double() + (resv.double() if res else 0)
    want_dw = dW0.double() + dz64.t() @ X.double()
    # the yardstick: the unfused pair in exact-fp32 arithmetic (GEMM mode 0) on the same inputs
    before = muscle_amd.get_gemm_mode()
    muscle_amd.set_gemm_mode(0)
    try:
        Gc = G.contiguous()
        dz = ops.bn_bwd_apply_plain(Gc, G2.contiguous(), coef, torch.empty_like(Gc)) if fold else Gc
        dx_ref = ops.pw_dgrad(dz, W, Ci, residual=resv.contiguous() if res else None)
        dw_ref = dW0.clone()
        ops.pw_wgrad(dz, X.contiguous(), dw_ref)
    finally:
        muscle_amd.set_gemm_mode(before)
    (buf, dW), (buf2, dW2) = _run(G, G2, coef, X, W, dW0, resv), _run(G, G2, coef, X, W, dW0, resv)
    assert torch.equal(buf, buf2) and torch.equal(dW, dW2)               # two runs, equal bits
    assert bool((buf[R:] == SENTINEL).all()) and bool((buf[:, Ci:] == SENTINEL).all())      # nothing behind row R - 1 or beside the rows
    for name, got, ref, want in (("dX", buf[:R, :Ci], dx_ref, want_dx), ("dW", dW, dw_ref, want_dw)):
        scale = float(want.abs().max())
        e_got, e_ref = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
        print(f"{name} Co={Co} Ci={Ci} R={R} fold={fold} res={res}: e_got={e_got:.3e} e_ref={e_ref:.3e} scale={scale:.3e}")
        assert e_got <= 1.5 * e_ref + 3e-7 * scale, (name, e_got, e_ref, scale)


@pytest.mark.parametrize("Co,Ci", SHAPES)
def test_deferred_reduce_gives_the_same_bits(Co, Ci):
    from muscle_amd import ops
    G, G2, coef, X, W, dW0, resv = _inputs(199, Co, Ci, True, True, 7 + Co)
    buf, dW = _run(G, G2, coef, X, W, dW0, resv)
    handed = []
    buf2, dW2 = _run(G, G2, coef, X, W, dW0, resv, defer=lambda part, dw: handed.append((part, dw)))
    assert len(handed) == 1 and torch.equal(dW2, dW0)                    # the kernel left dW alone
    part, dw = handed[0]
    assert part.shape[1] == Co * Ci and dw.data_ptr() == dW2.data_ptr()
    ops.pw_parts_reduce(part, dw)
    assert torch.equal(buf, buf2) and torch.equal(dW, dW2)


@pytest.mark.parametrize("Co,Ci", SHAPES)
def test_weight_gradient_half_is_bit_identical_to_the_split_pair(Co, Ci):
    """65 536 + 64 rows: the shortest reduction the small-output kernels take; both kernels cut it into the same row groups there."""
    from muscle_amd import ops, _lib
    R = 65536 + 64
    assert _lib.lib().mx_pw_wgrad_small_bnbwd_ok(R, Co, Ci) and _lib.lib().mx_pw_bwd_small_fused_ok(R, Co, Ci)
    assert _lib.lib().mx_pw_bwd_small_fused_groups(R, Co, Ci) * Co * Ci * 4 == _lib.lib().mx_pw_wgrad_small_ws(R, Co, Ci, 0)
    g = torch.Generator(device=DEV).manual_seed(Co)
    G, G2 = torch.randn(R, Co, device=DEV, generator=g), torch.randn(R, Co, device=DEV, generator=g)
    coef = torch.stack([torch.rand(Co, device=DEV, generator=g) + 0.5, torch.randn(Co, device=DEV, generator=g) * 0.3,
                        torch.randn(Co, device=DEV, generator=g) * 0.1]).contiguous()
    X = torch.randn(R, Ci, device=DEV, generator=g)
    W = torch.randn(Co, Ci, device=DEV, generator=g) * (Co ** -0.5)
    dW0 = torch.randn(Co, Ci, device=DEV, generator=g)
    want = dW0.clone()
    ops.pw_wgrad_bnbwd(G, G2, coef, X, want)
    got = dW0.clone()
    dX = ops.pw_bwd_fused(G, G2, coef, X, W, got)
    assert torch.equal(got, want)
    want_p, got_p = dW0.clone(), dW0.clone()
    ops.pw_wgrad(G, X, want_p)
    dXp = ops.pw_bwd_fused(G, None, None, X, W, got_p)
    assert torch.equal(got_p, want_p)
    # and the data gradient of a long reduction: a sample of rows against float64
    idx = torch.tensor([0, 1, 15, 16, 95, 96, 4097, R - 17, R - 1], device=DEV)
    dz64 = coef[0].double() * G[idx].double() + coef[1].double() * G2[idx].double() + coef[2].double()
    want_dx, want_dxp = dz64 @ W.double(), G[idx].double() @ W.double()
    # exact-fp32 chains of Co products of magnitude <= |dz| |W|: 1.5e-7 sum |a b| bounds a k-ordered fp32 chain of this length
    bound = 1.5e-7 * float((dz64.abs() @ W.double().abs()).max()) + 1e-7 * float(want_dx.abs().max())
    assert float((dX[idx].double() - want_dx).abs().max()) <= bound
    boundp = 1.5e-7 * float((G[idx].double().abs() @ W.double().abs()).max()) + 1e-7 * float(want_dxp.abs().max())
    assert float((dXp[idx].double() - want_dxp).abs().max()) <= boundp
