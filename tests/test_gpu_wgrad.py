"""Small-output weight gradient (csrc/wgrad.hip) against an fp64 reference on the B7 first-stage shapes (scaled-down row
counts would not take the kernel: it needs R >= 65536), with the operand prologue, and its run-to-run determinism."""
import numpy as np
import pytest
import torch

from muscle_amd import synth

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


@pytest.mark.parametrize("R,Co,Ci,mode", [(100352, 288, 48, "plain"), (100352, 48, 288, "bnact"), (131072, 32, 32, "bnact"),
                                          (90000, 64, 28, "plain"), (80000, 192, 32, "plain"), (66000 + 7, 48, 192, "bnact"),
                                          (99999, 32, 64, "bnact"), (131072, 32, 32, "plain")])
def test_wgrad_small_matches_fp64_and_is_deterministic(R, Co, Ci, mode):
    from muscle_amd import ops
    from muscle_amd._lib import lib
    assert lib().mx_pw_wgrad_small_ws(R, Co, Ci, 1 if mode == "bnact" else 0) > 0
    g = torch.Generator(device=DEV).manual_seed(R + Co)
    G = torch.randn(R, Co, device=DEV, generator=g)
    X = torch.randn(R, Ci, device=DEV, generator=g)
    kw = {}
    Xr = X.double()
    if mode == "bnact":
        rps = 1000                                        # rows per sample: the gate changes inside slabs
        sc = torch.rand(Ci, device=DEV, generator=g) + 0.5
        sh = torch.randn(Ci, device=DEV, generator=g) * 0.3
        gate = torch.rand((R + rps - 1) // rps, Ci, device=DEV, generator=g)
        kw = dict(x_mode=ops.BNACT, x_scale=sc, x_shift=sh, x_gate=gate, rows_per_sample=rps)
        z = Xr * sc.double() + sh.double()
        Xr = z * torch.sigmoid(z) * gate.double().repeat_interleave(rps, dim=0)[:R]
    ref = G.double().t() @ Xr
    base = torch.randn(Co, Ci, device=DEV, generator=g)           # dW += : a running sum must be kept
    outs = []
    for _ in range(2):
        dW = base.clone()
        ops.pw_wgrad(G, X, dW, **kw)
        outs.append(dW)
    assert torch.equal(outs[0], outs[1])                          # fixed summation order
    err = (outs[0].double() - base.double() - ref).abs().max().item()
    scale = ref.abs().max().item()
    assert err <= 2e-5 * scale, (err, scale)
    # and the tiled (atomic) kernel agrees
    ops.WGRAD_SMALL = False
    try:
        dW2 = base.clone()
        ops.pw_wgrad(G, X, dW2, **kw)
    finally:
        ops.WGRAD_SMALL = True
    assert (dW2 - outs[0]).abs().max().item() <= 1e-4 * scale


@pytest.mark.parametrize("R,Co,Ci,mode", [(25088, 384, 2304, "plain"), (25088, 2304, 384, "bnact"), (12544, 960, 160, "plain"),
                                          (12544, 224, 1344, "bnact"), (25088, 640, 3840, "plain"), (1111, 200, 136, "bnact"),
                                          (2048, 128, 128, "plain"), (5000 + 3, 480, 80, "bnact"), (4096, 1344, 224, "affine")])
def test_wgrad_tile_matches_fp64_and_is_deterministic(R, Co, Ci, mode):
    """Large-output weight gradient (wgrad_tile_kernel): every tile shape (128/64 x 128/64), ragged rows and edges, the
    operand prologues, a running sum in dW, bit-identical repeat runs, agreement with the atomic TN GEMM it replaces."""
    from muscle_amd import ops
    from muscle_amd._lib import lib
    assert lib().mx_pw_wgrad_small_ws(R, Co, Ci, 1 if mode == "bnact" else 0) == 0
    assert lib().mx_pw_wgrad_tile_ws(R, Co, Ci, {'plain': 0, 'bnact': 1, 'affine': 2}[mode]) > 0
    g = torch.Generator(device=DEV).manual_seed(R + Co)
    G = torch.randn(R, Co, device=DEV, generator=g)
    X = torch.randn(R, Ci, device=DEV, generator=g)
    kw = {}
    Xr = X.double()
    if mode != "plain":
        rps = 49
        sc = torch.rand(Ci, device=DEV, generator=g) + 0.5
        sh = torch.randn(Ci, device=DEV, generator=g) * 0.3
        gate = torch.rand((R + rps - 1) // rps, Ci, device=DEV, generator=g)
        Xr = Xr * sc.double() + sh.double()
        if mode == "bnact":
            kw = dict(x_mode=ops.BNACT, x_scale=sc, x_shift=sh, x_gate=gate, rows_per_sample=rps)
            Xr = Xr * torch.sigmoid(Xr) * gate.double().repeat_interleave(rps, dim=0)[:R]
        else:
            kw = dict(x_mode=ops.AFFINE, x_scale=sc, x_shift=sh, rows_per_sample=rps)
    ref = G.double().t() @ Xr
    base = torch.randn(Co, Ci, device=DEV, generator=g)
    outs = []
    for _ in range(2):
        dW = base.clone()
        ops.pw_wgrad(G, X, dW, **kw)
        outs.append(dW)
    assert torch.equal(outs[0], outs[1])
    scale = ref.abs().max().item()
    err = (outs[0].double() - base.double() - ref).abs().max().item()
    assert err <= 2e-5 * scale, (err, scale)
    ops.WGRAD_TILE = False
    try:
        dW2 = base.clone()
        ops.pw_wgrad(G, X, dW2, **kw)
    finally:
        ops.WGRAD_TILE = True
    assert (dW2 - outs[0]).abs().max().item() <= 1e-4 * scale


@pytest.mark.parametrize("R,Co,Ci,pad", [(25088, 2304, 384, 0), (25107, 640, 2304, 0), (12551, 1344, 256, 0), (1024, 128, 128, 0), (2048, 256, 384, 64),
                                         (50176, 384, 640, 0), (4700, 512, 128, 32), (3136, 1280, 640, 0)])
def test_exact_fp32_wgrad_on_specialised_waves_vs_fp64(R, Co, Ci, pad):
    """wgrad_f32_ws_kernel (mx_set_gemm_mode(0), plain operands, outputs tiled 128 x 128): rows moved by range-checked LDS-DMA, one float per
    operand and lane into v_mfma_f32_32x32x2_f32.  Ragged row counts, a last tile of 64 columns, operands that are column slices of wider
    tensors (leading dimension > width), one / two / three 1568-row chains per group, a running sum in dW, the same bits on a second run -
    against fp64, held to the error of an fp32 dot product of that length."""
    from muscle_amd import ops
    from muscle_amd._lib import lib
    prev = ops.get_gemm_mode()
    ops.set_gemm_mode(0)
    try:
        assert lib().mx_pw_wgrad_small_ws(R, Co, Ci, 0) == 0 and lib().mx_pw_wgrad_tile_ws(R, Co, Ci, 0) > 0
        g = torch.Generator(device=DEV).manual_seed(R * 3 + Co + Ci)
        Gw = torch.randn(R, Co + pad, device=DEV, generator=g)
        Xw = torch.randn(R, Ci + pad, device=DEV, generator=g)
        G, X = Gw[:, :Co], Xw[:, pad:] if pad else Xw          # (the X slice starts `pad` columns in: a base pointer off the row start)
        ref = G.double().t() @ X.double()
        base = torch.randn(Co, Ci, device=DEV, generator=g)
        outs = []
        from muscle_amd._lib import call, ptr, stream
        need = lib().mx_pw_wgrad_tile_ws(R, Co, Ci, 0)
        ws = torch.zeros(need, dtype=torch.uint8, device=DEV)
        for _ in range(2):
            dW = base.clone()
            if pad:      # the C entry point takes the leading dimensions; the Python wrapper only hands over whole tensors
                call("mx_pw_wgrad_tile", G.data_ptr(), X.data_ptr(), 0, None, None, None, 1, ptr(dW), R, Co, Ci, G.stride(0), X.stride(0),
                     ws.data_ptr(), ws.numel(), stream())
            else:
                ops.pw_wgrad(G, X, dW)
            outs.append(dW)
        assert torch.equal(outs[0], outs[1])
        scale = ref.abs().max().item()
        err = (outs[0].double() - base.double() - ref).abs().max().item()
        assert err <= 2e-6 * scale + 4e-7 * float(R) ** 0.5 * 4.0, (err, scale)
    finally:
        ops.set_gemm_mode(prev)


def _gen1_tile(layout, M, N):
    """The first-generation GEMM's tile rule (gemm.hip pick_cfg), restated to derive the shapes below: BN of the 128 x BN tile."""
    if layout == "TN":
        return 128 if N >= 384 and N % 128 == 0 else 96 if N % 96 == 0 else 32
    best, best_score = 32, -1.0
    for bn, eff in ((128, 1.00), (96, 0.97), (64, 0.95), (32, 0.85)):
        if bn == 64 and N % 64:
            continue
        nt = -(-N // bn)
        per_cu = -(-M // 128) * nt / 256.0
        score = eff * (N / (nt * bn)) * (per_cu / int(per_cu + 0.999999)) * (0.85 if per_cu < 2.0 else 1.0)
        if score > best_score + 1e-9:
            best, best_score = bn, score
    return best


# One case per (layout, tile) the library compiles, at the smallest shape the rule above sends to that tile.
# TN (rows M = Co, columns N = Ci): the rule reads Ci alone - 384 (>= 384 and a multiple of 128), 96, 32; Co = 200 gives two
# row tiles, the second ragged.  R = 301 is one reduction slice, added straight into dW; R = 1101 is three slices of 384 rows
# (the last ragged) through the partial matrices and their in-order join.
# NN: searched over M tiles and N in steps of 4 for the smallest M * N per tile; M is then taken 5 rows short of the tile edge.
# 128 x 128 needs the wide tile's padding and balance to beat four times as many 128 x 32 workgroups, first at 193 row tiles and
# N = 100; 128 x 96 needs two full workgroups per CU (512 row tiles) at a width only it pads least, N = 68; 128 x 64 first wins
# at 43 row tiles x N = 192.  The second 128 x 64 shape (65 row tiles x 2 column tiles, 0.8 % larger) is the smallest that
# takes the XCD-ordered 1-D grid.  128 x 32 takes every small shape: three ragged row tiles x two column tiles, two batches.
# K = 20 / 36 are multiples of 4 (the NN contract) and not of 16: a ragged last K slab.
_GEN1_CASES = [("TN", 200, 384, 301, 128), ("TN", 200, 384, 1101, 128), ("TN", 200, 96, 301, 96), ("TN", 200, 96, 1101, 96),
               ("TN", 200, 32, 301, 32), ("TN", 200, 32, 1101, 32),
               ("NN", 24699, 100, 20, 128), ("NN", 65531, 68, 20, 96), ("NN", 5499, 192, 36, 64), ("NN", 8315, 128, 20, 64),
               ("NN", 333, 36, 20, 32)]


@pytest.mark.parametrize("layout,M,N,K,bn", _GEN1_CASES)
def test_first_generation_gemm_tiles_vs_fp64(layout, M, N, K, bn):
    """gemm_kernel (exact-fp32 MFMA, NN and TN) on each tile its dispatch instantiates, against numpy fp64, held to the
    bound of the exact-fp32 weight-gradient cases above (the error of an fp32 dot product of the reduction's length)."""
    from muscle_amd import ops
    assert _gen1_tile(layout, M, N) == bn
    g = torch.Generator(device=DEV).manual_seed(M * 3 + N + K)
    if layout == "TN":
        G = torch.randn(K, M, device=DEV, generator=g)
        X = torch.randn(K, N, device=DEV, generator=g)
        base = torch.randn(M, N, device=DEV, generator=g)          # dW += : the running sum must be kept
        ref = G.cpu().numpy().astype(np.float64).T @ X.cpu().numpy().astype(np.float64)
        out = base.clone()
        ops.WGRAD_SMALL = ops.WGRAD_TILE = False
        try:
            ops.pw_wgrad(G, X, out)
        finally:
            ops.WGRAD_SMALL = ops.WGRAD_TILE = True
        got = out.cpu().numpy().astype(np.float64) - base.cpu().numpy().astype(np.float64)
    else:
        nb = 2 if bn == 32 else 1
        A = torch.randn(nb, M, K, device=DEV, generator=g)
        B = torch.randn(nb, K, N, device=DEV, generator=g)
        ref = A.cpu().numpy().astype(np.float64) @ B.cpu().numpy().astype(np.float64)
        out = torch.full((nb, M, N), float("nan"), device=DEV)
        ops.bgemm(1, A, B, out, M, N, K)
        got = out.cpu().numpy().astype(np.float64)
    scale = float(np.abs(ref).max())
    err = float(np.abs(got - ref).max())               # (a NaN left in `out` fails the comparison below)
    print(f"{layout} M={M} N={N} K={K} tile 128x{bn}: err {err:.3g} scale {scale:.3g}")
    assert err <= 2e-6 * scale + 4e-7 * float(K) ** 0.5 * 4.0, (err, scale)
