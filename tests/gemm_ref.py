"""Plain restatements of the forward / data-gradient GEMMs of muscle_amd/csrc/gemm.hip, CPU only (torch / numpy): the operand
prologues, the epilogue, the per-128-row-tile column statistics, and the layout of the pre-split weight image
(split_planes_kernel).  `dtype` is float64 for the reference and float32 for the yardstick e32."""
import numpy as np
import torch

PLAIN, BNACT, AFFINE, BNBWD = 0, 1, 2, 3
TILE_M = 128                                   # every tile of the NT family has 128 rows (mx_pw_fwd_parts)


def prologue(a_mode, A, *, scale=None, shift=None, gate=None, rps=1, X=None, coef=None, dtype=torch.float64):
    """A' of C = A' W^T.  PLAIN: A; AFFINE: sc*a + sh; BNACT: swish(sc*a + sh) * gate[row // rps]; BNBWD: c1*g + c2*x + c3
    (A = G, coef = [3, K])."""
    A = A.to(dtype)
    if a_mode == PLAIN:
        return A
    if a_mode == BNBWD:
        c = coef.to(dtype)
        return c[0] * A + c[1] * X.to(dtype) + c[2]
    v = A * scale.to(dtype) + shift.to(dtype)
    if a_mode == AFFINE:
        return v
    v = v * torch.sigmoid(v)
    if gate is not None:
        rows = torch.arange(A.shape[0]) // rps
        v = v * gate.to(dtype)[rows]
    return v


def epilogue(C, bias=None, residual=None, relu=False):
    if bias is not None:
        C = C + bias.to(C.dtype)
    if residual is not None:
        C = C + residual.to(C.dtype)
    if relu:
        C = C.clamp_min(0)
    return C


def gemm(Ap, W, bias=None, residual=None, relu=False):
    """epilogue(A' W^T) in the dtype of A'."""
    return epilogue(Ap @ W.to(Ap.dtype).t(), bias, residual, relu)


def tile_stats(C):
    """Per 128-row tile t and column: the float64 sum and sum of squares of the values in C [M, N] (the float32 values a kernel
    stored), and sum |c| for the a-priori bound of the tile's fp32 additions.  -> (sum [P, N], sumsq [P, N], sumabs [P, N])."""
    M, N = C.shape
    P = (M + TILE_M - 1) // TILE_M
    pad = torch.zeros(P * TILE_M, N, dtype=torch.float64, device=C.device)
    pad[:M] = C.double()
    t = pad.view(P, TILE_M, N)
    return t.sum(1), (t * t).sum(1), t.abs().sum(1)


STATS_EPS = (TILE_M + 8) * 2.0 ** -24          # 128 fp32 additions per column of a tile, and the cross-wave adds


# ---- the pre-split weight image (split_planes_kernel) --------------------------------------------------------------------------
# For W [N, K], K % 16 == 0: Npad = N rounded up to 128, KT = ceil(K / 32) K steps.  The image is bf16 [KT][3 planes][Npad][4][8]:
# 16-byte chunk c' of row n holds chunk c = c' ^ (3 * bit 3 of n) of the K step; element e of chunk c is term p (h, m, l) of
# W[n][32 kt + 4 c + e] for e < 4 and of W[n][32 kt + 16 + 4 c + (e - 4)] for e >= 4.  Rows n >= N and columns k >= K are zero.
# The three terms are the truncation split: h = the top 16 bits of w, m = the top 16 bits of w - h, l = those of w - h - m.
def planes_bytes(N, K):
    if N <= 0 or K <= 0 or K % 16:
        return -1
    return ((N + 127) // 128 * 128) * ((K + 31) // 32 * 32) * 6


def planes_tiles(N, K):
    if N <= 0 or K <= 0 or K % 16:
        return -1
    return ((N + 127) // 128 * 128 // 64) * ((K + 31) // 32)


def _image_index(N, K):
    """k[n, c', e] of the image slot (the same for every K step, plus 32 kt) as an int array [Npad, 4, 8]"""
    Npad = (N + 127) // 128 * 128
    n = np.arange(Npad)[:, None, None]
    cp = np.arange(4)[None, :, None]
    e = np.arange(8)[None, None, :]
    c = cp ^ (((n >> 3) & 1) * 3)
    return 4 * c + np.where(e < 4, e, 12 + e)


def planes_decode(image, N, K):
    """image: uint8 array of planes_bytes(N, K) bytes -> float32 [3, Npad, Kpad], the three terms at their (n, k) positions."""
    Npad, KT = (N + 127) // 128 * 128, (K + 31) // 32
    img = np.frombuffer(np.ascontiguousarray(image).tobytes(), dtype=np.uint16).reshape(KT, 3, Npad, 4, 8)
    kin = _image_index(N, K)
    out = np.zeros((3, Npad, KT * 32), dtype=np.uint32)
    rows = np.broadcast_to(np.arange(Npad)[:, None, None], kin.shape)
    for kt in range(KT):
        for p in range(3):
            out[p, rows, 32 * kt + kin] = img[kt, p].astype(np.uint32) << 16
    return out.view(np.float32)


def planes_encode(W):
    """The image of a float32 weight [N, K] as split_planes_kernel writes it -> uint8 array."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    N, K = W.shape
    Npad, KT = (N + 127) // 128 * 128, (K + 31) // 32
    full = np.zeros((Npad, KT * 32), dtype=np.float32)
    full[:N, :K] = W
    terms, rest = [], full
    for _ in range(3):
        t = (rest.view(np.uint32) & np.uint32(0xFFFF0000)).view(np.float32)
        terms.append(t)
        rest = rest - t                                   # exact
    kin = _image_index(N, K)
    rows = np.broadcast_to(np.arange(Npad)[:, None, None], kin.shape)
    img = np.zeros((KT, 3, Npad, 4, 8), dtype=np.uint16)
    for kt in range(KT):
        for p in range(3):
            img[kt, p] = (terms[p][rows, 32 * kt + kin].view(np.uint32) >> 16).astype(np.uint16)
    return np.frombuffer(img.tobytes(), dtype=np.uint8)


def check_planes_image(image, W):
    """The image decodes back to the weight exactly: h + m + l == w bit for bit, every term has at most 8 significant bits in bf16
    form (by construction of the decode), zero rows past N and zero columns past K."""
    W = np.ascontiguousarray(W, dtype=np.float32)
    N, K = W.shape
    t = planes_decode(image, N, K)
    total = (t[0].astype(np.float64) + t[1].astype(np.float64) + t[2].astype(np.float64)).astype(np.float32)
    assert np.array_equal(total[:N, :K].view(np.uint32), W.view(np.uint32)), "h + m + l != w"
    assert not t[:, N:, :].view(np.uint32).any(), "rows past N are not zero"
    assert not t[:, :, K:].view(np.uint32).any(), "columns past K are not zero"
