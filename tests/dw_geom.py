"""The depthwise kernels' launch geometry (muscle_amd/csrc/dwconv.hip: dw_fwd_geom, dw_fused_shape / dw_fused_geom,
dw_fused_s2_groups with the launch's tiles_x / tiles_y, dw_bww_geom), restated to derive the multi-tile cases of
tests/test_gpu_dwfused.py, test_gpu_dwfused_s2.py and test_gpu_dw_unfused.py.  A workgroup walks `tpb` consecutive tiles of the
(sample, tile) sequence; every case built on these functions first asserts the group count against the library's own
mx_dwconv_*_parts, so a changed target in the kernel file breaks the case instead of quietly taking it off the path it is for."""
from typing import NamedTuple

CB = 32                      # channels per workgroup
WS_COUNTER_BYTES = 65536     # the arrival counters in front of the pooled forward's scratch


def cdiv(a, b):
    return -(-a // b)


class Geom(NamedTuple):
    tiles_x: int
    tiles_y: int
    tpb: int         # tiles per workgroup
    groups: int      # workgroups per channel chunk = partial rows
    gpp: int = 0     # pooled forward: groups per sample

    @property
    def ntile(self):
        return self.tiles_x * self.tiles_y


def fwd_geom(N, Ho, Wo, C, S, pooled=False):
    tw = 28 if (S == 1 and Wo % 28 == 0) else 16 if S == 1 else 8
    tx, ty = cdiv(Wo, tw), cdiv(Ho, 8)
    ntile, chunks = tx * ty, cdiv(C, CB)
    g = min(max(4096 // chunks, 1), N * ntile)
    if pooled:
        per = min(max(g // N, 1), ntile)          # (N * chunks <= the 16384 arrival counters in every case here)
        tpb = cdiv(ntile, per)
        gpp = cdiv(ntile, tpb)
        return Geom(tx, ty, tpb, N * gpp, gpp)
    tpb = cdiv(N * ntile, g)
    return Geom(tx, ty, tpb, cdiv(N * ntile, tpb))


def fused_shape(H, W, K):
    """0 = 8 x 16 tiles, 1 = 14 x 28 (5x5), 3 = 8 x 28 (3x3)."""
    if K != 5:
        return 3 if W % 28 == 0 else 0
    small = cdiv(H, 8) * cdiv(W, 16) * (8 + K - 1) * (16 + K - 1)
    large = cdiv(H, 14) * cdiv(W, 28) * (14 + K - 1) * (28 + K - 1)
    return 1 if large < 0.9 * small else 0


def fused_geom(N, H, W, C, K):
    shape = fused_shape(H, W, K)
    tx, ty = cdiv(W, 28 if shape else 16), cdiv(H, 14 if shape == 1 else 8)
    ntiles, chunks = N * tx * ty, cdiv(C, CB)
    target = 4096 if shape == 3 else 512 if shape else 1024 if K == 5 else 4096
    g = min(max(target // chunks, 1), ntiles)
    tpb = cdiv(ntiles, g)
    return Geom(tx, ty, tpb, cdiv(ntiles, tpb))


def fused_s2_geom(N, H, W, C, K, pad_lo):
    """groups from the unshifted tiling (the count must not know pad_lo), tiles from the launch's: origins at 8 ty - (pad_lo & 1)."""
    ntiles = N * cdiv(W, 32) * cdiv(H, 8)
    g = min(max((2048 if K == 5 else 4096) // cdiv(C, CB), 1), 1024, ntiles)
    groups = cdiv(ntiles, cdiv(ntiles, g))
    tx, ty = cdiv(W + (pad_lo & 1), 32), cdiv(H + (pad_lo & 1), 8)
    return Geom(tx, ty, cdiv(N * tx * ty, groups), groups)


def bww_geom(N, Ho, Wo, C, S):
    tx, ty = cdiv(Wo, 16 if S == 1 else 8), cdiv(Ho, 8)
    ntiles = N * tx * ty
    g = min(max(2048 // cdiv(C, CB), 1), ntiles)
    tpb = cdiv(ntiles, g)
    return Geom(tx, ty, tpb, cdiv(ntiles, tpb))


def assert_multi_tile(geo: Geom):
    """The case is on the several-tiles-per-workgroup loop, and a group straddles two samples (or, pooled, the last group of a sample
    is short)."""
    assert geo.tpb > 1 and geo.ntile % geo.tpb != 0, geo
