"""Where the shapes of tests/test_gpu_bn_kernels.py land in the launch geometry of muscle_amd/csrc/bn.hip (col_geom / pool_geom),
through the two host-only queries mx_colreduce_parts and mx_pool_ws.  No kernel is launched.

The GPU cases were chosen for the branches they reach (fewer rows than one pass, a short last row block, a ragged last column
chunk, several row blocks per sample, the 4-at-a-time loop and the tail of the ordered join, 1000 partials).  If a retuning of
col_geom moves one of these values, the GPU cases must be chosen again so that they still reach those branches - do not just
update the numbers here."""
import pytest

from muscle_amd import _lib

COUNTER_BYTES = 65536      # MX_WS_COUNTER_BYTES: the arrival counters in front of the partials

# (rows, C) -> partial rows of the flat two-sum reductions (colstats, bn_bwd_reduce)
PARTS = {
    (1, 4): 1,                 # one float4, one row block
    (3, 36): 1,                # fewer rows than one pass of 28
    (1000, 36): 9,             # 9 row blocks of 112, the last 104 rows
    (130001, 36): 929,         # row blocks of 140, the last 81 rows
    (777, 1344): 25,           # row blocks of 32, the last 9 rows
    (5000, 1040): 105,         # row blocks of 48
    (9, 2304): 1,
}

# (rows, C, rows per sample) -> (scratch bytes, row blocks per sample)
POOL_WS_1 = {
    (600, 36, 300): (66400, 3),
    (22990, 1024, 22990): (4161536, 1000),
    (6274, 1344, 3137): (538624, 44),
    (147, 960, 49): (88576, 2),
    (40000, 128, 40000): (577536, 1000),
    (32, 1152, 16): (0, 1),    # one row block per sample: the plain-store path, no scratch
}
POOL_WS_5 = {
    (600, 36, 300): (69856, 3),
    (22990, 1024, 22990): (10530816, 511),
    (6274, 1344, 3137): (1248256, 22),
    (147, 960, 49): (180736, 2),
}


@pytest.mark.parametrize("shape,want", sorted(PARTS.items()))
def test_colreduce_parts_of_the_flat_shapes(shape, want):
    assert _lib.lib().mx_colreduce_parts(*shape) == want


@pytest.mark.parametrize("planes,table", [(1, POOL_WS_1), (5, POOL_WS_5)])
def test_pool_ws_of_the_per_sample_shapes(planes, table):
    L = _lib.lib()
    for (rows, C, rps), (want, blocks) in sorted(table.items()):
        got = L.mx_pool_ws(rows, C, rps, planes)
        assert got == want, (rows, C, rps, planes, got)
        if blocks > 1:      # counters, then [row blocks][planes][samples][C] fp32 partials
            assert want == COUNTER_BYTES + blocks * planes * (rows // rps) * C * 4


def test_geometry_queries_refuse_bad_shapes():
    L = _lib.lib()
    assert L.mx_colreduce_parts(0, 4) < 0 and L.mx_colreduce_parts(8, 6) < 0
    assert L.mx_pool_ws(10, 4, 3, 1) < 0 and L.mx_pool_ws(12, 4, 3, 2) < 0 and L.mx_pool_ws(12, 6, 3, 1) < 0
