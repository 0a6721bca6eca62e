"""Pins tests/irn_dense_ref.py, the restatement tests/test_gpu_irn_dense.py holds the dense IRN kernels to, and checks on the
CPU the conditions those GPU tests rely on.  No GPU needed.

  walk (fp64)          vs the oracle's irn_propagate_to_edge in fp64, 31 x 45, exp_times 0 / 1 / 8        <= 1e-12 of the maximum
  walk (fp64)          vs the reference's fixture tests/golden/irn_rw.npz (three cases)                   <= 2e-4, the GPU test's bound
  finish_values (fp64) vs F.interpolate in fp64 (the arithmetic of the oracle's irn_finish)               <= 1e-12
  search_paths         == muscle_amd.indexing.search_paths, radius 2 / 3 / 5 / 8
  affinity             symmetric, unit diagonal;  T: columns sum to 1 within 1e-12, zero pattern of the affinity
  ambiguity            share of pixels whose two best of [bg_thres, v_1..v_C] lie within tau = 2 e32 + 2e-7 in fp64  <= 1e-3

Measured here (bg_thres 0.25; the ambiguous share is also taken at the looser 4 e32 + 1e-7):

  case (C,h,w,H,W)            e32        tau        ambiguous share (tau)   (4 e32 + 1e-7)
  (20,19,23,74,90)            1.644e-07  5.287e-07  0                       0
  (20,19,23,76,92)            1.621e-07  5.242e-07  0                       0
  (1,1,1,1,1)                 0          2.000e-07  0                       0
  (3,1,9,4,33)                9.187e-08  3.837e-07  0                       0
  (3,9,1,33,4)                9.187e-08  3.837e-07  0                       0
  (254,3,3,12,12)             1.320e-07  4.639e-07  0                       0
  (5,128,128,512,512)         1.353e-07  4.706e-07  0                       0
  (1,257,256,1025,1024)       1.690e-07  5.380e-07  3.811e-06               4.764e-06

  restatement vs oracle in fp64, 31 x 45, exp_times 0 / 1 / 8: 2.1e-15 / 3.4e-15 / 2.9e-13;  vs the fixture a / b / c: 2.4e-05 /
  4.3e-06 / 1.0e-05;  finish_values vs F.interpolate in fp64: <= 1.2e-16.
"""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_dense_ref as D  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden")
BG = 0.25
AMBIGUOUS_CAP = 1e-3


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def synth_case(h, w, C, seed=7):
    from muscle_amd import synth
    x = synth.uniform(seed, "irn_x", (1, C, h, w)).astype(np.float32)
    edge = synth.uniform(seed, "irn_e", (1, h, w)).astype(np.float32) ** 3
    return x, edge


@pytest.mark.parametrize("radius", [2, 3, 5, 8])
def test_search_paths_equal_the_products(radius):
    from muscle_amd.indexing import search_paths
    mine, theirs = D.search_paths(radius), search_paths(radius)
    assert [[tuple(p) for p in path] for path in mine] == [[tuple(p) for p in path] for path in theirs]
    assert all(path[0] == max(path, key=lambda p: abs(p[0]) + abs(p[1])) for path in mine)      # the destination comes first


@pytest.mark.parametrize("times", [0, 1, 8])
def test_walk_fp64_equals_the_oracle(times):
    from oracle import mcl_oracle as O
    x, edge = synth_case(31, 45, 20)
    ref = O.irn_propagate_to_edge(torch.from_numpy(x).double(), torch.from_numpy(edge).double(), 5, 10, times).numpy()
    mine = D.walk(x, edge, 5, 10, times, np.float64)
    assert mine.shape == ref.shape and mine.dtype == np.float64
    e = rel(mine, ref)
    print(f"[irn_dense] restatement vs oracle, fp64, 31x45 exp_times {times}: {e:.3e}")
    assert e <= 1e-12, e


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_walk_fp64_vs_reference_fixture(tag):
    z = np.load(os.path.join(GOLD, "irn_rw.npz"))
    radius, beta, times = (int(v) for v in z[f"{tag}_params"])
    mine = D.walk(z[f"{tag}_x"], z[f"{tag}_edge"], radius, beta, times, np.float64)
    assert mine.shape == z[f"{tag}_rw"].shape
    e = rel(mine, z[f"{tag}_rw"])
    print(f"[irn_dense] restatement (fp64) vs fixture {tag}: {e:.3e}  (limit 2e-4)")
    assert e <= 2e-4, (tag, e)


@pytest.mark.parametrize("C,h,w,H,W", [c for c in D.FINISH_CASES if c[3] * c[4] <= 100000], ids=str)
def test_finish_values_fp64_equal_interpolate(C, h, w, H, W):
    from muscle_amd import synth
    rw = D.finish_input(synth.uniform, C, h, w)
    up = F.interpolate(torch.from_numpy(rw).double(), scale_factor=4, mode="bilinear", align_corners=False)[:, 0, :H, :W]
    assert float(np.abs(D.upsample4(rw, H, W, np.float64) - up.numpy()).max()) <= 1e-12 * float(up.max())
    ref = (up / torch.max(up)).numpy()
    mine = D.finish_values(rw, H, W, np.float64)
    d = float(np.abs(mine - ref).max())
    print(f"[irn_dense] finish_values vs F.interpolate, fp64, {(C, h, w, H, W)}: {d:.3e}")
    assert mine.shape == (C, H, W) and d <= 1e-12, d


@pytest.mark.parametrize("h,w,radius", [(13, 17, 5), (31, 45, 5), (3, 7, 5), (1, 9, 5), (9, 1, 5), (1, 1, 5), (16, 12, 3),
                                        (6, 5, 2), (10, 11, 8)])
def test_affinity_and_transition_properties(h, w, radius):
    _, edge = synth_case(h, w, 1, seed=5)
    edge[0, 0, 0] = 1.0
    edge[0, h // 2, w // 2] = 0.0
    for dtype in (np.float64, np.float32):
        A = D.affinity(edge, radius, dtype)
        assert A.dtype == dtype and A.shape == (h * w, h * w)
        assert np.array_equal(A, A.T) and (np.diag(A) == 1).all() and A.min() >= 0 and A.max() <= 1
    A32, A64 = D.affinity(edge, radius, np.float32), D.affinity(edge, radius, np.float64)
    assert np.array_equal(A32, A64.astype(np.float32))          # one subtraction of an fp32 maximum: fp32 is the rounded fp64
    # every non-zero lies inside the search disc
    f, t = np.nonzero(A64)
    dy, dx = t // w - f // w, t % w - f % w
    assert (dy * dy + dx * dx < radius * radius).all()
    for beta in (10, 2.5):
        scaled, colsum, T = D.transition(A64, beta, np.float64)
        assert float(np.abs(T.sum(axis=0) - 1).max()) <= 1e-12
        assert np.array_equal(T != 0, A64 != 0)
        assert np.array_equal(scaled.sum(axis=0), colsum)


@pytest.mark.parametrize("C,h,w,H,W", D.FINISH_CASES, ids=str)
def test_ambiguous_share_is_far_inside_the_cap(C, h, w, H, W):
    """The GPU test accepts either of two labels where the fp64 values lie within tau of each other; that rule means something
    only while such pixels are rare, which is a property of the inputs and is shown here."""
    from muscle_amd import synth
    rw = D.finish_input(synth.uniform, C, h, w)
    v64 = D.finish_values(rw, H, W, np.float64)
    e32 = float(np.abs(D.finish_values(rw, H, W, np.float32).astype(np.float64) - v64).max())
    tau = 2 * e32 + 2e-7
    _, _, _, gap = D.top_two(v64, BG)
    share, loose = float((gap <= tau).mean()), float((gap <= 4 * e32 + 1e-7).mean())
    print(f"[irn_dense] ambiguity {(C, h, w, H, W)}: e32 {e32:.3e}  tau {tau:.3e}  share {share:.3e}  at 4 e32 + 1e-7: {loose:.3e}")
    assert share <= AMBIGUOUS_CAP and loose <= AMBIGUOUS_CAP, (share, loose)
    if C == 254:
        assert (D.top_two(v64, BG)[1] == 254).any()
