"""The matrix-free IRN random walk, pinned on the CPU: tests/irn_walk_ref.py (the numpy restatement of csrc/irn_walk.hip) against
the reference's fixture tests/golden/irn_rw.npz and against the dense oracle (oracle.mcl_oracle.irn_propagate_to_edge) in fp64.

Bounds.  Against the fixture: 2e-4 of the output maximum, the tolerance tests/test_gpu_irn.py has for this comparison (the
fixture is the reference's fp32 result; the walk differs from it by the fixture's own error, 2.4e-5 / 4.3e-6 / 1.0e-5 for a / b /
c).  Against the fp64 oracle: e <= 2 e32 + 2e-7 with e32 = the fp32 oracle's own error on that input (the form of
tests/test_gpu_irn_net.py).  Every figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_walk_ref as WR  # noqa: E402

GOLD = os.path.join(os.path.dirname(__file__), "golden", "irn_rw.npz")


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def oracle_case(h, w, C, radius, beta, times, seed=7):
    """(x, edge, rw64, e32): synthetic input, the dense oracle in fp64 and the fp32 oracle's error against it."""
    from oracle import mcl_oracle as O
    from muscle_amd import synth
    x = torch.from_numpy(synth.uniform(seed, "irn_x", (1, C, h, w)).astype(np.float32))
    edge = torch.from_numpy(synth.uniform(seed, "irn_e", (1, h, w)).astype(np.float32)) ** 3
    r64 = O.irn_propagate_to_edge(x.double(), edge.double(), radius, beta, times).numpy()
    r32 = O.irn_propagate_to_edge(x, edge, radius, beta, times).numpy()
    return x.numpy(), edge.numpy(), r64, rel(r32, r64)


@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_restatement_vs_reference_fixture(tag):
    z = np.load(GOLD)
    radius, beta, times = (int(v) for v in z[f"{tag}_params"])
    rw = WR.walk(z[f"{tag}_x"], z[f"{tag}_edge"], radius, beta, times)
    ref = z[f"{tag}_rw"]
    assert rw.shape == ref.shape and rw.dtype == np.float32
    e = rel(rw, ref)
    print(f"[irn_walk] restatement vs fixture {tag}: {e:.3e} (limit 2e-4)")
    assert e <= 2e-4, (tag, e)


@pytest.mark.parametrize("h,w,C,radius,beta,times", [(31, 45, 20, 5, 10, 8), (3, 7, 1, 5, 10, 8), (16, 12, 3, 3, 10, 8)],
                         ids=["31x45", "3x7-smaller-than-radius", "16x12-radius3"])
def test_restatement_vs_fp64_oracle(h, w, C, radius, beta, times):
    x, edge, r64, e32 = oracle_case(h, w, C, radius, beta, times)
    e = rel(WR.walk(x, edge, radius, beta, times), r64)
    print(f"[irn_walk] restatement vs fp64 oracle {h}x{w} C={C} r={radius}: e {e:.3e}  e32 {e32:.3e}  bound {2 * e32 + 2e-7:.3e}")
    assert e <= 2 * e32 + 2e-7, (e, e32)


def test_fp32_state_is_not_enough():
    """Why the state is fp64 ("IRN random-walk propagation"): the same walk with an fp32 state is worse than the dense fp32
    oracle at 256 steps, the fp64 state two orders of magnitude better."""
    x, edge, r64, e32 = oracle_case(31, 45, 20, 5, 10, 8)
    e_f32 = rel(WR.walk(x, edge, 5, 10, 8, state_dtype=np.float32), r64)
    e_f64 = rel(WR.walk(x, edge, 5, 10, 8), r64)
    print(f"[irn_walk] 31x45, 256 steps: fp32 state {e_f32:.3e}  fp64 state {e_f64:.3e}  dense fp32 oracle {e32:.3e}")
    assert e_f64 < e32 < e_f32


def _oracle_dense(edge, radius):
    """The oracle's fp32 `dense` (its affinity matrix before the power), recovered through its public function: with beta = 1, no
    squaring and unit rows, rw[i][j] = (1 - e_i) dense[i][j] / colsum[j] and dense[j][j] = 1.  fp64, then rounded to fp32: exact
    when 1 - edge is exactly representable, which the caller's edge map (multiples of 1/256) makes it."""
    from oracle import mcl_oracle as O
    h, w = edge.shape
    n = h * w
    e = torch.from_numpy(edge).double()
    rw = O.irn_propagate_to_edge(torch.eye(n, dtype=torch.float64).reshape(n, 1, h, w), e.reshape(1, h, w), radius, 1, 0)
    t = (rw.reshape(n, n) / (1 - e.reshape(n, 1))).numpy()           # = dense / colsum
    return (t * (1.0 / np.diag(t))[None, :]).astype(np.float32)


def test_weights_are_the_oracles_scaled_matrix():
    """The stencil weights, placed into an n x n matrix, against `scaled = dense ** beta` of the oracle (mcl_oracle.py, the line after
    the path loop) in fp32: the same non-zero pattern exactly, values within 1 fp32 ulp.

    The 1-ulp comparison runs at beta 1 and 2, where both sides are correctly rounded.  At the scripts' beta (8, 10) torch.pow
    calls powf while the kernels multiply repeatedly (required, so that the weights equal the dense HIP path's entries bit for
    bit; the GPU test checks that): measured on 2e6 random values, the two differ by up to 5 ulp at beta 8 and 7 ulp at beta 10.
    There the pattern is still asserted exactly and the values against the exact power, within the 9 half-ulps that
    square-and-multiply can lose at beta 10 (x^2: 1, x^4: 3, x^8: 7, x^2 * x^8: 1 + 7 + 1)."""
    from muscle_amd import synth
    h, w, radius = 13, 17, 5
    edge = (np.floor(synth.uniform(3, "walk_e", (h, w)) ** 2 * 256) / 256).astype(np.float32)       # 0 .. 255/256, exact zeros included
    assert (edge == 0).any() and edge.max() < 1
    dense = _oracle_dense(edge, radius)
    for beta in (1, 2, 10):
        W, cs = WR.walk_weights(edge, radius, beta)
        mine = WR.dense_from_weights(W, radius)
        scaled = torch.pow(torch.from_numpy(dense), beta).numpy()
        assert ((mine != 0) == (scaled != 0)).all(), beta
        nz = scaled != 0
        ulps = float((np.abs(mine[nz].astype(np.float64) - scaled[nz]) / np.spacing(scaled[nz])).max())
        exact = dense[nz].astype(np.float64) ** beta
        half_ulps = float((np.abs(mine[nz] - exact) / exact).max() / 2.0 ** -24)
        csum = float(np.abs(cs.reshape(-1) - mine.astype(np.float64).sum(0)).max() / cs.max())
        print(f"[irn_walk] weights beta {beta}: {int(nz.sum())} non-zeros, {ulps:.1f} ulp from torch.pow, {half_ulps:.2f} x 2^-24 from "
              f"the exact power, cs vs column sums {csum:.2e}")
        if beta <= 2:
            assert ulps <= 1, (beta, ulps)
        assert half_ulps <= 9, (beta, half_ulps)
        assert csum <= 1e-12


def test_restatement_conserves_mass():
    """T is column-stochastic: an all-ones map with edge = 0 stays all ones."""
    one = WR.walk(np.ones((1, 9, 11), np.float32), np.zeros((9, 11), np.float32), 5, 10, 3)
    assert float(np.abs(one - 1).max()) <= 1e-6


def test_script_parses_walk_flag():
    from muscle_amd.infer_irn import parse_args
    base = ["--irn_weights_name", "w.pth", "--cam_dir", "cams"]
    assert parse_args(base).walk == "dense"
    assert parse_args(base + ["--walk", "stencil"]).walk == "stencil"
    with pytest.raises(SystemExit):
        parse_args(base + ["--walk", "sparse"])


def test_bad_method_and_exp_times_raise_before_any_launch():
    from muscle_amd import indexing
    x, e = torch.zeros(1, 1, 4, 5), torch.zeros(1, 4, 5)
    with pytest.raises(ValueError, match="method"):
        indexing.propagate_to_edge(x, e, method="sparse")
    for bad in (13, -1, 2.5):
        with pytest.raises(ValueError, match="exp_times"):
            indexing.propagate_to_edge(x, e, exp_times=bad, method="stencil")


def test_entry_points_report_argument_errors():
    """steps outside 1..4096, radius < 1 and null pointers are refused before any launch (no GPU needed)."""
    from muscle_amd import _lib
    L = _lib.lib()
    p = 4096                                                       # any non-null address: the checks come before the first use
    args = lambda **k: [k.get("x", p), p, p, p, 4, 5, k.get("radius", 5), p, p, p, 34, 1, k.get("steps", 1), p, p + 8, p, None]  # noqa: E731
    for kw, word in (({"steps": 0}, b"steps"), ({"steps": 4097}, b"steps"), ({"radius": 0}, b"radius"), ({"x": None}, b"null")):
        assert L.mx_irn_walk(*args(**kw)) < 0 and word in L.mx_last_error(), kw
    assert L.mx_irn_walk_weights(None, 4, 5, 5, p, p, p, 34, 10.0, p, p, None) < 0 and b"null" in L.mx_last_error()
    assert L.mx_irn_walk_weights(p, 4, 5, 0, p, p, p, 34, 10.0, p, p, None) < 0
    assert L.mx_irn_walk_ws(20, 1395) == 20 * 1395 * 8 and L.mx_irn_walk_ws(0, 5) < 0
