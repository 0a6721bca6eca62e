"""CPU checks behind the phase-2 unit tests: the float64 references of tests/phase2_ref.py against the oracle's own
get_dynamic_crops / emd_dynamic, the host-side crop planner (muscle_amd.phase2._plan_crops) against the same oracle calls, and the
LDS arithmetic that decides which Sinkhorn kernel variant the pair tables of tests/test_gpu_phase2_kernels.py reach."""
import os
import re

import numpy as np
import pytest
import torch

import phase2_ref as R
from oracle import mcl_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---- references against the oracle ---------------------------------------------------------------------------------------------
# windows (h, w) of view 1 and recorded draws (lh, lw, sh, sw): an odd 15 x 15 window (view-2 crops pool to ONE pixel), 17 x 23,
# a stride above 28 (the view-1 crops are pooled too), a skipped sample (h < 15)
WINDOWS = [(15, 15), (17, 23), (90, 100), (14, 30)]
GEOMETRY = [(7, 7, 7, 7), (8, 11, 7, 8), (40, 45, 30, 25), None]


def _views(K=21, size=128, seed=5):
    g = torch.Generator().manual_seed(seed)
    n = len(WINDOWS)
    x1 = torch.rand(n, K, size, size, generator=g, dtype=torch.float64)
    x2 = torch.rand(n, K, size, size, generator=g, dtype=torch.float64)
    c1 = torch.tensor([[3 + b, 5 + 2 * b, h, w] for b, (h, w) in enumerate(WINDOWS)])
    c2 = torch.tensor([[7 + b, 1 + b, h, w] for b, (h, w) in enumerate(WINDOWS)])
    return x1, c1, x2, c2


def test_packed_crops_reproduce_the_oracle():
    x1, c1, x2, c2 = _views()
    o1, o2, ob = O.get_dynamic_crops(x1, c1, x2, c2, GEOMETRY)
    r1, r2, rb = R.packed_dynamic_crops(x1, c1, x2, c2, GEOMETRY)
    assert rb == ob == [0, 1, 2]
    shapes = [[tuple(c.shape) for c in s] for s in o1], [[tuple(c.shape) for c in s] for s in o2]
    assert shapes[0][0] == [(1, 21, 7, 7)] * 4 and shapes[1][0] == [(1, 21, 1, 1)] * 4          # 15 x 15: one-pixel view-2 crops
    assert shapes[0][2][0] == (1, 21, 7, 6) and shapes[1][2][0] == (1, 21, 11, 12)             # stride 30 x 25: pooled
    for ours, theirs in ((r1, o1), (r2, o2)):
        assert [len(s) for s in ours] == [len(s) for s in theirs]
        for sa, sb in zip(ours, theirs):
            for a, b in zip(sa, sb):
                assert a.shape == b.shape and a.dtype == b.dtype == torch.float64
                assert torch.equal(a, b)


def test_per_pair_emd_reproduces_emd_dynamic():
    """Scores per pair, the first minimum per sample, the mean over samples and the gradient of the chosen view-1 crop only
    (what phase2._EMD does with the kernels' results) against oracle.emd_dynamic on the same crops."""
    x1, c1, x2, c2 = _views(seed=6)
    x1, x2 = torch.nn.functional.normalize(x1, dim=1), torch.nn.functional.normalize(x2, dim=1)
    o1, o2, _ = O.get_dynamic_crops(x1, c1, x2, c2, GEOMETRY)
    o1 = [[c.clone().requires_grad_() for c in s] for s in o1]
    loss = O.emd_dynamic(o1, o2)
    loss.backward()
    total, ns = 0.0, len(o1)
    for s1, s2 in zip(o1, o2):
        res = [(i, R.emd_pair(R.pack(a.detach()), R.pack(b))) for i, a in enumerate(s1) for b in s2]
        scores = torch.stack([r[1][0] for r in res])
        best = int(torch.argmin(scores))                        # first minimum
        assert int((scores == scores[best]).sum()) == 1
        i, (sc, gx, _) = res[best]
        total = total + sc
        for q, a in enumerate(s1):
            if q != i:
                assert a.grad is None or not bool(a.grad.any())
        got = R.unpack(gx / ns, *s1[i].shape[2:])
        assert not bool(got[:, 21:].any())
        assert float((got[:, :21] - s1[i].grad).abs().max()) <= 1e-12 * float(s1[i].grad.abs().max())
    assert abs(float(total / ns) - float(loss.detach())) <= 1e-14 * abs(float(loss.detach()))


def test_sinkhorn_states_end_in_the_oracle_score():
    x, y = R.emd_features(49, 1), R.emd_features(272, 2)
    score, _, traj = R.emd_pair(x, y)
    assert traj.shape == (11, 49 + 272) and not bool(traj[0].any())
    cost = 1 - R.f64(x) @ R.f64(y).t()
    u, v = traj[10, :49], traj[10, 49:]
    pi = torch.exp((-cost + u[:, None] + v[None, :]) / 0.1)
    assert float(torch.sum(pi * cost) / pi.numel()) == float(score)


# ---- the planner ----------------------------------------------------------------------------------------------------------------
PLAN_WINDOWS = [(15, 15), (15, 23), (16, 75), (14, 30), (224, 224)]


@pytest.mark.parametrize("seed", [0, 1, 2, 3])
def test_plan_crops_follows_the_oracle(seed):
    from muscle_amd.phase2 import _plan_crops
    n = len(PLAN_WINDOWS)
    c1 = torch.tensor([[b, 2 * b, h, w] for b, (h, w) in enumerate(PLAN_WINDOWS)])
    c2 = torch.tensor([[3 + b, 1, h, w] for b, (h, w) in enumerate(PLAN_WINDOWS)])
    x = torch.zeros(n, 1, 240, 240, dtype=torch.float64)
    np.random.seed(seed)
    o1, o2, ob = O.get_dynamic_crops(x, c1, x, c2)
    np.random.seed(seed)
    p = _plan_crops(c1, c2, None)
    assert p.bidx == ob and 3 not in ob                                          # 14 x 30 is skipped
    assert 4 in ob                                                               # 224 x 224 always yields crops
    assert [[(h, w) for _, h, w in s] for s in p.per1] == [[tuple(c.shape[2:]) for c in s] for s in o1]
    assert [[(h, w) for _, h, w in s] for s in p.per2] == [[tuple(c.shape[2:]) for c in s] for s in o2]
    assert len(p.t1) == sum(len(s) for s in o1) and len(p.t2) == sum(len(s) for s in o2)
    # the pooled flag: every view-2 crop, and the view-1 crops with a resized side above 28
    pooled_in = {(r[0], r[1], r[2]) for r in p.pool}
    for t in p.t1:
        assert ((t[7], t[5], t[6]) in pooled_in) == (t[5] > 28 or t[6] > 28)
        assert t[1] >= c1[t[0], 0] and t[1] + t[3] <= c1[t[0], 0] + c1[t[0], 2] and t[2] + t[4] <= c1[t[0], 1] + c1[t[0], 3]
    for t in p.t2:
        assert (t[7], t[5], t[6]) in pooled_in and (t[3], t[4]) == (t[5], t[6])
    assert len(p.pool) == len(p.t2) + sum(t[5] > 28 or t[6] > 28 for t in p.t1)
    # offsets: the resized crops, then the pooled ones, back to back over [0, total)
    spans = sorted([(t[7], t[5] * t[6]) for t in p.t1 + p.t2] + [(r[3], (r[1] // 4) * (r[2] // 4)) for r in p.pool])
    end = 0
    for off, ln in spans:
        assert off == end and ln > 0
        end += ln
    assert end == p.total and p.nA == sum(t[5] * t[6] for t in p.t1 + p.t2)
    # every crop the pair table names is a final (pooled where flagged) crop; order = the oracle's enumeration
    want = [[o1_, h1 * w1, o2_, h2 * w2, s, 0] for s, (a, b) in enumerate(zip(p.per1, p.per2)) for (o1_, h1, w1) in a
            for (o2_, h2, w2) in b]
    assert p.pairs == want
    assert [r[1] for r in p.pairs] == [a.shape[2] * a.shape[3] for s1, s2 in zip(o1, o2) for a in s1 for _ in s2]
    assert [r[3] for r in p.pairs] == [b.shape[2] * b.shape[3] for s1, s2 in zip(o1, o2) for _ in s1 for b in s2]
    final = {(o, h, w) for s in p.per1 + p.per2 for (o, h, w) in s}
    assert all((r[3], r[1] // 4, r[2] // 4) in final for r in p.pool)
    assert all(((t[7], t[5], t[6]) in final) != ((t[7], t[5], t[6]) in pooled_in) for t in p.t1)


def test_plan_crops_one_pixel_view2_crops():
    """A window 15 to 23 pixels high gives view-2 crops of (h // 2) // 4 = 1 row: n2 = 1 reaches the Sinkhorn kernels."""
    from muscle_amd.phase2 import _plan_crops
    c = torch.tensor([[0, 0, 15, 15]])
    p = _plan_crops(c, c, [(7, 7, 7, 7)])
    assert [r[1] for r in p.pairs] == [49] * 16 and [r[3] for r in p.pairs] == [1] * 16


# ---- the LDS threshold ----------------------------------------------------------------------------------------------------------
FP, EMD_T, LDS_LIMIT = 24, 1024, 160 * 1024


def lds_bytes(n1, n2, grad, xg):
    """emd_lds of phase2.hip: floats of xs (unless XG), ys, u, v, lmu, lnu, tmp, pm, ps (+ the gradient's cl, ub, vb)."""
    f = ((0 if xg else n1) + n2) * FP + 2 * (n1 + n2) + n1 + 2 * EMD_T
    if grad:
        f += n1 + 2 * n2
    return 4 * f


def is_xg(sizes, grad):
    """The variant is chosen from the table-wide maxima."""
    return lds_bytes(max(a for a, _ in sizes), max(b for _, b in sizes), grad, False) > LDS_LIMIT


def slices(n_own):
    S = 1
    while S < 16 and 2 * S * n_own <= EMD_T:
        S *= 2
    return S


def test_lds_arithmetic_is_the_kernels():
    """The copy above is the expression in the source: a change of the layout has to come through here."""
    src = re.sub(r"\s+", " ", open(os.path.join(ROOT, "muscle_amd", "csrc", "phase2.hip")).read())
    assert ("size_t f = (size_t)((xg ? 0 : maxn1) + maxn2) * FP + 2 * (size_t)(maxn1 + maxn2) + (size_t)maxn1 + 2 * EMD_T; "
            "if (grad) f += (size_t)(maxn1 + 2 * maxn2); return f * sizeof(float);") in src
    assert "const int xg = emd_lds(maxn1, maxn2, 0, 0) > 160 * 1024;" in src and "const int xg = emd_lds(maxn1, maxn2, 1, 0) > 160 * 1024;" in src
    assert "constexpr int FP = 24;" in src and "constexpr int EMD_T = 1024;" in src and "constexpr int EMD_MAXS = 16;" in src
    assert "while (S < EMD_MAXS && 2 * S * n_own <= EMD_T) S *= 2;" in src


def test_emd_tables_fall_on_the_intended_side():
    for s in R.EMD_SINGLE:
        assert not is_xg([s], 0) and not is_xg([s], 1), s
    for s in R.EMD_FWD_LDS_GRAD_XG:
        assert not is_xg([s], 0) and is_xg([s], 1), s
        assert lds_bytes(*s, 1, True) <= LDS_LIMIT
    assert is_xg(R.EMD_MIXED_XG, 0) and is_xg(R.EMD_MIXED_XG, 1)
    assert lds_bytes(700, 784, 1, True) <= LDS_LIMIT
    assert is_xg([(784, 784)], 0) and is_xg([(784, 784)], 1)
    # the bands the issue names: n2 = 784 -> n1 in 606..686; n1 = n2 -> 695..734
    assert [n for n in range(1, 1025) if not is_xg([(n, 784)], 0) and is_xg([(n, 784)], 1)] == list(range(606, 687))
    assert [n for n in range(1, 1025) if not is_xg([(n, n)], 0) and is_xg([(n, n)], 1)] == list(range(695, 735))


def test_emd_tables_reach_the_slice_edges():
    """What each single-pair table is there for, from the slice arithmetic of emd_slice."""
    chunk = lambda n_own, n_other: -(-n_other // slices(n_own))          # noqa: E731
    assert slices(1) == 16 and slices(49) == 16 and slices(63) == 16 and slices(64) == 16 and slices(65) == 8
    assert slices(512) == 2 and slices(513) == 1 and slices(1024) == 1 and slices(272) == 2
    sizes = set(R.EMD_SINGLE)
    assert {(1, 1), (1, 49), (49, 1)} <= sizes                                                   # n_own = 1
    assert any(n2 < slices(n1) for n1, n2 in sizes) and any(n1 < slices(n2) for n1, n2 in sizes)   # empty slices both ways
    assert (3, 5) in sizes and 5 < slices(3)
    assert {63, 64, 65, 512, 513} <= {n for s in sizes for n in s}
    assert any(chunk(a, b) % 4 for a, b in sizes) and any(chunk(b, a) % 4 for a, b in sizes)      # the 4-wide unroll's remainder
    assert any(chunk(a, b) >= 4 and chunk(a, b) % 4 for a, b in sizes)                             # ... after at least one full group
