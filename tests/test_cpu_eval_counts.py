"""CPU tests of the evaluation counting rule's restatement (tests/eval_counts_ref.py), which tests/test_gpu_eval_counts.py holds
every counting entry point to, and of the one threshold-list check of muscle_amd.evaluation."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import eval_counts_ref as R  # noqa: E402


def seeded_case(K, H, W, seed, nkeep=None):
    """(dict, gt, thresholds): values on a grid of eighths (ties between channels), among them negatives and the thresholds
    themselves (ties with the threshold); gt holds classes below K, values in K..254 and 255."""
    rng = np.random.RandomState(seed)
    thresholds = (0.0, 0.25, 0.5, 1.0)
    keys = sorted(rng.choice(K - 1, size=nkeep or max(1, (K - 1) // 2), replace=False).tolist())
    d = {int(k): (rng.randint(-2, 9, size=(H, W)) / 8.0).astype(np.float32) for k in keys}
    gt = rng.randint(0, K, size=(H, W)).astype(np.uint8)
    kind = rng.rand(H, W)
    gt[kind < 0.15] = 255
    gt[(kind >= 0.15) & (kind < 0.3)] = rng.randint(K, 255, size=int(((kind >= 0.15) & (kind < 0.3)).sum())).astype(np.uint8)
    return d, gt, thresholds


def test_restatement_equals_eval_compare_at_21_classes():
    from oracle.mcl_oracle import eval_compare
    for seed, (H, W) in enumerate(((1, 1), (1, 257), (37, 53))):
        d, gt, thresholds = seeded_case(21, H, W, seed, nkeep=2)         # two maps: their maximum is still negative somewhere
        stack = np.stack(list(d.values()))
        if H * W > 1:
            best = stack.max(axis=0)
            assert any((best == t).any() for t in thresholds) and (best < 0).any() and (gt == 255).any() and (gt < 21).any()
            assert ((stack == best).sum(axis=0) > 1).any() and ((gt >= 21) & (gt < 255)).any()
        for t in thresholds:
            TP, P, T = eval_compare(d, gt, t)
            assert np.array_equal(R.dict_counts(d, gt, t, 21), np.stack([TP, P, T], axis=1)), (H, W, t)
        assert np.array_equal(R.curve_counts(d, gt, thresholds, 21)[2], R.dict_counts(d, gt, thresholds[2], 21))


@pytest.mark.parametrize("K", [2, 5, 24])
def test_restatement_equals_a_brute_force_count(K):
    d, gt, thresholds = seeded_case(K, 9, 14, 40 + K)
    assert (gt < K).any() and ((gt >= K) & (gt < 255)).any() and (gt == 255).any()
    for t in thresholds:
        pred = R.dict_predict(d, t, K)
        want = np.zeros((K, 3), np.int64)
        for p, g in zip(pred.ravel().tolist(), gt.ravel().tolist()):
            if g != 255:
                want[p, 1] += 1
                if g < K:
                    want[g] += (int(p == g), 0, 1)
        assert np.array_equal(R.counts(pred, gt, K), want), t
        # the prediction itself, pixel by pixel: the first maximum of [t, v_1 .. v_{K-1}], absent channels 0
        for (y, x), p in np.ndenumerate(pred):
            col = [np.float32(t)] + [d[k][y, x] if k in d else np.float32(0) for k in range(K - 1)]
            assert p == col.index(max(col))
    assert np.array_equal(R.counts(np.full_like(gt, K), gt, K)[:, :2], np.zeros((K, 2), np.int64))       # a predict >= K counts nowhere


def test_half_dict_rounds_to_float16():
    pred = np.array([[[9.0]], [[0.1]], [[0.30005]]], np.float32)
    d = R.half_dict(pred, np.array([1, 1, 0], np.float32))
    assert sorted(d) == [0, 1] and d[0][0, 0] == np.float32(np.float16(0.1)) and d[1][0, 0] == 0 and d[0].dtype == np.float32


def test_threshold_lists_are_checked_in_one_place():
    from muscle_amd.evaluation import CamDictEval, check_thresholds
    from muscle_amd.irn_sweep import check_grid
    assert check_thresholds([0, 0.5, 0.5, 1], 21, "x") == (0.0, 0.5, 0.5, 1.0)
    assert len(check_thresholds([i / 64 for i in range(64)], 24, "x")) == 64 and check_thresholds((0.3,), 2, "x") == (0.3,)
    bad = ([], [i / 100 for i in range(65)], [-0.1, 0.2], [0.3, 0.2], [0.1, float("nan")], [float("nan")], [0.1, float("inf")])
    for who, make in (("CamDictEval", lambda t, k=21: CamDictEval("cpu", t, k)), ("irn_sweep", lambda t, k=21: check_grid((8,), (0,), t, k)),
                      ("anyone", lambda t, k=21: check_thresholds(t, k, "anyone"))):
        for t in bad:
            with pytest.raises(ValueError, match="^" + who):
                make(t)
        for k in (1, 25):
            with pytest.raises(ValueError, match="^" + who + ": num_cls"):
                make([0.2], k)
    with pytest.raises(ValueError, match="finite"):                      # refused by both callers; CamDictEval used to let a NaN through
        CamDictEval("cpu", [0.2, float("nan")])
    ev = CamDictEval("cpu", [0.0, 0.2], 5)
    assert ev.thresholds == (0.0, 0.2) and tuple(ev.counts.shape) == (2, 5, 3)
