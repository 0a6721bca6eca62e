"""GPU tests of the CAM-dict evaluation (mx_camdict_confusion, evaluation.CamDictEval): integer (TP, P, T) tables for the 60
thresholds of src/evaluation.py:126-133 from one launch per image.  Integer work: the counts must be exact."""
import os

import numpy as np
import pytest
import torch

pytestmark = [pytest.mark.gpu]
DEV = "cuda:0"
CURVE = [i / 100.0 for i in range(60)]
GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "eval_curve.npz")


def _gt(seed, H, W):
    rng = np.random.default_rng(seed)
    g = rng.integers(0, 21, size=(H // 8 + 1, W // 8 + 1)).astype(np.uint8)
    g = np.kron(g, np.ones((8, 8), np.uint8))[:H, :W].copy()
    g[rng.random((H, W)) < 0.05] = 255                     # ignore label
    return g


def _dicts():
    """Three images of different sizes: float32 dicts of 1-6 keys inserted unsorted, exact ties between channels and with the
    thresholds 0.00 and 0.30, negative values, 255-pixels in the ground truth."""
    rng = np.random.default_rng(9)
    out = []
    for im, nk in enumerate((1, 4, 6)):
        H, W = 37 + 20 * im, 53 + 11 * im
        keys = rng.permutation(20)[:nk].tolist()
        if nk > 1 and keys == sorted(keys):
            keys = keys[::-1]
        maps = (rng.random((nk, H, W)) * 0.8 - 0.1).astype(np.float32)
        maps[:, rng.random((H, W)) < 0.1] = np.float32(0.3)
        maps[:, rng.random((H, W)) < 0.05] = 0.0
        maps[:, rng.random((H, W)) < 0.03] = -0.25                         # every kept channel negative
        gt = _gt(im, H, W)
        gt[rng.random((H, W)) < 0.3] = keys[0] + 1
        gt[rng.random((H, W)) < 0.05] = 255
        out.append(({k: maps[j] for j, k in enumerate(keys)}, gt))
    return out


def _ref_counts(dicts, thresholds):
    from oracle import mcl_oracle as O
    ref = np.zeros((len(thresholds), 21, 3), np.int64)
    for pd, gt in dicts:
        for ti, t in enumerate(thresholds):
            tp, p, tt = O.eval_compare(pd, gt, t)
            ref[ti, :, 0] += tp; ref[ti, :, 1] += p; ref[ti, :, 2] += tt
    return ref


def test_curve_counts_exact():
    from oracle import mcl_oracle as O
    from muscle_amd.evaluation import CamDictEval
    dicts = _dicts()
    assert [len(d) for d, _ in dicts] == [1, 4, 6] and any(list(d) != sorted(d) for d, _ in dicts)
    ev = CamDictEval(DEV, CURVE)
    for pd, gt in dicts:
        ev.add(pd, gt)
    ref = _ref_counts(dicts, CURVE)
    got = ev.counts.cpu().numpy()
    assert np.array_equal(got, ref), np.argwhere(got != ref)[:10]
    mious = ev.mious()
    for ti in range(len(CURVE)):
        m, per = O.eval_miou(ref[ti, :, 0], ref[ti, :, 1], ref[ti, :, 2])
        ll = ev.loglist(ti)
        assert ll['mIoU'] == m == mious[ti] and [ll[c] for c in list(ll)[:21]] == per
    # accumulation across calls and a single-threshold table (the --t path): the row of the curve
    one = CamDictEval(DEV, [0.3])
    for pd, gt in dicts:
        one.add(pd, torch.from_numpy(gt).to(DEV))
    assert np.array_equal(one.counts.cpu().numpy()[0], ref[30])


def test_float16_dict_counts_as_its_float32_upcast():
    """The training_eval format (train_mcl.py:300: np.half maps): `tensor[key+1] = ...` upcasts exactly."""
    from muscle_amd.evaluation import CamDictEval
    dicts = _dicts()
    a, b = CamDictEval(DEV, CURVE), CamDictEval(DEV, CURVE)
    half = [({k: v.astype(np.half) for k, v in pd.items()}, gt) for pd, gt in dicts]
    for ph, gt in half:
        a.add(ph, gt)
        b.add({k: v.astype(np.float32) for k, v in ph.items()}, gt)
    assert np.array_equal(a.counts.cpu().numpy(), b.counts.cpu().numpy())
    assert np.array_equal(a.counts.cpu().numpy(), _ref_counts(half, CURVE))


def test_matches_reference_fixture():
    """CamDictEval and SegEval against what src/evaluation.py::do_python_eval itself returned (tests/golden/eval_curve.npz,
    tools/gen_eval_curve_golden.py): IoUs derived from integers, 1e-12 relative."""
    from muscle_amd.evaluation import CamDictEval, SegEval, categories
    z = np.load(GOLDEN)
    thr = [float(t) for t in z["thresholds"]]
    assert thr == CURVE
    ev, sev = CamDictEval(DEV, thr), SegEval(DEV)
    i = 0
    while f"maps{i}" in z:
        ev.add({int(k): z[f"maps{i}"][j] for j, k in enumerate(z[f"keys{i}"])}, z[f"gt{i}"])
        sev.add(torch.from_numpy(z[f"png{i}"]).to(DEV), torch.from_numpy(z[f"gt{i}"]).to(DEV))
        i += 1
    assert i >= 3
    for ti in range(len(thr)):
        ll = ev.loglist(ti)
        got = np.array([ll[c] for c in categories] + [ll["mIoU"]])
        assert np.allclose(got, z["loglists_npy"][ti], rtol=1e-12, atol=0), ti
    ll = sev.loglist()
    assert np.allclose(np.array([ll[c] for c in categories] + [ll["mIoU"]]), z["loglist_png"], rtol=1e-12, atol=0)


def test_argument_checks():
    from muscle_amd._lib import lib, ptr
    from muscle_amd.evaluation import CamDictEval
    with pytest.raises(ValueError):
        CamDictEval(DEV, [-0.1, 0.2])
    with pytest.raises(ValueError):
        CamDictEval(DEV, [0.3, 0.2])
    with pytest.raises(ValueError):
        CamDictEval(DEV, [i / 100 for i in range(65)])
    ev = CamDictEval(DEV, [0.2])
    gt = np.zeros((4, 5), np.uint8)
    with pytest.raises(ValueError):
        ev.add({}, gt)
    with pytest.raises(ValueError):
        ev.add({20: np.zeros((4, 5), np.float32)}, gt)
    with pytest.raises(ValueError):
        ev.add({3: np.zeros((4, 6), np.float32)}, gt)
    L = lib()
    m = torch.zeros(1, 4, 5, device=DEV)
    k = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = torch.zeros(4, 5, dtype=torch.uint8, device=DEV)
    good = (ptr(m), ptr(k), 1, ptr(g), ptr(ev.thr), 1, 21, 4, 5, ptr(ev.counts))
    for i, v in ((0, None), (1, None), (3, None), (4, None), (9, None), (2, 0), (2, 21), (5, 0), (5, 65), (6, 1), (6, 25), (7, 0)):
        args = list(good)
        args[i] = v
        assert L.mx_camdict_confusion(*args, None) < 0, (i, v)
        assert b"camdict_confusion" in L.mx_last_error()
    torch.cuda.synchronize()
    assert int(ev.counts.sum()) == 0
