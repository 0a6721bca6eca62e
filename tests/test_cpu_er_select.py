"""The ER references of tests/er_ref.py against torch itself, without a GPU: the exact select oracle against fp64
torch.topk, and the value / gradient references against oracle.mcl_oracle.er_loss."""
import numpy as np
import pytest
import torch

import er_ref as R
from muscle_amd import synth
from oracle import mcl_oracle as O

T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


def _rows():
    n = 5000
    rnd = np.abs(synth.normal(1, "sel.rnd", (n,))).astype(np.float32) * 0.25
    dup = rnd.copy(); dup[n // 2:] = dup[:n // 2]                       # every value occurs at least twice
    const = rnd.copy(); const[100:500] = const[7]                       # 401 identical values
    sparse = rnd.copy(); sparse[np.abs(synth.normal(2, "sel.mask", (n,))) < 1.6] = 0.0     # ~89 % exact zeros
    return {"random": rnd, "dup": dup, "const": const, "sparse": sparse, "zeros": np.zeros(64, np.float32)}


ROWS = _rows()


@pytest.mark.parametrize("name", list(ROWS))
def test_select_oracle_matches_fp64_topk(name):
    row = ROWS[name]
    nnz = int((row != 0).sum())
    srt = np.sort(row)[::-1]
    ks = {1, 2, 7, row.size // 5, nnz, nnz + 1, row.size, int(np.searchsorted(-srt, -srt[min(250, row.size - 1)])) + 5}
    for k in sorted(k for k in ks if 1 <= k <= row.size):
        o = R.select_oracle(row, k)
        want = float(torch.topk(T(row).double(), k).values.sum())
        got = R.row_topk_sum(o)
        assert abs(got - want) <= 1e-12 * abs(want), (name, k, got, want)
        # the fields against a plain sort
        assert R.tau_of(o) == float(srt[k - 1]) and o["tau_bits"] == int(srt[k - 1:k].view(np.uint32)[0])
        assert o["krem"] == k - int((row > srt[k - 1]).sum()) and o["cnt_eq"] == int((row == srt[k - 1]).sum())
        if k <= nnz:
            assert 1 <= o["krem"] <= o["cnt_eq"]
        else:
            assert o["tau_bits"] == 0 and o["krem"] == k - nnz
    if name == "const":
        o = R.select_oracle(row, int((row > row[7]).sum()) + 100)
        assert o["cnt_eq"] >= 401 and o["krem"] == 100
    if name == "dup":
        assert R.select_oracle(row, 3)["cnt_eq"] == 2 and R.select_oracle(row, 3)["krem"] == 1


def test_select_weights_sum_to_k():
    rows = np.stack([ROWS["dup"], ROWS["const"], ROWS["sparse"]])
    for k in (3, 333, 1000):
        loss, os_ = R.select_loss(rows, k)
        w = R.select_weights(rows, os_)
        for n in range(3):
            assert abs(w[n].sum() - min(k, int((rows[n] != 0).sum()))) < 1e-9
        want = torch.topk(T(rows).double(), k, dim=1).values.mean()
        assert abs(float(loss) - float(want)) <= 6e-8 * float(want)        # one fp32 rounding


def _small(K=21, L=24):
    n, h, w = 3, 4, 5
    cam = synth.normal(4, "er.cam", (n, h, w, L)).astype(np.float32)
    sgc = synth.normal(4, "er.sgc", (n, h, w, L)).astype(np.float32)
    lab = synth.synth_labels(n, 6)
    lwb = np.concatenate([np.ones((n, 1), np.float32), lab], 1)
    return cam, sgc, lab, lwb


def test_value_and_grad_refs_match_oracle_er_loss():
    cam, sgc, lab, lwb = _small()
    K, H, W = 21, 9, 11
    vc = int(lab.sum())
    k = int(0.2 * vc * H * W)
    cf, sf = R.upsample_lr(cam, K, H, W), R.upsample_lr(sgc, K, H, W).requires_grad_()
    want = O.er_loss(O.cam_softmaxnorm(cf), O.cam_softmaxnorm(sf), T(lwb).double(), vc)
    want.backward()
    want = want.detach()
    v_full = R.er_values_ref(cf, sf.detach(), lwb)
    v_lr = R.er_values_lr_ref(cam, sgc, lwb, K, H, W)
    assert torch.equal(v_full, v_lr)
    got = torch.topk(v_lr.flatten(1), k, dim=1).values.mean()
    assert abs(float(got) - float(want)) <= 1e-14
    # fixed weights from the select of the fp32-rounded values reproduce autograd of the reference expression (no ties here)
    rows = v_lr.flatten(1).float().numpy()
    loss, os_ = R.select_loss(rows, k)
    assert abs(float(loss) - float(want)) <= 2e-7 * float(want)
    wts = R.select_weights(rows, os_)
    g_full = R.er_grad_ref(cf, sf.detach(), lwb, wts, k)
    assert float((g_full - sf.grad).abs().max()) <= 1e-15
    # ... and the low-resolution gradient is that gradient pulled back through the upsample; padding channels get none
    s_lr = T(sgc).double().requires_grad_()
    R.upsample_lr(s_lr, K, H, W).backward(sf.grad)
    g_lr = R.er_grad_ref(cam, sgc, lwb, wts, k, lr=(K, H, W))
    assert float((g_lr - s_lr.grad).abs().max()) <= 1e-15 and float(g_lr[..., K:].abs().max()) == 0.0
    assert float(g_lr[..., 0].abs().max()) == 0.0
    assert R.min_small_diff(cam, sgc, lwb, lr=(K, H, W)) > 1e-6


def test_tie_k_finds_a_pair():
    k = R.tie_k(ROWS["dup"], 50, odd=True)
    o = R.select_oracle(ROWS["dup"], k)
    assert k % 2 == 1 and k >= 50 and o["cnt_eq"] == 2 and o["krem"] == 1
