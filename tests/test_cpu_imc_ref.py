"""CPU checks behind tests/test_gpu_imc.py: the float64 reference of tests/imc_ref.py against a literal restatement of the
reference's double loop, the reference's own recorded outputs (tests/golden/units.npz) and the oracle's closed form, and the
structure of the label design (valid anchor rows per block of 16) that the GPU cases rely on."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import golden_util as gu
import imc_ref as R
from muscle_amd import synth
from oracle import mcl_oracle as O

T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


def loop_imc(emb, label):
    """loss_multilabel.py:36-66 as it stands, pair by pair: the sums become tensors with their first term, a row counts
    when both are tensors and it saw more negatives than positives, and the result is 0 / n = 0 (a Python number) when no
    row counted."""
    total = 0
    e = F.normalize(emb, eps=1e-6, dim=-1)
    n = e.shape[0]
    for i in range(n):
        pos, neg, n_pos, n_neg = 1e-6, 1e-6, 0, 0
        for j in range(i + 1, n):
            if all(torch.eq(label[i], label[j])):
                pos = pos + torch.exp((e[i] * e[j]).sum() / 0.1)
                n_pos += 1
            if torch.bitwise_and(label[i].long(), label[j].long()).sum() == 0:
                neg = neg + torch.exp((e[i] * e[j]).sum() / 0.1)
                n_neg += 1
        if torch.is_tensor(pos) and torch.is_tensor(neg) and n_neg > n_pos:
            total = total - torch.log(pos / (pos + neg))
    return total / n


def _loop_cases():
    for d in (16, 36):
        for name in R.HAND:
            yield f"{name}-{d}", R.hand_case(name, d)[:2]
    for n, d, L in [(17, 16, 20), (33, 64, 20), (7, 36, 9)]:
        yield f"groups-{n}x{d}", (R.imc_emb(n, d, seed=n), R.imc_labels(n, L))
    x, _ = R.low_norm(R.imc_emb(33, 64, seed=33))
    yield "lownorm-33x64", (x, R.imc_labels(33, 20))


LOOP_CASES = dict(_loop_cases())


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_imc_ref_equals_the_double_loop(name):
    emb, lab = LOOP_CASES[name]
    r = R.imc_ref(emb, lab)
    x = T(emb).double().requires_grad_()
    want = loop_imc(x, T(lab))
    assert torch.is_tensor(want) == (r.n_valid > 0)
    if r.n_valid == 0:
        assert want == 0 and r.loss == 0.0 and not r.grad.any()
        return
    want.backward()
    want = float(want.detach())
    assert abs(r.loss - want) <= 1e-12 * abs(want)
    assert np.isfinite(r.grad).all() and gu.rel_err(r.grad, x.grad.numpy()) <= 1e-12


def test_hand_cases_have_the_stated_structure():
    for name, (lab, n_valid) in R.HAND.items():
        r = R.imc_ref(R.hand_case(name, 16)[0], lab)
        assert r.n_valid == n_valid, name
    r = R.imc_ref(*R.hand_case("AAB", 16)[:2])
    assert (r.vp[0], r.vn[0]) == (1, 1)
    r = R.imc_ref(*R.hand_case("AABC", 16)[:2])
    assert (r.vp[0], r.vn[0]) == (1, 2) and list(r.valid) == [True, False, False, False]
    r = R.imc_ref(*R.hand_case("AAA'", 16)[:2])
    assert (r.vp[0], r.vn[0]) == (1, 0)
    r = R.imc_ref(*R.hand_case("two", 16)[:2])
    assert (r.vp[0], r.vn[0]) == (1, 2) and r.valid[0]


def test_imc_ref_reproduces_the_reference_outputs():
    U = gu.load("units.npz")
    emb = synth.normal(3, "imc.emb", (8, 48)).astype(np.float32)
    r = R.imc_ref(emb, synth.synth_labels(8, 4))
    assert bool(U["imc_is_tensor"]) and r.n_valid > 0
    assert abs(r.loss - float(U["imc"])) <= 1e-6 * abs(float(U["imc"]))
    assert gu.rel_err(r.grad, U["imc_demb"]) <= 1e-6
    r0 = R.imc_ref(synth.normal(3, "imc.emb0", (4, 48)).astype(np.float32), np.ones((4, 20), np.float32))
    assert r0.n_valid == 0 and r0.loss == 0.0 == float(U["imc_degenerate"][0]) and not r0.grad.any()


@pytest.mark.parametrize("name", list(LOOP_CASES))
def test_imc_ref_agrees_with_the_oracle_in_float64(name):
    emb, lab = LOOP_CASES[name]
    r = R.imc_ref(emb, lab)
    x = T(emb).double().requires_grad_()
    want = O.image_level_contrast(x, T(lab))
    if r.n_valid == 0:
        assert not torch.is_tensor(want) and want == 0.0
        return
    want.backward()
    want = float(want.detach())
    assert abs(r.loss - want) <= 1e-12 * abs(want)
    assert gu.rel_err(r.grad, x.grad.numpy()) <= 1e-12


@pytest.mark.parametrize("n", list(R.BLOCK_TABLE))
def test_label_design_puts_valid_anchors_in_every_block(n):
    for L, groups in [(20, R.GROUPS), (32, R.spread_groups(32)), (70, R.spread_groups(70))]:
        P, G = R.pair_masks(R.imc_labels(n, L, groups))
        vp, vn = P.sum(1), G.sum(1)
        assert R.valid_per_block((vp >= 1) & (vn >= 1) & (vn > vp)) == R.BLOCK_TABLE[n], (n, L)
    if n == 64:                      # up to 20 positives in one row, spread over all four column tiles
        assert vp.max() == 20
        assert all(P[int(vp.argmax()), 16 * t:16 * t + 16].any() for t in range(4))


@pytest.mark.parametrize("L,first", [(32, 31), (33, 32), (70, 69), (70, 64)])
def test_last_label_column_decides_pairs(L, first):
    """The wide-label cases of tests/test_gpu_imc.py: without column L - 1 (for L = 70: without the columns past the first 64)
    some pairs are identical that were not, some disjoint that were not, and another number of rows is valid."""
    lab = R.last_column_labels(33, L)
    assert lab[:, first:].any() and lab[list(R.LAST_ROWS), L - 1].all()
    (P, G), (P0, G0) = R.pair_masks(lab), R.pair_masks(R.without_columns(lab, first))
    assert P0[1, 4] and not P[1, 4] and P0[13, 19] and not P[13, 19]             # identical but for the last column
    assert G0[4, 5] and not G[4, 5] and G0[19, 23] and not G[19, 23]             # disjoint but for the last column
    emb = R.imc_emb(33, 64, seed=97)
    a, b = R.imc_ref(emb, lab), R.imc_ref(emb, R.without_columns(lab, first))
    assert (a.n_valid, b.n_valid) == (27, 28) and abs(a.loss - b.loss) > 2e-3 * a.loss
    assert R.valid_per_block(a.valid) == [16, 11, 0]
