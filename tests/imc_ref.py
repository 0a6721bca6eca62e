"""Float64 reference of the image-level contrast (IMC) loss, loss_multilabel.py:36-66, and the inputs of its tests
(tests/test_cpu_imc_ref.py, tests/test_gpu_imc.py).  CPU only; nothing here touches the project's kernels or its oracle.

  e      = x / max(||x||, 1e-6)
  s_ij   = exp(e_i . e_j / 0.1)
  P_ij   = label_i == label_j everywhere,           j > i
  G_ij   = sum_c (long(label_i) & long(label_j)) == 0,   j > i
  sp_i   = 1e-6 + sum_j P_ij s_ij,   sn_i = 1e-6 + sum_j G_ij s_ij
  valid  = vp >= 1 and vn >= 1 and vn > vp      (vp, vn: the row counts of P, G)
  loss   = sum_valid -log(sp / (sp + sn)) / N

and the gradient is float64 autograd of exactly that (the clamp passes no gradient to a norm below 1e-6: such a row gets g / 1e-6).
"""
import collections

import numpy as np
import torch

from muscle_amd import synth

GROUPS = [(0,), (1, 2), (0, 3), (4,), (1, 2), (5, 6, 7)]
# valid anchor rows per block of 16 rows with imc_labels(n, L, GROUPS)
BLOCK_TABLE = {15: [10], 16: [11], 17: [12, 0], 33: [16, 12, 0], 48: [16, 16, 11], 49: [16, 16, 12, 0], 63: [16, 16, 16, 10],
               64: [16, 16, 16, 11]}

ImcRef = collections.namedtuple("ImcRef", "loss n_valid grad vp vn valid")


def pair_masks(label):
    """(P, G) as bool [n, n], upper triangle only."""
    lab = np.asarray(label)
    n = lab.shape[0]
    li = lab.astype(np.int64)
    upper = np.triu(np.ones((n, n), bool), 1)
    same = (lab[:, None, :] == lab[None, :, :]).all(-1)
    disj = (li[:, None, :] & li[None, :, :]).sum(-1) == 0
    return same & upper, disj & upper


def imc_ref(emb, label):
    """ImcRef(loss, n_valid, grad [n, d] float64, vp [n], vn [n], valid [n]) from the fp32 (or any) input values."""
    x = torch.from_numpy(np.array(emb, dtype=np.float64)).requires_grad_()
    n = x.shape[0]
    P, G = pair_masks(label)
    vp, vn = P.sum(1), G.sum(1)
    valid = (vp >= 1) & (vn >= 1) & (vn > vp)
    e = x / torch.linalg.vector_norm(x, dim=1, keepdim=True).clamp_min(1e-6)
    s = torch.exp(e @ e.t() / 0.1)
    sp = 1e-6 + (s * torch.from_numpy(P)).sum(1)
    sn = 1e-6 + (s * torch.from_numpy(G)).sum(1)
    per = -torch.log(sp / (sp + sn))
    loss = (per * torch.from_numpy(valid)).sum() / n
    loss.backward()
    return ImcRef(float(loss.detach()), int(valid.sum()), x.grad.numpy(), vp, vn, valid)


def valid_per_block(valid):
    v = np.asarray(valid)
    return [int(v[b:b + 16].sum()) for b in range(0, len(v), 16)]


def row_err(got, ref):
    """max_i ( max_d |got - ref|_i / (max_d |ref_i| + 0.01 max |ref|) ): a row's own scale, floored at 1 % of the largest."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    rows = np.abs(ref).max(1)
    return float((np.abs(got - ref).max(1) / (rows + 0.01 * rows.max())).max())


# ---- inputs --------------------------------------------------------------------------------------------------------------
def imc_labels(n, L, groups=GROUPS):
    """[n, L] float32 multi-hot: row i carries the class set groups[i % len(groups)]."""
    lab = np.zeros((n, L), np.float32)
    for i in range(n):
        lab[i, list(groups[i % len(groups)])] = 1.0
    return lab


def spread_groups(L):
    """GROUPS with class c moved to column c (L - 1) // 7: the same pair structure on columns spread up to L - 1.  (The last
    column alone decides nothing here: class 7 occurs only together with 5 and 6.  last_column_labels() adds pairs it decides.)"""
    return [tuple(c * (L - 1) // 7 for c in g) for g in GROUPS]


LAST_ROWS = (4, 19)


def last_column_labels(n, L):
    """imc_labels(n, L, spread_groups(L)) with column L - 1 also set in rows 4 and 19, both of the set (1, 2).  Only that column
    tells them from the other (1, 2) rows (P: rows 1-4, 4-7, 13-19, 19-25, ... are no longer identical) and only there do they
    meet the (5, 6, 7) rows (G: rows 4-5, 4-11, 19-23, ... are no longer disjoint): a kernel that skips the last label column
    gets other masks and another count of valid rows (without_columns(), asserted in tests/test_cpu_imc_ref.py)."""
    lab = imc_labels(n, L, spread_groups(L))
    lab[[r for r in LAST_ROWS if r < n], L - 1] = 1.0
    return lab


def without_columns(label, first):
    lab = np.array(label)
    lab[:, first:] = 0.0
    return lab


def imc_emb(n, d, seed=0):
    """[n, d] float32, 1.5 base[i % 6] + noise with every seventh row (2, 9, ...) negated: rows of one base are strongly
    correlated, so s = exp(cos / 0.1) spans many orders of magnitude inside every 16 x 16 tile."""
    base = synth.normal(seed, f"imc.base.{d}", (6, d))
    x = 1.5 * base[np.arange(n) % 6] + synth.normal(seed, f"imc.noise.{n}.{d}", (n, d))
    x[2::7] *= -1.0
    return x.astype(np.float32)


def low_norm(emb):
    """Rows 1 and 20 zero, row 4 of norm 1e-8; every other norm >= 1e-3 (asserted), nothing near the 1e-6 switch."""
    x = np.array(emb, np.float32)
    tiny = [r for r in (1, 20) if r < len(x)]
    x[tiny] = 0.0
    x[4] *= np.float32(1e-8 / np.linalg.norm(x[4].astype(np.float64)))
    nrm = np.linalg.norm(x.astype(np.float64), axis=1)
    assert 0.5e-8 < nrm[4] < 2e-8 and (np.delete(nrm, tiny + [4]) >= 1e-3).all()
    return x, tiny + [4]


def _sets(L, *sets):
    lab = np.zeros((len(sets), L), np.float32)
    for i, s in enumerate(sets):
        for c, v in (s.items() if isinstance(s, dict) else [(c, 1.0) for c in s]):
            lab[i, c] = v
    return lab


# name: (labels [n, 20], valid anchor rows); A = {3}, B = {5}, C = {9, 11}, A' = {3, 4}
HAND = {
    "AAB": (_sets(20, (3,), (3,), (5,)), 0),                     # row 0: vp = 1, vn = 1 - not vn > vp
    "AABC": (_sets(20, (3,), (3,), (5,), (9, 11)), 1),           # row 0: vp = 1, vn = 2
    "AAA'": (_sets(20, (3,), (3,), (3, 4)), 0),                  # row 0: vp = 1, vn = 0
    "N1": (_sets(20, (3,)), 0),
    "alleq": (_sets(20, (3, 7), (3, 7), (3, 7), (3, 7)), 0),
    # a label value 2.0 meets 1.0 in the same column: 2 & 1 == 0, the pair counts as disjoint; row 0: vp = 1, vn = 2
    "two": (_sets(20, {3: 2.0}, {3: 2.0}, {3: 1.0}, {3: 1.0, 6: 1.0}), 1),
}


def hand_case(name, d):
    lab, n_valid = HAND[name]
    return imc_emb(len(lab), d, seed=40 + d), lab, n_valid
