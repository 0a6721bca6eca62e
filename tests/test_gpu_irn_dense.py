"""The kernels of the dense IRN walk (muscle_amd/csrc/irn.hip), each called alone through muscle_amd._lib.call and held to
tests/irn_dense_ref.py, the plain restatement tests/test_cpu_irn_dense.py pins on the CPU:

  mx_irn_affinity     the fp32 restatement, every word of the n4 x ld buffer                          identical bits
  mx_irn_transition   colsum vs fp64 column sums of power_f32(input)        (integral beta)           (n4/4 + 4) 2^-24 relative
                      T vs fp32(power_f32(input)) / the kernel's colsum     (integral beta)           1 ulp per element
                      T, colsum vs fp64 ** on the same input                (powf: 2.5, 0.5, 65)      2 e32 + 2e-7 of the column max
                      zero pattern, padding diagonal == 1.0, fp64 column sums of T within (n4/4 + 8) 2^-24 of 1
  propagate_to_edge   exp_times 0 / 1 / 2 vs walk(fp64)                                               2 e32 + 2e-7 of the maximum
  mx_irn_up_max       the word mx_irn_finish leaves (identical bits); vs the fp64 maximum             tau relative
  mx_irn_finish       label: fp64 value >= fp64 maximum - tau, == the fp64 arg-max where the gap > tau; ambiguous share <= 1e-3
                      soft: half(v64 - tau) <= soft <= half(v64 + tau); plane 0 == half(bg_thres); ties, all-zero maps

e32 is always the error of the fp32 restatement against the fp64 restatement on the same input, computed in the test, never
from a kernel; tau = 2 e32 + 2e-7 with e32 = max |finish_values(fp32) - finish_values(fp64)|.  The summation bounds: a column
sum adds n4 non-negative terms in four strided chains of n4/4 and a join of three additions, so its relative error is at most
(n4/4 + 2) u to first order, u = 2^-24; the + 4 covers the higher orders.  A column of T is p_i / colsum with one rounded
division each, so its fp64 sum is within that plus one more u of 1.  Every kernel runs twice and must give the same bits;
every figure is printed before it is asserted.

The inputs of the transition tests keep every non-zero affinity >= 0.3 (edge = 0.7 uniform^3 with exact 0.0 and 1.0 planted),
because a smaller one raised to 64 or 65 underflows in fp32 (0.26^65 < 2^-126) and the zero pattern of T would then differ from
the input's for a reason that is not the kernel's.

mx_bgemm in layout NN (the squarings and the final product) is the exact-fp32 MFMA GEMM in either GEMM arithmetic: only the NT
dispatch consults the mode (gemm.hip, nt_uses_split), so the walk tests are not marked both_arith.

The grid cap of irn_affinity_kernel (65535 x 256 = 16.7M work items of n * nd + n4) needs n > 490000 at radius 5; the dense
path would need a 960 GB matrix there, so that stride is out of reach and is not tested.

Measured on an MI355X (the e32 of the walk rows comes from torch's CPU GEMM and moves with the host):

  affinity     all ten cases: 0 words differ (10872 non-zeros at 13x17, 85620 at 31x45)
  transition   integral beta 1 / 2 / 10 / 64: T bit-equal (0 ulp) everywhere; colsum relative error
                 13x17 (n4 224, either ld)  1.916e-07 1.738e-07 4.232e-07 2.456e-07   bound 3.576e-06
                 31x45 (n4 1396)            2.751e-07 3.361e-07 5.748e-07 4.346e-07   bound 2.104e-05
                 banded 4100, beta 10       1.681e-07, last eight rows 0 ulp          bound 6.133e-05
               powf beta 2.5 / 0.5 / 65: T error (e32, bound)
                 13x17   2.957e-07 (1.852e-07, 5.703e-07)  2.649e-07 (2.191e-07, 6.382e-07)  2.104e-07 (2.706e-07, 7.412e-07)
                 31x45   3.120e-07 (2.537e-07, 7.074e-07)  2.677e-07 (2.112e-07, 6.223e-07)  2.835e-07 (3.235e-07, 8.470e-07)
               colsum on the powf route <= 2.944e-07 (bounds from 5.257e-07); max |column sum of T - 1| <= 5.518e-07 (bounds from 3.815e-06)
  walk         e_HIP (e32) at exp_times 0 / 1 / 2; the bound is 2 e32 + 2e-7
                 31x45 C=1  beta 10   3.056e-07 (3.577e-07)  4.595e-07 (6.604e-07)  8.774e-07 (8.863e-07)
                 31x45 C=1  beta 2.5  2.446e-07 (3.400e-07)  3.217e-07 (6.437e-07)  6.897e-07 (1.175e-06)
                 31x45 C=3  beta 10   3.031e-07 (3.548e-07)  4.595e-07 (8.536e-07)  8.776e-07 (1.233e-06)
                 31x45 C=3  beta 2.5  2.546e-07 (3.400e-07)  3.938e-07 (6.330e-07)  6.588e-07 (1.313e-06)
                 31x45 C=21 beta 10   2.989e-07 (3.435e-07)  5.269e-07 (5.815e-07)  9.192e-07 (1.302e-06)
                 31x45 C=21 beta 2.5  3.326e-07 (3.324e-07)  4.057e-07 (5.144e-07)  6.510e-07 (6.868e-07)
                 3x7   C=3  beta 10   2.626e-07 (2.626e-07)  3.274e-07 (3.274e-07)  4.660e-07 (4.660e-07)
                 3x7   C=3  beta 2.5  1.891e-07 (2.034e-07)  2.104e-07 (2.104e-07)  2.768e-07 (2.859e-07)
                 1x9   C=2  beta 10   1.179e-07 (1.152e-07)  1.831e-07 (1.831e-07)  3.783e-07 (3.199e-07)
                 1x9   C=2  beta 2.5  9.402e-08 (9.206e-08)  1.860e-07 (1.860e-07)  1.424e-07 (1.908e-07)
               with the final product as one fp32 chain over K (before it was blocked, indexing.py) the 31x45 rows read
               3.7e-07..4.0e-07 / 5.3e-07..9.2e-07 / 1.1e-06..1.7e-06, and C=21 beta 2.5 exp_times 2 missed its bound: 1.697e-06
               against 1.574e-06
  finish       case (C,h,w,H,W)        e32        tau        max rel    ambiguous share
                 (20,19,23,74,90)      1.644e-07  5.287e-07  3.086e-08  0
                 (20,19,23,76,92)      1.621e-07  5.242e-07  7.632e-09  0
                 (1,1,1,1,1)           0          2.000e-07  0          0
                 (3,1,9,4,33)          9.187e-08  3.837e-07  9.242e-09  0
                 (3,9,1,33,4)          9.187e-08  3.837e-07  9.242e-09  0
                 (254,3,3,12,12)       1.320e-07  4.639e-07  6.190e-08  0
                 (5,128,128,512,512)   1.353e-07  4.706e-07  0          0
                 (1,257,256,1025,1024) 1.690e-07  5.380e-07  4.824e-08  3.811e-06
               in every case: no label differs from the fp64 arg-max, label shortfall 0, no soft value outside its bracket
               ties: label 3 at 382 pixels, label 8 at none;  bg_thres 1.0: 0 of 196 maps with a foreground label (16 before the fix)
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_dense_ref as D  # noqa: E402
from irn_walk_ref import power_f32  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
U = 2.0 ** -24
CANARY = np.float32(-12345.6789)
NCANARY = 64
AMBIGUOUS_CAP = 1e-3
BG = 0.25


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


def ulps(a, b):
    """Largest distance in units of the last place between two non-negative finite fp32 arrays."""
    return int(np.abs(bits(a).astype(np.int64) - bits(b).astype(np.int64)).max())


def rel(a, ref):
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def n4_of(n):
    return (n + 3) // 4 * 4


@functools.lru_cache(maxsize=None)
def edge_map(h, w, scale=1.0):
    """fp32 [h,w]: scale * uniform^3 with exact 0.0 and exact 1.0 pixels planted, a corner among them."""
    from muscle_amd import synth
    e = (np.float32(scale) * synth.uniform(5, "dense_e", (h, w)).astype(np.float32) ** 3).astype(np.float32)
    e[0, 0] = 1.0
    if h * w > 4:
        e[h // 2, w // 2] = 1.0
        e[h // 3, (2 * w) // 3] = 0.0
    if h * w > 1:
        e[h - 1, w - 1] = 0.0
    e.setflags(write=False)
    return e


@functools.lru_cache(maxsize=None)
def affinity_ref(h, w, radius, scale=1.0):
    a = D.affinity(edge_map(h, w, scale), radius, np.float32)
    a.setflags(write=False)
    return a


# ---- a. mx_irn_affinity -------------------------------------------------------------------------------------------------
def run_affinity(edge, radius, ld):
    """The whole buffer (n4 x ld and the canary behind it) after mx_irn_affinity, run twice on canary-filled memory."""
    from muscle_amd import indexing
    from muscle_amd._lib import call, ptr, stream
    h, w = edge.shape
    n4 = n4_of(h * w)
    e = torch.from_numpy(np.array(edge)).to(DEV)
    pc, off, ln, nd = indexing._path_table(radius, e.device)
    out = []
    for _ in range(2):
        buf = torch.full((n4 * ld + NCANARY,), float(CANARY), dtype=torch.float32, device=DEV)
        call("mx_irn_affinity", ptr(e), h, w, radius, ptr(pc), ptr(off), ptr(ln), nd, ptr(buf), ld, n4, stream())
        torch.cuda.synchronize()
        out.append(buf.cpu().numpy())
    assert np.array_equal(bits(out[0]), bits(out[1])), "mx_irn_affinity: two runs differ"
    return out[0], n4


@pytest.mark.parametrize("h,w,radius,extra_ld", [(13, 17, 5, 0), (31, 45, 5, 0), (3, 7, 5, 0), (1, 9, 5, 0), (9, 1, 5, 0), (1, 1, 5, 0),
                                                 (16, 12, 3, 0), (6, 5, 2, 0), (10, 11, 8, 0), (13, 17, 5, 8)])
def test_affinity_bit_for_bit(h, w, radius, extra_ld):
    """Every entry is one correctly rounded fp32 subtraction of a maximum of fp32 inputs, so the fp32 restatement is exact.
    Rows / columns n..n4-1: zero but for a unit diagonal; columns n4..ld-1: zero (the entry clears n4 * ld words); the 64 words
    behind the buffer keep their canary."""
    n = h * w
    buf, n4 = run_affinity(edge_map(h, w), radius, n4_of(n) + extra_ld)
    ld = n4 + extra_ld
    got, tail = buf[:n4 * ld].reshape(n4, ld), buf[n4 * ld:]
    want = D.padded_affinity(affinity_ref(h, w, radius), n4, ld, fill=0.0)
    wrong = int((bits(got) != bits(want)).sum())
    pad = got[n:n4, :n4].copy(), got[:n4, n:n4].copy()
    print(f"[irn_dense] affinity {h}x{w} r={radius} n4={n4} ld={ld}: {int((want != 0).sum())} non-zeros, {wrong} words differ")
    assert tail.size == NCANARY and (bits(tail) == bits(np.full(NCANARY, CANARY))).all(), "wrote behind the buffer"
    assert wrong == 0
    for v in range(n, n4):                                     # (implied by the comparison above; spelt out)
        assert got[v, v] == 1.0 and np.count_nonzero(got[v]) == 1 and np.count_nonzero(got[:, v]) == 1
    assert all(np.count_nonzero(p) == n4 - n for p in pad) and not got[:, n4:].any()


# ---- b. mx_irn_transition -----------------------------------------------------------------------------------------------
def run_transition(full, n4, ld, beta):
    """full fp32 [n4, ld] (uploaded, so nothing chains) -> (T [n4, ld], colsum [n4]); twice, identical bits, canaries kept."""
    from muscle_amd._lib import call, ptr, stream
    out = []
    for _ in range(2):
        buf = torch.full((n4 * ld + NCANARY,), float(CANARY), dtype=torch.float32, device=DEV)
        buf[:n4 * ld] = torch.from_numpy(full.reshape(-1)).to(DEV)
        cs = torch.full((n4 + NCANARY,), float(CANARY), dtype=torch.float32, device=DEV)
        call("mx_irn_transition", ptr(buf), n4, ld, float(beta), ptr(cs), stream())
        torch.cuda.synchronize()
        out.append((buf.cpu().numpy(), cs.cpu().numpy()))
        del buf, cs
    assert np.array_equal(bits(out[0][0]), bits(out[1][0])) and np.array_equal(bits(out[0][1]), bits(out[1][1])), "two runs differ"
    buf, cs = out[0]
    canary = bits(np.full(NCANARY, CANARY))
    assert (bits(buf[n4 * ld:]) == canary).all() and (bits(cs[n4:]) == canary).all(), "wrote behind a buffer"
    T = buf[:n4 * ld].reshape(n4, ld)
    assert (bits(T[:, n4:]) == bits(CANARY)).all(), "the pad columns n4..ld-1 were touched"
    return np.ascontiguousarray(T[:, :n4]), cs[:n4].copy()


def check_transition(name, inp, beta, T, colsum):
    """inp fp32 [n4,n4] (what was uploaded), T / colsum from the kernel."""
    n4 = inp.shape[0]
    assert np.isfinite(T).all() and np.isfinite(colsum).all()
    if 0 < beta <= 64 and float(beta) == int(beta):
        P = power_f32(inp, beta)
        cs64 = P.astype(np.float64).sum(axis=0)
        e_cs = float((np.abs(colsum.astype(np.float64) - cs64) / cs64).max())
        want = (P / colsum[None, :]).astype(np.float32)
        d = ulps(T, want)
        print(f"[irn_dense] transition {name} beta {beta}: colsum rel {e_cs:.3e} (bound {(n4 / 4 + 4) * U:.3e})  T {d} ulp "
              f"({'bit-equal' if d == 0 else 'not bit-equal'})")
        assert e_cs <= (n4 / 4 + 4) * U
        assert d <= 1
    else:
        s64, cs64, T64 = D.transition(inp.astype(np.float64), beta, np.float64)
        _, cs32, T32 = D.transition(inp, beta, np.float32)
        colmax = T64.max(axis=0)
        err = float((np.abs(T.astype(np.float64) - T64) / colmax).max())
        e32 = float((np.abs(T32.astype(np.float64) - T64) / colmax).max())
        e_cs = float((np.abs(colsum.astype(np.float64) - cs64) / cs64).max())
        e32_cs = float((np.abs(cs32.astype(np.float64) - cs64) / cs64).max())
        print(f"[irn_dense] transition {name} beta {beta} (powf): T {err:.3e} e32 {e32:.3e} bound {2 * e32 + 2e-7:.3e}  "
              f"colsum {e_cs:.3e} e32 {e32_cs:.3e} bound {2 * e32_cs + 2e-7:.3e}")
        assert err <= 2 * e32 + 2e-7
        assert e_cs <= 2 * e32_cs + 2e-7
    assert np.array_equal(T != 0, inp != 0), "zero pattern"
    sums = T.astype(np.float64).sum(axis=0)
    e_sum = float(np.abs(sums - 1).max())
    print(f"[irn_dense] transition {name} beta {beta}: max |column sum of T - 1| {e_sum:.3e} (bound {(n4 / 4 + 8) * U:.3e})")
    assert e_sum <= (n4 / 4 + 8) * U


@pytest.mark.parametrize("beta", [1, 2, 10, 64, 2.5, 0.5, 65])
@pytest.mark.parametrize("h,w,extra_ld", [(13, 17, 0), (13, 17, 8), (31, 45, 0)])
def test_transition_from_uploaded_affinity(h, w, extra_ld, beta):
    n = h * w
    n4 = n4_of(n)
    ld = n4 + extra_ld
    full = D.padded_affinity(affinity_ref(h, w, 5, 0.7), n4, ld, fill=CANARY)
    inp = np.ascontiguousarray(full[:, :n4])
    assert inp[inp != 0].min() >= 0.2999
    T, colsum = run_transition(full, n4, ld, beta)
    check_transition(f"{h}x{w} ld={ld}", inp, beta, T, colsum)
    for v in range(n, n4):                                     # the isolated padding vertices stay isolated: 1 / 1
        assert T[v, v] == 1.0 and colsum[v] == 1.0 and np.count_nonzero(T[v]) == 1 and np.count_nonzero(T[:, v]) == 1
    assert n4 > n


def test_transition_grid_stride():
    """n4 = ld = 4100: 4100^2 = 16,810,000 elements against the 65535 x 256 = 16,776,960 threads of irn_col_scale_kernel's capped
    grid, so the last 33,040 elements (rows 4092.. from column 20 on, to the end) are reached only by the second stride.  A banded
    non-negative matrix (13 diagonals, values in [0.3, 1), unit diagonal), beta 10; the fp64 reference is one power and one
    column sum."""
    from muscle_amd import synth
    n4, half = 4100, 6
    assert n4 * n4 - 65535 * 256 == 33040
    band = (0.3 + 0.7 * synth.uniform(3, "band", (n4, 2 * half + 1))).astype(np.float32)
    inp = np.zeros((n4, n4), np.float32)
    r = np.arange(n4)
    for k in range(-half, half + 1):
        ok = (r + k >= 0) & (r + k < n4)
        inp[r[ok], r[ok] + k] = band[ok, k + half]
    inp[r, r] = 1.0
    T, colsum = run_transition(inp, n4, n4, 10)
    check_transition("banded 4100", inp, 10, T, colsum)
    P = power_f32(inp[-8:], 10)
    once = (P / colsum[None, :]).astype(np.float32)
    twice = (once / colsum[None, :]).astype(np.float32)
    nz = P != 0
    d = ulps(T[-8:], once)
    print(f"[irn_dense] transition banded 4100: last eight rows {d} ulp from scaled-once; colsum in [{colsum.min():.3f}, {colsum.max():.3f}]")
    assert d <= 1 and colsum[-16:].min() > 1.01
    assert (T[-8:][nz] < P[nz]).all() and (T[-8:][nz] > twice[nz]).all()      # neither unscaled nor scaled twice


# ---- c. the walk at few squarings ---------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def walk_case(h, w, C):
    from muscle_amd import synth
    x = synth.uniform(7, "irn_x", (1, C, h, w)).astype(np.float32)
    edge = (synth.uniform(7, "irn_e", (1, h, w)).astype(np.float32) ** 3).astype(np.float32)
    return x, edge


@functools.lru_cache(maxsize=None)
def walk_refs(h, w, C, beta, times):
    x, edge = walk_case(h, w, C)
    r64 = D.walk(x, edge, 5, beta, times, np.float64)
    return r64, rel(D.walk(x, edge, 5, beta, times, np.float32), r64)


@pytest.mark.parametrize("beta", [10, 2.5])
@pytest.mark.parametrize("h,w,C", [(31, 45, 1), (31, 45, 3), (31, 45, 21), (3, 7, 3), (1, 9, 2)])
def test_walk_at_few_squarings(h, w, C, beta):
    """exp_times 0 (no squaring: the transition matrix itself times the masked maps), 1 and 2: nothing has mixed yet, so a
    misplaced tap or a wrong padded row shows at full size.  C is no multiple of 4 (padded class rows); x as [1,C,h,w] and
    as [C,h,w].

    Which way it went: with the final product (class maps x T^(2^exp_times)) as one fp32 accumulation chain over all n4 vertices,
    31 x 45, C = 21, beta 2.5, exp_times 2 read 1.697e-06 against a bound of 1.574e-06; an fp32 numpy product that adds the K
    terms one after another reproduces that figure, and with the squarings alone in fp32 the error is 4.6e-07.  propagate_to_edge
    now cuts that product's K into blocks of 128 and adds the partial products; the case reads 6.510e-07."""
    from muscle_amd import indexing
    x, edge = walk_case(h, w, C)
    xg, eg = torch.from_numpy(x).to(DEV), torch.from_numpy(edge).to(DEV)
    for times in (0, 1, 2):
        r64, e32 = walk_refs(h, w, C, beta, times)
        rw = indexing.propagate_to_edge(xg, eg, radius=5, beta=beta, exp_times=times, method="dense")
        rw3 = indexing.propagate_to_edge(xg[0].contiguous(), eg, radius=5, beta=beta, exp_times=times, method="dense")
        again = indexing.propagate_to_edge(xg, eg, radius=5, beta=beta, exp_times=times, method="dense")
        assert tuple(rw.shape) == (C, 1, h, w) == r64.shape and rw.dtype == torch.float32
        assert torch.equal(rw, again) and torch.equal(rw, rw3)
        e = rel(rw.cpu().numpy(), r64)
        print(f"[irn_dense] walk {h}x{w} C={C} beta {beta} exp_times {times}: e_HIP {e:.3e}  e32 {e32:.3e}  bound {2 * e32 + 2e-7:.3e}")
        assert e <= 2 * e32 + 2e-7, (times, e, e32)


# ---- d. mx_irn_up_max and mx_irn_finish ---------------------------------------------------------------------------------
def run_finish(rw, H, W, bg):
    """rw fp32 numpy [C,1,h,w] -> (label [H,W], soft [H,W,C+1], word): finish_semseg(soft_output=True) twice (identical bits), the
    word mx_irn_finish leaves in its scratch (a direct call, whose label must equal finish_semseg's) and the word of
    mx_irn_up_max alone, twice: one value."""
    from muscle_amd import indexing
    from muscle_amd._lib import call, ptr, stream
    C, _, h, w = rw.shape
    g = torch.from_numpy(rw).to(DEV)
    lab, soft = indexing.finish_semseg(g, H, W, bg, soft_output=True)
    lab2, soft2 = indexing.finish_semseg(g, H, W, bg, soft_output=True)
    assert torch.equal(lab, lab2) and torch.equal(soft.view(torch.int16), soft2.view(torch.int16))
    r = g.reshape(C, h, w).contiguous()
    words = []
    for _ in range(2):
        s = torch.full((1 + NCANARY,), 0x7FC12345, dtype=torch.int32, device=DEV)
        call("mx_irn_up_max", ptr(r), C, h, w, H, W, ptr(s), stream())
        words.append(s.cpu().numpy())
    s = torch.full((1 + NCANARY,), 0x7FC12345, dtype=torch.int32, device=DEV)
    lab3 = torch.full((H * W + NCANARY,), 0xA5, dtype=torch.uint8, device=DEV)
    call("mx_irn_finish", ptr(r), C, h, w, H, W, float(bg), ptr(s), ptr(lab3), None, stream())
    words.append(s.cpu().numpy())
    lab3 = lab3.cpu().numpy()
    assert all((wd[1:] == 0x7FC12345).all() for wd in words) and (lab3[H * W:] == 0xA5).all(), "wrote behind a buffer"
    assert words[0][0] == words[1][0] == words[2][0], "mx_irn_up_max alone and inside mx_irn_finish leave different words"
    lab, soft = lab.cpu().numpy(), soft.cpu().numpy()
    assert lab.dtype == np.uint8 and lab.shape == (H, W) and soft.dtype == np.float16 and soft.shape == (H, W, C + 1)
    assert np.array_equal(lab3[:H * W].reshape(H, W), lab)
    return lab, soft, words[0][:1].view(np.float32)[0]


@pytest.mark.parametrize("C,h,w,H,W", D.FINISH_CASES, ids=str)
def test_finish_against_fp64(C, h, w, H, W):
    """Cropped and uncropped, one pixel, one row, one column, the largest class count (label 254 occurs), and the two sizes at
    which irn_up_max_kernel (C*H*W > 1,048,576) and irn_label_kernel (H*W > 1,048,576) take a second stride."""
    from muscle_amd import synth
    rw = D.finish_input(synth.uniform, C, h, w)
    lab, soft, vmax = run_finish(rw, H, W, BG)
    up64 = D.upsample4(rw, H, W, np.float64)
    v64 = up64 / up64.max()
    e32 = float(np.abs(D.finish_values(rw, H, W, np.float32).astype(np.float64) - v64).max())
    tau = 2 * e32 + 2e-7
    # the maximum
    e_max = abs(float(vmax) - up64.max()) / up64.max()
    # the labels
    stack, arg, best, gap = D.top_two(v64, BG)
    mine = np.take_along_axis(stack, lab[None].astype(np.int64), axis=0)[0]
    short = float((best - mine).max())
    clear = gap > tau
    share = float(1 - clear.mean())
    wrong = int((lab[clear] != arg[clear]).sum())
    # the soft values
    lo = (v64 - tau).astype(np.float16).astype(np.float32)
    hi = (v64 + tau).astype(np.float16).astype(np.float32)
    s = soft.astype(np.float32)
    val = np.moveaxis(s[..., 1:], -1, 0)
    outside = int(((val < lo) | (val > hi)).sum())
    print(f"[irn_dense] finish {(C, h, w, H, W)}: e32 {e32:.3e} tau {tau:.3e}  max rel {e_max:.3e}  worst label shortfall {short:.3e}  "
          f"ambiguous share {share:.3e}  labels differing {int((lab != arg).sum())} (outside the ambiguous: {wrong})  "
          f"soft outside its bracket {outside}  soft max diff {float(np.abs(val - v64).max()):.3e}")
    assert e_max <= tau
    assert short <= tau
    assert wrong == 0
    assert share <= AMBIGUOUS_CAP
    assert outside == 0
    assert (soft[..., 0] == np.float16(BG)).all()
    if C > 2:
        assert not (lab == (4 if C > 3 else 2)).any()          # the absent class
    if C == 254:
        assert (lab == 254).any()


def test_finish_exact_ties_first_maximum_wins():
    """Channel 2 copied into channel 7: wherever that value is the largest the label is 3 (channel 2, the first maximum) and the
    label of channel 7, 8, never occurs.  A threshold above every value (1.5): label 0 everywhere."""
    from muscle_amd import synth
    C, h, w, H, W = D.FINISH_CASES[0]
    rw = D.finish_input(synth.uniform, C, h, w)
    rw[7] = rw[2]
    lab, soft, _ = run_finish(rw, H, W, BG)
    print(f"[irn_dense] ties: label 3 at {int((lab == 3).sum())} pixels, label 8 at {int((lab == 8).sum())}")
    assert (lab == 3).any() and not (lab == 8).any()
    assert np.array_equal(soft[..., 3].view(np.uint16), soft[..., 8].view(np.uint16))
    lab, soft, _ = run_finish(rw, H, W, 1.5)
    assert not lab.any() and (soft[..., 0] == np.float16(1.5)).all()


def test_finish_quotient_at_the_maximum_is_one():
    """bg_thres = 1.0.  In the reference rw_up / max(rw_up) is exactly 1.0 at the arg-max pixel and below 1 elsewhere, so no value
    beats the threshold and every label is 0.  If the maximum kernel and the label kernel round the blend differently at the
    arg-max pixel, the quotient is 1 + 1 ulp there and a foreground label appears.  Maps whose maximum is an interior pixel (no upsampled pixel copies an interior
    source pixel, so the maximum is always a blend): 192 small ones with different data, and four of 32 x 128 x 128 -> 512 x 512
    (8.4M values, 8 per thread, so the unrolled loop of the maximum kernel runs as well as its remainder) whose 4 x 4 block
    repeats, so the maximum is reached at about a thousand pixels in every channel.

    Which way it went: with the maximum formed by the plain, compiler-contracted blend (irn_up4_max, as irn_up_max_kernel had it)
    16 of these 196 maps came back with a foreground label, 976 pixels in all.  irn_up_max_kernel now forms the maximum with
    irn_up4 (irn_soft.h), the arithmetic of the values that are divided by it, and no map does."""
    from muscle_amd import synth
    cases = []
    for i in range(192):
        C, h, w = 1 + i % 3, 5 + i % 4, 6 + (i // 4) % 5
        m = (synth.uniform(100 + i, "peak", (C, 1, h, w)).astype(np.float32) ** 2).astype(np.float32)
        m[:, :, 0, :] *= 0.5
        m[:, :, -1, :] *= 0.5
        m[:, :, :, 0] *= 0.5
        m[:, :, :, -1] *= 0.5
        m[i % C, 0, 1 + i % (h - 2), 1 + (i // 3) % (w - 2)] = 1.0 + (i % 7) / 8
        cases.append((m, 4 * h - i % 3, 4 * w - i % 2))
    for i in range(4):
        block = (synth.uniform(300 + i, "peak", (32, 1, 4, 4)).astype(np.float32) ** 2).astype(np.float32)
        m = np.tile(block, (1, 1, 32, 32))
        m[:, :, 0, :] *= 0.5
        m[:, :, -1, :] *= 0.5
        m[:, :, :, 0] *= 0.5
        m[:, :, :, -1] *= 0.5
        cases.append((np.ascontiguousarray(m), 512, 512))
    hot, pixels = 0, 0
    for m, H, W in cases:
        lab, _, vmax = run_finish(m, H, W, 1.0)
        hot += int(lab.any())
        pixels += int(np.count_nonzero(lab))
        assert vmax > 0
    print(f"[irn_dense] bg_thres 1.0 on {len(cases)} maps: {hot} maps with a foreground label, {pixels} such pixels")
    assert hot == 0


def test_finish_all_zero_maps():
    """Documented in finish_semseg: an all-zero rw leaves the word 0 (values NaN) and every label 0.  Not compared with the
    reference, whose arg-max over NaN differs."""
    rw = np.zeros((3, 1, 5, 7), np.float32)
    lab, soft, vmax = run_finish(rw, 20, 27, BG)
    assert vmax.view(np.uint32) == 0 and not lab.any()
    assert (soft[..., 0] == np.float16(BG)).all()
