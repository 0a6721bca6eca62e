"""The support kernels at the top of muscle_amd/csrc/head.hip, and mx_resize_nhwc_bwd of dec.hip beside the resize it transposes,
each ALONE against the float64 restatements of tests/dec_ref.py, at the smallest shapes that reach each branch (the tables in
dec_ref.py; tests/test_cpu_dec_ref.py checks their input conditions on the reference alone).  Every case runs twice and must give
the same bits; every output buffer carries canaries where the kernel must not write.

Tolerances, by the rule of tests/test_gpu_bn_kernels.py, in units of U = 2^-24 times the magnitude dec_ref returns:
  elementwise      k*U*magnitude, k = the arithmetic operations on the path (stated at each test);
  bilinear values  BLEND_OPS*U*(blend of |src|) + the slope term of dec_ref.bil_slope_units (the fp32 source coordinate is off by at
                   most 2U(in-1) pixels; the value is piecewise linear), from the actual source array;
  bilinear adjoints and wave sums
                   (4*e_ref + 2U) * sum|term|, e_ref = the error of the fp32 restatement on the same inputs; asserted with it: the
                   allowance stays below a tenth of the share of one destination row or column (adjoints: what a gather range one
                   index too tight would drop) or of one element (row sums);
  exact regimes    torch.equal: the identity resize, integer inputs of sym_relu_grad, untouched or zeroed regions.
No tolerance is taken from a kernel's output.  DEC_KERNELS_PROFILE=<file> records every case's figures (profiles/dec_kernels_error.txt; the pair of files shares it).
"""
import pytest
import torch

import dec_ref as R
from dec_ref import U
from dec_gpu_util import CANARY, DEV, Profile, check_elementwise, check_sums, twice

pytestmark = pytest.mark.gpu

PROF = Profile("tests/test_gpu_head_kernels.py")


@pytest.fixture(scope="module", autouse=True)
def _profile_file():
    yield
    PROF.write()


def _id(c):
    return "-".join(map(str, c))


# ---- resize_nhwc and its adjoint ----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("pad", [False, True], ids=["dense", "slice"])
@pytest.mark.parametrize("relu", [0, 1])
@pytest.mark.parametrize("case", R.RESIZE_CASES, ids=_id)
def test_resize_nhwc(case, relu, pad):
    """dst[..., coff:coff+C] = [relu] bilinear(src); (ldd, coff) = (C, 0) or (C+8, 4): the other channels keep their canaries."""
    from muscle_amd import ops
    N, C, Hs, Ws, Hd, Wd = case
    ldd, coff = (C + 8, 4) if pad else (C, 0)
    src = R.resize_inputs(case)[0]
    d_src = src.to(DEV)

    def run():
        dst = torch.full((N, Hd, Wd, ldd), CANARY, device=DEV)
        ops.resize_nhwc(d_src, dst, coff, relu=bool(relu))
        return dst
    dst = twice(run)
    got = dst[..., coff:coff + C]
    rest = torch.cat([dst[..., :coff], dst[..., coff + C:]], -1)
    assert bool((rest == CANARY).all()), "channels outside [coff, coff+C) were written"
    ref, mag = R.resize_nhwc(src, Hd, Wd, bool(relu))
    if (Hs, Ws) == (Hd, Wd):
        assert torch.equal(got, src.clamp_min(0) if relu else src)          # scale exactly 1: every weight 0 or 1
    check_elementwise(PROF, f"resize_nhwc {case} relu={relu} ldd={ldd}", got, ref, mag, float(R.BLEND_OPS),
                      extra_abs=R.bil_slope_units(src, Hd, Wd))


@pytest.mark.parametrize("case", [c for c in R.RESIZE_CASES if c != R.RESIZE_FWD_ONLY], ids=_id)
def test_resize_nhwc_bwd(case):
    """gsrc += W^T gdst on a non-zero base against the explicit transpose, and <resize(x), g> = <x, resize_bwd(g)> in float64 from
    the two kernels' own outputs."""
    from muscle_amd import ops
    from muscle_amd._lib import call, ptr, stream
    N, C, Hs, Ws, Hd, Wd = case
    src, g, base = R.resize_inputs(case)
    d_g = g.to(DEV)

    def run():
        gsrc = base.to(DEV)
        call("mx_resize_nhwc_bwd", ptr(d_g), ptr(gsrc), N, Hs, Ws, C, Hd, Wd, stream())
        return gsrc
    got = twice(run).double() - base.double()
    ref, mag, e_ref, rel, share = R.adjoint_rule(g, Hs, Ws)
    assert rel < 0.1 * share, f"a dropped destination row could hide ({rel:.3g} >= {0.1 * share:.3g})"
    check_sums(PROF, f"resize_nhwc_bwd {case}", got, ref, mag, e_ref, rel, extra=2 * U * (base.double().abs() + ref.abs()))
    dst = torch.empty(N, Hd, Wd, C, device=DEV)
    ops.resize_nhwc(src.to(DEV), dst, 0, relu=False)
    fwd = dst.cpu().double()
    lhs, rhs = float((fwd * g.double()).sum()), float((src.double() * got).sum())
    fmag = R.resize_nhwc(src, Hd, Wd)[1]
    tol = float(((R.BLEND_OPS * fmag + R.bil_slope_units(src, Hd, Wd)) * U * g.double().abs()).sum()) + \
        float((src.double().abs() * (rel * mag + 2 * U * (base.double().abs() + ref.abs()))).sum())
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ---- upsample_to_nchw and its adjoint -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", R.UPSAMPLE_CASES, ids=_id)
def test_upsample_to_nchw(case):
    from muscle_amd import ops
    N, K, lds, Hs, Ws, Hd, Wd = case
    src = R.upsample_inputs(case)[0]
    d_src = src.to(DEV)
    got = twice(lambda: ops.upsample_to_nchw(d_src, K, Hd, Wd))
    ref, mag = R.upsample_to_nchw(src, K, Hd, Wd)
    if (Hs, Ws) == (Hd, Wd):
        assert torch.equal(got, src[..., :K].permute(0, 3, 1, 2))
    check_elementwise(PROF, f"upsample_to_nchw {case}", got, ref, mag, float(R.BLEND_OPS), extra_abs=R.bil_slope_units(src[..., :K], Hd, Wd))


@pytest.mark.parametrize("accumulate", [0, 1])
@pytest.mark.parametrize("case", [c for c in R.UPSAMPLE_CASES if c != R.UPSAMPLE_FWD_ONLY], ids=_id)
def test_upsample_to_nchw_bwd(case, accumulate):
    """accumulate = 0 overwrites the K used columns of a NaN-filled gsrc; accumulate = 1 adds to a random base; the padding columns
    from K to lds keep what they held (NaN / the base) in both."""
    from muscle_amd import ops
    N, K, lds, Hs, Ws, Hd, Wd = case
    src, g, base = R.upsample_inputs(case)
    if not accumulate:
        base = torch.full_like(base, float("nan"))
    d_g = g.to(DEV)

    def run():
        gsrc = base.to(DEV)
        ops.upsample_to_nchw_bwd(d_g, gsrc, accumulate=bool(accumulate))
        return gsrc
    out = twice(run)
    pad, b_pad = out[..., K:], base[..., K:]
    assert bool(pad.isnan().all()) if not accumulate else torch.equal(pad, b_pad), "padding columns were written"
    ref, mag, e_ref, rel, share = R.adjoint_rule(g.permute(0, 2, 3, 1), Hs, Ws)
    assert rel < 0.1 * share, f"a dropped destination row could hide ({rel:.3g} >= {0.1 * share:.3g})"
    b = base[..., :K].double() if accumulate else torch.zeros_like(ref)
    got = out[..., :K].double() - b
    assert not bool(got.isnan().any()), "a used column was left unwritten"
    check_sums(PROF, f"upsample_to_nchw_bwd {case} acc={accumulate}", got, ref, mag, e_ref, rel, extra=2 * U * (b.abs() + ref.abs()))
    fwd = ops.upsample_to_nchw(src.to(DEV), K, Hd, Wd).cpu().double()
    lhs, rhs = float((fwd * g.double()).sum()), float((src[..., :K].double() * got).sum())
    fmag = R.upsample_to_nchw(src, K, Hd, Wd)[1]
    tol = float(((R.BLEND_OPS * fmag + R.bil_slope_units(src[..., :K], Hd, Wd)) * U * g.double().abs()).sum()) + \
        float((src[..., :K].double().abs() * (rel * mag + 2 * U * (b.abs() + ref.abs()))).sum())
    assert abs(lhs - rhs) <= tol, (lhs, rhs, tol)


# ---- row_l2norm ---------------------------------------------------------------------------------------------------------------
EPS = R.ROW_EPS
NAN = float("nan")


def _call(name, *args):
    from muscle_amd._lib import call, ptr, stream
    call(name, *(ptr(a) if isinstance(a, torch.Tensor) else a for a in args), stream())


@pytest.mark.parametrize("C", R.ROW_C)
@pytest.mark.parametrize("Rn", R.ROW_R)
def test_row_l2norm(Rn, C):
    """nrm by the sum rule on the square sum (all terms positive; the square root halves the relative error, not used); y = x * (1 /
    (nrm + eps)): the norm's allowance plus 4 operations (the products x*x are inside e_ref; add eps, reciprocal, product, and one
    for the rounding of nrm itself).  A zero row gives exactly 0.  One element's share of the norm is half its share 1/C of the sum
    (the condition is also checked in tests/test_cpu_dec_ref.py).  Both outputs start NaN-filled."""
    x, _ = R.row_inputs(Rn, C)
    d_x = x.to(DEV)

    def run():
        y, nrm = torch.full((Rn, C), NAN, device=DEV), torch.full((Rn,), NAN, device=DEV)
        _call("mx_row_l2norm", d_x, y, nrm, Rn, C, EPS)
        return y, nrm
    y, nrm = twice(run)
    ry, rn, my = R.row_l2norm(x, EPS)
    e_ref, rel = R.row_norm_rule(x)
    assert rel < 1.0 / (20.0 * C)
    check_sums(PROF, f"row_l2norm nrm {(Rn, C)}", nrm, rn, rn, e_ref, rel)
    check_elementwise(PROF, f"row_l2norm y {(Rn, C)}", y, ry, my, rel / U + 4.0)
    zero = (x == 0).all(1)
    assert bool((y[zero] == 0).all()) and bool((nrm[zero] == 0).all())


@pytest.mark.parametrize("C", R.ROW_C)
@pytest.mark.parametrize("Rn", R.ROW_R)
def test_row_l2norm_bwd(Rn, C):
    """gx = gy*inv - x*k, k = (gy.x) * inv^2 / n: the dot product by the sum rule (relative to sum |gy x|), 6 more operations (add
    eps, reciprocal, two products and a division in k, the two products and the subtraction share the rest); zero rows: gy / eps.
    gx starts NaN-filled."""
    x, gy = R.row_inputs(Rn, C)
    nrm = R.row_l2norm(x, EPS)[1].float()
    d = [t.to(DEV) for t in (x, nrm, gy)]

    def run():
        gx = torch.full((Rn, C), NAN, device=DEV)
        _call("mx_row_l2norm_bwd", d[0], d[1], d[2], gx, Rn, C, EPS)
        return gx
    gx = twice(run)
    ref, mag = R.row_l2norm_bwd(x, nrm, gy, EPS)
    e_ref, rel = R.row_dot_rule(x, gy)
    assert rel < 1.0 / (10.0 * C)
    check_elementwise(PROF, f"row_l2norm_bwd {(Rn, C)}", gx, ref, mag, rel / U + 6.0, e_ref / U)
    zero = (x == 0).all(1)
    if bool(zero.any()):
        assert bool(((gx[zero].double() - gy[zero].double() / EPS).abs() <= 3 * U * (gy[zero].double() / EPS).abs()).all())


# ---- pcm_norm -----------------------------------------------------------------------------------------------------------------
PCM_CASES = [(7, 20, 24), (7, 21, 24), (300, 23, 24), (R.GRID_CAP + 5, 20, 24)]
PCM_CHUNK = 1 << 18          # rows per float64 reference block: the case above the grid cap never holds a whole float64 copy


def _pcm_inputs(rows, K, L):
    gen = torch.Generator().manual_seed(R.case_seed(rows, K, L))
    return torch.rand(1, rows, L, generator=gen) + 0.5, torch.randn(1, rows, L, generator=gen)


@pytest.mark.parametrize("rows,K,L", PCM_CASES)
def test_pcm_norm(rows, K, L):
    """Forward: add eps, reciprocal, product (3 operations; 4 allowed); the padding columns from K on are written as zero over a
    canary.  (The case above the grid cap is 201 MB per tensor: the two runs never hold their outputs on the device together.)"""
    from muscle_amd import ops
    T, _ = _pcm_inputs(rows, K, L)
    d_T = T.to(DEV)
    out = twice(lambda: ops.pcm_norm(d_T, torch.full((1, rows, L), CANARY, device=DEV), K, EPS), frugal=True)[0]
    assert bool((out[:, K:] == 0).all())
    for lo in range(0, rows, PCM_CHUNK):
        ref, mag = R.pcm_norm(T[0, lo:lo + PCM_CHUNK], K, EPS)
        check_elementwise(PROF, f"pcm_norm {(rows, K, L)} rows {lo}+", out[lo:lo + PCM_CHUNK, :K], ref[:, :K], mag[:, :K], 4.0)


@pytest.mark.parametrize("rows,K,L", PCM_CASES)
def test_pcm_norm_bwd(rows, K, L):
    """Backward: as the forward for the K used columns; column K is a sum of K products times r^2: K + 4 operations of its
    magnitude; the columns after K are written as zero over a canary."""
    from muscle_amd import ops
    T, grv = _pcm_inputs(rows, K, L)
    d_T, d_g = T.to(DEV), grv.to(DEV)
    gT = twice(lambda: ops.pcm_norm(d_T, torch.full((1, rows, L), CANARY, device=DEV), K, EPS, grv=d_g), frugal=True)[0]
    assert bool((gT[:, K + 1:] == 0).all())
    for lo in range(0, rows, PCM_CHUNK):
        ref, mag = R.pcm_norm_bwd(T[0, lo:lo + PCM_CHUNK], grv[0, lo:lo + PCM_CHUNK], K, EPS)
        check_elementwise(PROF, f"pcm_norm bwd {(rows, K, L)} rows {lo}+", gT[lo:lo + PCM_CHUNK, :K + 1], ref[:, :K + 1], mag[:, :K + 1],
                          K + 4.0)


# ---- sym_relu_grad, ew, bcast_add ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B", [1, 3])
@pytest.mark.parametrize("n,ld", [(5, 5), (5, 52), (49, 49), (49, 52), (840, 844)])      # the last, at B = 3: above the grid cap
def test_sym_relu_grad(B, n, ld):
    """Integer inputs: (gaff + gaff^T) * (aff > 0) is exact; aff holds negatives and exact zeros; padding columns come out zero."""
    gen = torch.Generator().manual_seed(R.case_seed(B, n, ld))
    gaff = torch.randint(-9, 10, (B, n, ld), generator=gen).float()
    aff = torch.randint(-2, 3, (B, n, ld), generator=gen).float()
    assert bool((aff == 0).any()) and bool((aff < 0).any())
    d = gaff.to(DEV), aff.to(DEV)

    def run():
        out = torch.full((B, n, ld), CANARY, device=DEV)          # the padding columns must be WRITTEN as zero
        _call("mx_sym_relu_grad", d[0], d[1], out, B, n, ld)
        return out
    out = twice(run)
    assert torch.equal(out.double(), R.sym_relu_grad(gaff, aff, n))
    assert bool((out[:, :, n:] == 0).all())


@pytest.mark.parametrize("n", [1, 1001, R.GRID_CAP + 77])
def test_ew(n):
    """op 0: one product; op 1: a product and a sum (2; an fma only removes one); op 2: y > 0 selects a (+ b, one sum), with exact
    zeros and -0.0 in y selecting 0.  The alphas are fp32 numbers: the entry takes a float."""
    from muscle_amd import ops
    gen = torch.Generator().manual_seed(R.case_seed(n, 11))
    a, b = torch.randn(n, generator=gen), torch.randn(n, generator=gen)
    y = torch.randn(n, generator=gen)
    y[::3] = 0.0
    y[1::5] = -0.0
    d_a, d_b, d_y = a.to(DEV), b.to(DEV), y.to(DEV)
    for tag, fn, ref, k in (("op0", lambda: ops.ew(0, d_a, alpha=-1.75), R.ew(0, a, alpha=-1.75), 1.0),
                            ("op1", lambda: ops.ew(1, d_a, d_b, alpha=0.375), R.ew(1, a, b, alpha=0.375), 2.0),
                            ("op2+b", lambda: ops.ew(2, d_a, d_b, d_y), R.ew(2, a, b, y), 1.0),
                            ("op2", lambda: ops.ew(2, d_a, None, d_y), R.ew(2, a, None, y), 0.0)):
        got = twice(fn)
        if k == 0.0:
            assert torch.equal(got.double(), ref[0])
        else:
            check_elementwise(PROF, f"ew {tag} n={n}", got, ref[0], ref[1], k)
        if tag.startswith("op2"):
            assert bool((got[y <= 0] == 0).all())


@pytest.mark.parametrize("rows,C,rps", [(7, 4, 3), (7, 36, 3), (1, 4, 1), (10, 36, 4), (R.GRID_CAP // 9 * 4 + 7, 36, 100000)])
def test_bcast_add(rows, C, rps):
    """X[r] += alpha * v[r // rps] with rows_per_sample not dividing rows and alpha negative: a product and a sum (2)."""
    from muscle_amd import ops
    gen = torch.Generator().manual_seed(R.case_seed(rows, C, rps))
    X, v = torch.randn(rows, C, generator=gen), torch.randn(-(-rows // rps), C, generator=gen)
    d_v = v.to(DEV)

    def run():
        d_X = X.to(DEV)
        ops.bcast_add(d_X, d_v, -0.5, rps)
        return d_X
    ref, mag = R.bcast_add(X, v, -0.5, rps)
    check_elementwise(PROF, f"bcast_add {(rows, C, rps)}", twice(run), ref, mag, 2.0)
