"""Every entry of muscle_amd/csrc/dec.hip ALONE against the float64 restatements of tests/dec_ref.py (mx_resize_nhwc_bwd is in
tests/test_gpu_head_kernels.py, beside the resize it transposes), at the smallest shapes that reach each branch: a second sweep of
every grid-stride loop (more than 8192 x 256 items), workgroups of field_edge_kernel that span two and three samples, its f >= 64
path, the 2048-partial cap of the square sum, the opted-in LDS tile of field_tile_gather_kernel, arg-max ties.  The case tables
are in dec_ref.py; tests/test_cpu_dec_ref.py checks their input conditions on the reference alone.  Every case runs twice and must
give the same bits (field_scatter mode 0 adds with float atomics by design: tolerance only); outputs carry canaries (or NaN) where
the kernel must not write (or must overwrite).

Tolerances, by the rule of tests/test_gpu_bn_kernels.py, in units of U = 2^-24 times the magnitude dec_ref returns:
  exact regimes     torch.equal: avgpool on integers below 2^20 (every 9-term sum is exact; the result is float32(sum) * float32(1/9)),
                    the point lists and counts of field_select, untouched and zeroed regions;
  elementwise       k*U*magnitude, k = the arithmetic operations on the path (stated at each test);
  transcendentals   (__expf / __logf / expf / atan2f paths) the error of the plain fp32 torch restatement against float64 is
                    MEASURED once per option set on a fixed large draw of the same distribution (dec_ref.ce_bwd_units, edge_calib,
                    gather_calib; elements below the smallest normal number left out) and the kernel is allowed 4x that, plus
                    one subnormal absolutely where a result may be flushed;
  sums              (4*e_ref + 2U) * sum|term|, e_ref = the fp32 restatement's error on the same inputs; asserted with it where a
                    sum has at most 100 000 terms: the allowance is below a tenth of one term's share.  Longer sums (ce loss,
                    clip norm) cannot meet that in fp32 (2U alone is above it): they have an exact regime instead, integer terms
                    whose every partial sum is exact, asserted with torch.equal, where one dropped term moves the last places;
  discontinuous     orient is compared where dec_ref.orient_compare_mask says (magnitude floor, 4x the measured angle error - of
                    the fixed draw or of the case, the larger - away from every sector boundary); field_terms' inputs clear their decision margins by construction.
No tolerance is taken from a kernel's output.  DEC_KERNELS_PROFILE=<file> records every case's figures (profiles/dec_kernels_error.txt; the pair of files shares it).
"""
import numpy as np
import pytest
import torch

import dec_ref as R
from dec_ref import F32, U
from dec_gpu_util import CANARY, DEV, FLUSH, Profile, check_elementwise, check_sums, twice

pytestmark = pytest.mark.gpu

PROF = Profile("tests/test_gpu_dec_kernels.py")
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _profile_file():
    yield
    PROF.write()


def _call(name, *args):
    from muscle_amd._lib import call, stream
    call(name, *args, stream())


def _p(t):
    from muscle_amd._lib import ptr
    return ptr(t)


def _id(c):
    return "x".join(map(str, c))


# ---- avgpool3s2 ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("bwd", [0, 1], ids=["fwd", "bwd"])
@pytest.mark.parametrize("exact", [True, False], ids=["exact", "random"])
@pytest.mark.parametrize("shape", R.AVGPOOL_SHAPES, ids=_id)
def test_avgpool3s2(shape, exact, bwd):
    """Forward and adjoint; the output starts NaN-filled (the backward must overwrite, dec.py hands it empty_like).  Random regime:
    eight additions, the rounding of 1/9 and the product: 10 operations of sum |x| / 9."""
    N, H, W, C = shape
    Ho, Wo = (H - 1) // 2 + 1, (W - 1) // 2 + 1
    gen = torch.Generator().manual_seed(R.case_seed(*shape, exact, bwd))
    ishape, oshape = ((N, Ho, Wo, C), (N, H, W, C)) if bwd else ((N, H, W, C), (N, Ho, Wo, C))
    x = torch.randint(-2 ** 20 + 1, 2 ** 20, ishape, generator=gen).float() if exact else torch.randn(ishape, generator=gen)
    d_x = x.to(DEV)

    def run():
        y = torch.full(oshape, NAN, device=DEV)
        _call("mx_avgpool3s2", _p(d_x), _p(y), N, H, W, C, bwd)
        return y
    got = twice(run)
    if exact:
        assert torch.equal(got, R.avgpool3s2_exact(x, bool(bwd), H, W))
    else:
        ref, mag = R.avgpool3s2_bwd(x, H, W) if bwd else R.avgpool3s2(x)
        check_elementwise(PROF, f"avgpool3s2 {shape} bwd={bwd}", got, ref, mag, 10.0)


# ---- ce_argmax ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("kind", ["spread", "confident"])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_argmax_forward(shape, kind):
    """loss[0] += mean over pixels of (log sum exp - seg[label]), label = the first maximum of the mask (zero pixels, two and three
    equal maxima); loss[0] starts at 0.75 and the 8 bytes of scratch hold garbage."""
    N, K, HW = shape
    seg, mask = R.ce_inputs(shape, kind)
    d_seg, d_mask = seg.to(DEV), mask.to(DEV)

    def run():
        loss = torch.full((1,), 0.75, device=DEV)
        ws = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        _call("mx_ce_argmax", _p(d_seg), _p(d_mask), None, _p(loss), None, N, K, HW, 0, ws.data_ptr(), 8)
        return loss
    got = twice(run).double() - 0.75
    ref, mag, e_ref, rel = R.ce_fwd_rule(seg, mask)
    if N * HW <= 100000:
        assert rel < 1.0 / (10.0 * N * HW)
    check_sums(PROF, f"ce_argmax fwd {shape} {kind}", got, ref.reshape(1), mag.reshape(1), e_ref, rel,
               extra=2 * U * (0.75 + abs(float(ref))))


@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_argmax_forward_exact(shape):
    """The exact regime of dec_ref.ce_exact_inputs: every term is an integer 20..27 and every partial sum is exact, so the loss
    (from 0) is float32(sum / (N*HW)) bit for bit.  This is what shows a dropped or doubled pixel in the sums of more than
    100 000 terms, where the sum rule's allowance is above one term's share."""
    N, K, HW = shape
    seg, mask, want = R.ce_exact_inputs(shape)
    d_seg, d_mask = seg.to(DEV), mask.to(DEV)

    def run():
        loss = torch.zeros(1, device=DEV)
        ws = torch.full((1,), 0x5A5A5A5A5A5A5A5A, dtype=torch.int64, device=DEV)
        _call("mx_ce_argmax", _p(d_seg), _p(d_mask), None, _p(loss), None, N, K, HW, 0, ws.data_ptr(), 8)
        return loss
    got = twice(run)
    assert torch.equal(got, want), (float(got), float(want))


@pytest.mark.parametrize("kind", ["spread", "confident"])
@pytest.mark.parametrize("shape", R.CE_SHAPES, ids=_id)
def test_ce_argmax_backward(shape, kind):
    """gseg = gup * (softmax - onehot) / (N*HW) with gup = 0.37, over a NaN-filled gseg."""
    N, K, HW = shape
    seg, mask = R.ce_inputs(shape, kind)
    d_seg, d_mask = seg.to(DEV), mask.to(DEV)
    gup = torch.full((1,), 0.37, device=DEV)

    def run():
        gseg = torch.full((N, K, HW), NAN, device=DEV)
        _call("mx_ce_argmax", _p(d_seg), _p(d_mask), _p(gup), None, _p(gseg), N, K, HW, 1, None, 0)
        return gseg
    got = twice(run)
    ref, mag = R.ce_argmax_bwd(seg, mask, R.CE_GUP)
    u = R.ce_bwd_units(kind)
    check_elementwise(PROF, f"ce_argmax bwd {shape} {kind}", got, ref, mag, 4.0 * u, u, extra_abs=FLUSH)


# ---- clip_grad_norm -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", R.CLIP_N)
def test_clip_grad_norm_exact(n):
    """The exact regime of dec_ref.clip_exact_inputs: every element +-4, the fp64 square sum 16 n exact, the norm float32(sqrt(16 n))
    bit for bit - one element dropped or doubled among a million moves its last places; max_norm is far above it, so the vector
    comes back unchanged."""
    x, want = R.clip_exact_inputs(n)
    d_x = x.to(DEV)

    def run():
        v = d_x.clone()
        sq = torch.full((2048,), NAN, dtype=torch.float64, device=DEV)
        norm = torch.full((1,), CANARY, device=DEV)
        _call("mx_clip_grad_norm", _p(v), n, 1e9, _p(sq), _p(norm))
        return v, norm
    v, norm = twice(run)
    assert torch.equal(norm, want), (float(norm), float(want))
    assert torch.equal(v, x)


@pytest.mark.parametrize("scenario", R.CLIP_SCENARIOS)
@pytest.mark.parametrize("n", R.CLIP_N)
def test_clip_grad_norm(n, scenario):
    """norm by the sum rule (all terms positive); the scaled vector: the norm's allowance plus the addition of 1e-6, the division
    and the product (3).  Below max_norm and for an all-zero vector the input comes back bit for bit.  'equal': max_norm =
    float32(norm + 1e-6), either outcome of coef >= 1 is accepted but the vector must be the one the REPORTED norm implies.  The
    scratch of 2048 doubles is NaN-filled: the kernel must write every partial it reads."""
    x, mx = R.clip_inputs(n, scenario)
    d_x = x.to(DEV)

    def run():
        v = d_x.clone()
        sq = torch.full((2048,), NAN, dtype=torch.float64, device=DEV)
        norm = torch.full((2,), CANARY, device=DEV)
        _call("mx_clip_grad_norm", _p(v), n, mx, _p(sq), None if scenario == "nonorm" else _p(norm))
        return v, norm
    v, norm = twice(run)
    assert float(norm[1]) == CANARY
    ref_n, ref_v, e_ref, rel = R.clip_rule(x, mx)
    if n <= 100000:
        assert rel < 1.0 / (20.0 * n)            # the norm moves by half of an element's share of the square sum
    if scenario == "nonorm":
        assert float(norm[0]) == CANARY
    else:
        check_sums(PROF, f"clip_grad_norm norm n={n} {scenario}", norm[:1], ref_n.reshape(1), ref_n.reshape(1), e_ref, rel)
    if scenario == "zero":
        assert float(norm[0]) == 0.0 and torch.equal(v, x)
    elif scenario == "below":
        assert torch.equal(v, x)
    elif scenario == "equal":
        c32 = min(np.float32(mx) / (np.float32(float(norm[0])) + np.float32(1e-6)), np.float32(1.0))
        if c32 >= np.float32(1.0):
            assert torch.equal(v, x)
        else:
            assert torch.equal(v, x * torch.tensor(c32))
    else:
        check_elementwise(PROF, f"clip_grad_norm vector n={n} {scenario}", v, ref_v, ref_v.abs(), rel / U + 3.0)


# ---- field_edges --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("beta", R.EDGE_BETAS)
@pytest.mark.parametrize("shape", R.EDGE_SHAPES, ids=_id)
def test_field_edges(shape, beta):
    """prob, mag, edge_fg at 4x the error measured on the fixed draw (dec_ref.edge_calib); mx at the tolerance of mag (the largest over its plane), exactly 0 where
    unlabelled (it starts as garbage: the entry zero-fills it); unlabelled planes exactly sqrtf(1e-8f) with sector 7; orient
    where the float64 angle is clear of every sector boundary.  The band around the boundaries is 4x the fp32 restatement's angle error
    on the calibration draw or on the case itself, whichever is larger: the angle error is set by the pixels just above the magnitude
    floor, and the 2.1 M pixel single-class case has thousands of them where the 64 x 64 draw has none (restatement error 3.4e-4
    against 2.9e-6 at beta = 2; under the draw's band alone the plain fp32 restatement itself is one sector off there)."""
    N, K, H, W = shape
    Fg, HW = K - 1, H * W
    seg, lab = R.edge_inputs(shape, beta)
    d_seg, d_lab = seg.to(DEV), lab.to(DEV)

    def run():
        prob, mag = torch.full((N, Fg, HW), NAN, device=DEV), torch.full((N, Fg, HW), NAN, device=DEV)
        orient = torch.full((N, Fg, HW), 99, dtype=torch.uint8, device=DEV)
        mx = torch.full((N * Fg,), 0x7F7F7F7F, dtype=torch.int32, device=DEV)
        edge = torch.full((N, H, W), NAN, device=DEV)
        _call("mx_field_edges", _p(d_seg), _p(d_lab), beta, _p(prob), _p(mag), _p(orient), _p(mx), _p(edge), N, K, H, W)
        return prob, mag, orient, mx, edge
    prob, mag, orient, mx, edge = twice(run)
    ref = R.field_edges(seg, lab, beta)
    up, um, ue, ang = R.edge_calib(beta)
    ang = max(ang, R.angle_error(seg, lab, beta, ref))      # the exclusion band, not an allowance: see the docstring
    tag = f"field_edges {shape} beta={beta:g}"
    check_elementwise(PROF, tag + " prob", prob.view(N, Fg, H, W), ref["prob"], ref["prob"], 4.0 * up, up, extra_abs=FLUSH)
    check_elementwise(PROF, tag + " mag", mag.view(N, Fg, H, W), ref["mag"], ref["mag_m"], 4.0 * um, um)
    check_elementwise(PROF, tag + " edge_fg", edge, ref["edge_fg"], ref["mag_m"].sum(1), 4.0 * ue, ue)
    lb = ref["labelled"]
    unl = ~lb.reshape(N, Fg, HW)
    assert bool((mag[unl] == R.M_ZERO).all()) and bool((orient[unl] == 7).all())
    mxf = mx.view(torch.float32).view(N, Fg)
    assert bool((mx.view(N, Fg)[lab == 0] == 0).all())
    mtol = (4.0 * um * U * ref["mag_m"]).flatten(2).max(-1).values
    assert bool(((mxf.double() - ref["mx"]).abs() <= mtol)[lab != 0].all())
    cmp_, floor = R.orient_compare_mask(ref, ang)
    base = int(lb.sum()) if beta < 10 else int(floor.sum())
    if base:
        assert int(cmp_.sum()) >= 0.95 * base
    bad = int((orient.view(N, Fg, H, W).long() != ref["orient"])[cmp_].sum())
    PROF.record(tag + " orient", compared=float(cmp_.sum()), of=float(base), differ=float(bad), angle_err=ang)
    assert bad == 0, f"{bad} sectors differ away from every boundary"


# ---- field_select -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", R.SELECT_STEPS)
@pytest.mark.parametrize("hw", R.SELECT_HW, ids=_id)
def test_field_select(hw, step):
    """Counts and the first `count` entries of both lists, in order, exactly; the tails keep their canaries."""
    H, W = hw
    mag, orient, mx, slots = R.select_inputs(H, W)
    S, HW = len(slots), H * W
    d = mag.to(DEV), orient.to(DEV), mx.view(torch.int32).to(DEV), torch.tensor(slots, dtype=torch.int32, device=DEV)

    def run():
        ol, il = torch.full((S, HW), -1234567, dtype=torch.int32, device=DEV), torch.full((S, HW), -1234567, dtype=torch.int32, device=DEV)
        cnt = torch.full((S, 3), -1, dtype=torch.int32, device=DEV)
        _call("mx_field_select", _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), S, step, _p(ol), _p(il), _p(cnt), mag.shape[1], H, W)
        return ol, il, cnt
    ol, il, cnt = twice(run)
    outs, ins, counts = R.field_select(mag.numpy(), orient.numpy(), mx.numpy(), slots, step, H, W)
    assert cnt.tolist() == counts.tolist()
    for s in range(S):
        for got, want in ((ol[s], outs[s]), (il[s], ins[s])):
            assert got[:len(want)].tolist() == want.tolist(), (slots[s], step)
            assert bool((got[len(want):] == -1234567).all()), "a list tail was written"


# ---- field_gather -------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("geo", R.GATHER_GEO, ids=_id)
@pytest.mark.parametrize("kml", range(3))
@pytest.mark.parametrize("ch", range(5))
def test_field_gather(ch, kml, geo):
    """Channel softmax of the point values (mode 0: NCHW pixel, mode 1: bilinear from the low-resolution NHWC map) and the class
    softmax of the mask padded with zeros to ML columns; points at the corners, on the last row and column, repeated."""
    CH, (K, ML), npts = R.GATHER_CH[ch], R.GATHER_KML[kml], R.GATHER_NPTS[(ch + kml) % 3]
    mode, h, w, H, W = geo
    dense, mask, pts = R.gather_inputs(geo, CH, K, npts)
    d = dense.to(DEV), mask.to(DEV), pts.to(DEV)

    def run():
        feat, mfeat = torch.full((npts, CH), NAN, device=DEV), torch.full((npts, ML), NAN, device=DEV)
        _call("mx_field_gather", _p(d[0]), mode, h, w, _p(d[1]), _p(d[2]), npts, _p(feat), _p(mfeat), CH, K, ML, H, W)
        return feat, mfeat
    feat, mfeat = twice(run)
    rf, rm = R.field_gather(dense, mode, mask, pts, K, ML, H, W)
    uf, um = R.gather_calib(mode)
    tag = f"field_gather {geo} CH={CH} K={K} npts={npts}"
    check_elementwise(PROF, tag + " feat", feat, rf, rf, 4.0 * uf, uf, extra_abs=FLUSH)
    check_elementwise(PROF, tag + " mfeat", mfeat[:, :K], rm[:, :K], rm[:, :K], 4.0 * um, um, extra_abs=FLUSH)
    assert bool((mfeat[:, K:] == 0).all())


# ---- field_terms --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.TERMS_S)
@pytest.mark.parametrize("k", R.TERMS_K)
def test_field_terms(k, S):
    """The slot terms by the sum rule (relative to the sum of the eight |terms|), loss[0] = 0.75 + their sum (S more additions),
    gsim = sign/(k*cnt) * inv_n for the row + the same for the column: a division, a product and the sum (4 allowed) of the
    magnitude dec_ref returns.  inv_n = 0.5; the class decisions are clear of their margins (tests/test_cpu_dec_ref.py)."""
    sim, simm = R.terms_inputs(k, S)
    d_sim, d_simm = sim.to(DEV), simm.to(DEV)

    def run():
        loss = torch.full((1,), 0.75, device=DEV)
        gsim, slot = torch.full((S, k, k), NAN, device=DEV), torch.full((S,), NAN, device=DEV)
        _call("mx_field_terms", _p(d_sim), _p(d_simm), S, k, 0.5, _p(loss), _p(gsim), _p(slot))
        return loss, gsim, slot
    loss, gsim, slot = twice(run)
    ref, r32 = R.field_terms(sim, simm, 0.5), R.field_terms(sim, simm, 0.5, F32)
    assert torch.equal(ref["counts"], r32["counts"])
    mag = ref["terms"].abs().sum((1, 2)) * 0.5
    e_ref = float(((r32["slot_loss"].double() - ref["slot_loss"]).abs() / mag).max())
    rel = 4.0 * e_ref + 2.0 * U
    assert rel < 1.0 / (10.0 * 8)
    check_sums(PROF, f"field_terms slot k={k} S={S}", slot, ref["slot_loss"], mag, e_ref, rel)
    total = float(ref["slot_loss"].sum())
    tol = rel * float(mag.sum()) + (S + 2) * U * (0.75 + float(ref["slot_loss"].abs().sum()))
    assert abs(float(loss[0]) - 0.75 - total) <= tol
    check_elementwise(PROF, f"field_terms gsim k={k} S={S}", gsim, ref["gsim"], ref["gsim_m"], 4.0)


# ---- field_scatter ------------------------------------------------------------------------------------------------------------
def _scatter_case(h, w, CH, mode, gup, once=False):
    c = R.scatter_rule(h, w, CH, mode, gup)
    feat, gfeat, pts, base, N, H, W = (c[k] for k in ("feat", "gfeat", "pts", "base", "N", "H", "W"))
    d = feat.to(DEV), gfeat.to(DEV), pts.to(DEV)
    d_gup = torch.full((1,), gup, device=DEV) if gup is not None else None

    def run():
        gd = base.to(DEV)
        gpt = torch.full((40, CH), NAN, device=DEV) if mode == 1 else None
        _call("mx_field_scatter", _p(d[0]), _p(d[1]), _p(d[2]), 40, mode, h if mode else 0, w if mode else 0, _p(d_gup), _p(gd),
              _p(gpt), N, CH, H, W)
        return gd
    if once:
        out = run().cpu()
    else:
        out = twice(run)
    assert torch.equal(out[1], base[1]), "the sample without points was written"
    ref, mag, e_ref, rel, share, atomics = (c[k] for k in ("ref", "mag", "e_ref", "rel", "share", "atomics"))
    assert rel + atomics < 0.1 * share, f"a dropped point could hide ({rel + atomics:.3g} >= {0.1 * share:.3g})"
    if mode == 1 and h > 8 and w > 8:
        Wy, Wx = R.bil_matrix(h, H)[int(pts[16, 1]) // W], R.bil_matrix(w, W)[int(pts[16, 1]) % W]
        assert Wy[7] > 0 and Wy[8] > 0 and Wx[7] > 0 and Wx[8] > 0          # corners in four 8 x 8 tiles
    check_sums(PROF, f"field_scatter mode={mode} {(h, w)} CH={CH} gup={gup}", out.double() - base.double(), ref, mag, e_ref, rel,
               extra=2 * U * (base.double().abs() + ref.abs()) + atomics * (base.double().abs() + mag))


@pytest.mark.parametrize("ch", range(5))
@pytest.mark.parametrize("hw", range(4))
def test_field_scatter_lowres(hw, ch):
    """Mode 1: per-point gradient rows, then the ordered tile gather into a non-zero gdense; gup NULL and 0.37 alternate."""
    (h, w), CH = R.SCATTER_HW[hw], R.SCATTER_CH[ch]
    _scatter_case(h, w, CH, 1, R.scatter_gup(hw, ch, 1))


@pytest.mark.parametrize("ch", range(2))
@pytest.mark.parametrize("hw", range(4))
def test_field_scatter_fullres_atomics(hw, ch):
    """Mode 0: float atomics into the NCHW gradient, order not fixed: tolerance only (each of up to 40 additions onto an element
    rounds at the running value, at most |base| + sum |term|, on top of the sum rule)."""
    (h, w), CH = R.SCATTER_HW[hw], R.SCATTER_CH[ch]
    _scatter_case(h, w, CH, 0, R.scatter_gup(hw, ch, 0), once=True)
