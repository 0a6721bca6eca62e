"""Every compiled instantiation of the forward / data-gradient GEMM kernels of muscle_amd/csrc/gemm.hip (gemm_nt_kernel,
gemm_nt_split_kernel, gemm_nt_split3_kernel) alone against float64, at the smallest shape its launch planner sends there
(tests/gemm_nt_cases.py, written by tools/gemm_unit_cases.py from the query mx_pw_fwd_plan), plus the paths no workload shape pins:
the non-lean epilogue, the XCD-ordered and chunked 1-D grids with early-return tiles, batch strides, lda > K / ldc > N, SE-gate
boundaries inside a tile, the K tails; and split_planes_kernel / the transposes bit for bit.

Every case runs on hostile buffers: the operands are slices of wider, taller tensors with NaN everywhere else, the outputs are
slices of buffers holding NaN inside and a fixed bit pattern outside.  Bounds: outputs within 2 * e32 + 2e-7 * max|ref| of float64
(e32 = the error of a CPU float32 evaluation of the same case; the rule of test_gpu_irn_walk.py / test_gpu_irn_net.py), statistics
within the a-priori bound of 128 fp32 additions of the float32 values the kernel stored; sentinels,
repeat runs, transposes, the image and power-of-two scaling exactly.  The module sets the arithmetic mode of each case itself."""
import math
import time

import numpy as np
import pytest
import torch

import gemm_ref as gr
from gemm_nt_cases import SMALLEST

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
ENTRY = {"fwd": 0, "bgemm": 0, "planes": 1, "planes_act": 1, "bnbwd_planes": 1}
PATTERN = 0x5A5A5A5A                      # outside every output slice (as a float: 1.5e16)
STATS_TAIL = 512                          # floats of pattern behind the statistics rows

# (id, route, a_mode, arithmetic mode, M, K, N, batch, epilogue options, rows_per_sample, plan): paths the smallest shapes leave out
EXTRA = [
    ("x_n21", "fwd", 0, 0, 123, 36, 21, 1, "bias+res+relu", 1, 10320),                 # N % 4 != 0 inside one tile: scalar stores
    ("x_n130_split", "fwd", 0, 2, 251, 40, 130, 1, "bias+relu+stats", 1, 20640),       # ... and across three tiles of the first split kernel
    ("x_planes_n130", "planes", 0, 1, 251, 48, 130, 1, "bias+res+relu+stats", 1, 30640),
    ("x_bgemm_f1", "bgemm", 0, 0, 251, 20, 70, 3, "relu", 1, 10320),                   # batch strides sa / sb / sc with gaps
    ("x_bgemm_f2", "bgemm", 0, 2, 251, 24, 130, 3, "relu", 1, 20640),
    ("x_rps_gt_m_f1", "fwd", 1, 0, 123, 16, 40, 1, "stats", 130, 10320),               # one sample longer than the matrix
    ("x_rps_gt_m_f2", "fwd", 1, 2, 123, 16, 40, 1, "stats", 130, 20640),
    ("x_rps_gt_m_f3", "planes_act", 1, 1, 123, 32, 48, 1, "stats", 130, 30640),
    ("x_rps49_f2", "fwd", 1, 2, 251, 32, 72, 1, "", 49, 20640),                        # several sample boundaries inside a tile
    ("x_rps49_f3", "planes_act", 1, 1, 251, 64, 48, 1, "stats", 49, 30640),
    ("x_bnbwdp_nt3", "bnbwd_planes", 3, 1, 251, 64, 130, 1, "res", 1, 30640),
    ("x_ldc_odd_f1", "fwd", 0, 0, 251, 16, 64, 1, "res+stats+ldc_odd", 1, 10320),      # N % 4 == 0 but ldc % 4 != 0: no 16-byte stores
    ("x_ldc_odd_f2", "fwd", 0, 2, 251, 16, 64, 1, "res+stats+ldc_odd", 1, 20640),
]
CASES = SMALLEST + EXTRA
RESULTS = []                              # (id, plan, M, K, N, err, e32, limit, seconds)


def _family(plan):
    return plan // 10000


class _Slice:
    """A [batch, rows, cols] slice of a wider, taller buffer: one row above, two below, four columns to the left, at least four to
    the right (so that the slice starts 16-byte aligned whenever the leading dimension is a multiple of 4)."""

    def __init__(self, batch, rows, cols, *, odd_ld=False, outside=float("nan"), inside=None):
        self.rows, self.cols, self.batch = rows, cols, batch
        self.ld = cols + 8 + (-cols) % 4 + (1 if odd_ld else 0)
        self.buf = torch.empty(batch, rows + 3, self.ld, dtype=torch.float32, device=DEV)
        if isinstance(outside, int):
            self.buf.view(torch.int32).fill_(outside)
        else:
            self.buf.fill_(outside)
        self.view = self.buf[:, 1:1 + rows, 4:4 + cols]
        if inside is None:
            self.view.fill_(float("nan"))
        else:
            self.view.copy_(inside.reshape(batch, rows, cols))
        self.ptr = self.buf.data_ptr() + 4 * (self.ld + 4)
        self.stride = (rows + 3) * self.ld

    def outside_untouched(self):
        chk = self.buf.clone()
        chk[:, 1:1 + self.rows, 4:4 + self.cols] = torch.tensor([PATTERN], dtype=torch.int32).view(torch.float32).item()
        return bool((chk.view(torch.int32) == PATTERN).all())


def _data(case, seed):
    """CPU float32 operands of a case"""
    cid, route, a_mode, _, M, K, N, batch, opts, rps, _ = case
    g = torch.Generator().manual_seed(1000 + seed)
    d = {"A": torch.randn(batch, M, K, generator=g), "W": torch.randn(batch if route == "bgemm" else 1, N, K, generator=g) * K ** -0.5}
    if a_mode in (gr.BNACT, gr.AFFINE):
        d["scale"] = torch.rand(K, generator=g) + 0.5
        d["shift"] = torch.randn(K, generator=g) * 0.3
    if a_mode == gr.BNACT:
        d["gate"] = torch.rand((M + rps - 1) // rps, K, generator=g)
    if a_mode == gr.BNBWD:
        d["X"] = torch.randn(M, K, generator=g)
        d["coef"] = torch.stack([torch.rand(K, generator=g) + 0.5, torch.randn(K, generator=g) * 0.3, torch.randn(K, generator=g) * 0.1])
    if "bias" in opts:
        d["bias"] = torch.randn(N, generator=g)
    if "res" in opts:
        d["res"] = torch.randn(batch, M, N, generator=g)
    return d


def _reference(case, d, dtype):
    _, _, a_mode, _, M, K, N, batch, opts, rps, _ = case
    outs = []
    for b in range(batch):
        Ap = gr.prologue(a_mode, d["A"][b], scale=d.get("scale"), shift=d.get("shift"), gate=d.get("gate"), rps=rps, X=d.get("X"),
                         coef=d.get("coef"), dtype=dtype)
        res = d["res"][b] if "res" in d else None
        outs.append(gr.gemm(Ap, d["W"][min(b, d["W"].shape[0] - 1)], d.get("bias"), res, "relu" in opts))
    return torch.stack(outs)


def _execute(case, d):
    """One launch of the case's entry point on fresh hostile buffers -> (C slice, statistics buffer or None)"""
    from muscle_amd import ops
    from muscle_amd._lib import call, lib, stream
    _, route, a_mode, _, M, K, N, batch, opts, rps, _ = case
    A = _Slice(batch, M, K, inside=d["A"].to(DEV))
    C = _Slice(batch, M, N, odd_ld="ldc_odd" in opts, outside=PATTERN)
    R = _Slice(batch, M, N, odd_ld="ldc_odd" in opts, inside=d["res"].to(DEV)) if "res" in d else None
    dev = {k: d[k].to(DEV).contiguous() for k in ("scale", "shift", "gate", "coef", "bias") if k in d}
    p = lambda k: dev[k].data_ptr() if k in dev else None
    stats, P = None, 0
    if "stats" in opts:
        P = lib().mx_pw_fwd_parts(M, N, K)
        stats = torch.empty(P * 2 * N + STATS_TAIL, dtype=torch.float32, device=DEV)
        stats.view(torch.int32).fill_(PATTERN)
        stats[:P * 2 * N] = float("nan")
    sp = stats.data_ptr() if stats is not None else None
    rp = R.ptr if R is not None else None
    relu = int("relu" in opts)
    keep = [dev, A, R]
    X = None
    if a_mode == gr.BNBWD:
        X = _Slice(1, M, K, inside=d["X"].to(DEV))
        assert X.ld == A.ld
    if route in ("planes", "planes_act", "bnbwd_planes"):
        W = d["W"][0].to(DEV).contiguous()
        plan = ops.PlanesPlan([W])
        (image,) = plan.run()
        assert image is not None
        keep += [W, plan]
    if route == "fwd":
        W = d["W"][0].to(DEV).contiguous()
        call("mx_pw_fwd", A.ptr, a_mode, p("scale"), p("shift"), p("gate"), rps, W.data_ptr(), C.ptr, M, K, N, A.ld, C.ld, p("bias"), rp, relu,
             sp, stream())
    elif route == "bgemm":
        B = _Slice(batch, N, K, inside=d["W"].to(DEV))
        assert A.stride > M * A.ld and B.stride > N * B.ld and C.stride > M * C.ld
        call("mx_bgemm", 0, A.ptr, B.ptr, C.ptr, M, N, K, A.ld, B.ld, C.ld, A.stride, B.stride, C.stride, batch, relu, stream())
    elif route == "planes":
        call("mx_pw_fwd_planes", A.ptr, image, C.ptr, M, K, N, A.ld, C.ld, p("bias"), rp, relu, sp, stream())
    elif route == "planes_act":
        call("mx_pw_fwd_planes_act", A.ptr, p("scale"), p("shift"), p("gate"), rps, image, C.ptr, M, K, N, A.ld, C.ld, sp, stream())
    else:
        call("mx_pw_dgrad_bnbwd_planes", A.ptr, X.ptr, p("coef"), image, C.ptr, M, K, N, A.ld, C.ld, rp, stream())
    torch.cuda.synchronize()
    del keep
    return C, stats


def _bits_equal(a, b):
    return torch.equal(a.view(torch.int32), b.view(torch.int32))


def _set_mode_and_check_plan(case):
    import muscle_amd
    from muscle_amd._lib import lib
    _, route, a_mode, gmode, M, K, N, batch, _, _, plan = case
    muscle_amd.set_gemm_mode(gmode)
    got = lib().mx_pw_fwd_plan(ENTRY[route], a_mode, M, K, N, batch)
    assert got == plan, f"the planner now answers {got} for this shape, the table says {plan}: regenerate tests/gemm_nt_cases.py"


@pytest.mark.parametrize("case", CASES, ids=[c[0] for c in CASES])
def test_gemm_nt_instantiation_vs_fp64(case):
    import muscle_amd
    from muscle_amd._lib import lib
    t0 = time.perf_counter()
    cid, route, a_mode, gmode, M, K, N, batch, opts, rps, plan = case
    d = _data(case, CASES.index(case))
    ref = _reference(case, d, torch.float64)
    e32 = float((_reference(case, d, torch.float32).double() - ref).abs().max())
    scale = float(ref.abs().max())
    before = muscle_amd.get_gemm_mode()
    try:
        _set_mode_and_check_plan(case)
        runs = [_execute(case, d) for _ in range(2)]
    finally:
        muscle_amd.set_gemm_mode(before)
    (C, stats), (C2, stats2) = runs
    # run to run: the same bits everywhere, sentinels included
    assert _bits_equal(C.buf, C2.buf)
    assert stats is None or _bits_equal(stats, stats2)
    del C2, stats2, runs
    # every element inside written, nothing outside touched
    assert bool(torch.isfinite(C.view).all()), "an output element inside [M, N] was not written (or is not finite)"
    assert C.outside_untouched(), "a store outside the [M, N] slice"
    err = float((C.view.double() - ref.to(DEV)).abs().max())
    limit = 2.0 * e32 + 2e-7 * scale
    print(f"\nGEMMUNIT {cid} plan={plan} M={M} K={K} N={N} b={batch} a_mode={a_mode} opts='{opts}' rps={rps}: err={err:.3e} e32={e32:.3e} "
          f"err/e32={err / max(e32, 1e-300):.2f} limit={limit:.3e} err/limit={err / limit:.3f}")
    assert err <= limit
    if stats is not None:
        P = lib().mx_pw_fwd_parts(M, N, K)
        assert P == (M + 127) // 128
        assert bool((stats[P * 2 * N:].view(torch.int32) == PATTERN).all()), "a statistics store past the [P, 2, N] rows"
        st = stats[:P * 2 * N].view(P, 2, N).double()
        assert bool(torch.isfinite(st).all()), "a statistics element was not written"
        s, q, sabs = gr.tile_stats(C.view[0])
        es = float(((st[:, 0] - s).abs() - gr.STATS_EPS * sabs).max())
        eq = float(((st[:, 1] - q).abs() - gr.STATS_EPS * q).max())
        rs = float(((st[:, 0] - s).abs() / (gr.STATS_EPS * sabs).clamp_min(1e-300)).max())
        rq = float(((st[:, 1] - q).abs() / (gr.STATS_EPS * q).clamp_min(1e-300)).max())
        print(f"GEMMUNIT {cid} statistics: worst |sum - ref| / bound = {rs:.3f}, worst |sumsq - ref| / bound = {rq:.3f}")
        assert es <= 0.0 and eq <= 0.0
    RESULTS.append((cid, plan, M, K, N, err, e32, limit, time.perf_counter() - t0))


@pytest.mark.parametrize("route,gmode,K", [("fwd", 0, 40), ("fwd", 2, 40), ("planes", 1, 48)], ids=["fp32", "split", "planes"])
def test_plain_gemm_commutes_with_powers_of_two(route, gmode, K):
    """A * 2^-20 against W * 2^12 gives exactly 2^-8 times the output bits: truncation splitting, the products and fp32 accumulation
    all commute with powers of two away from underflow, in exact fp32 and in both split generations."""
    import muscle_amd
    case = ("scale", route, 0, gmode, 251, K, 70, 1, "", 1, None)
    d = _data(case, 77)
    d2 = dict(d, A=d["A"] * 2.0 ** -20, W=d["W"] * 2.0 ** 12)
    before = muscle_amd.get_gemm_mode()
    try:
        muscle_amd.set_gemm_mode(gmode)
        a, b = _execute(case, d)[0], _execute(case, d2)[0]
    finally:
        muscle_amd.set_gemm_mode(before)
    assert bool(torch.isfinite(a.view).all())
    assert _bits_equal(b.view.contiguous(), (a.view * 2.0 ** -8).contiguous())


def test_planes_images_decode_to_the_weights():
    """PlanesPlan over several weights, some without an image: every image is split_planes_kernel's layout as gemm_ref states it,
    h + m + l == w bit for bit with zero rows past N and zero columns past K, and is rebuilt after an in-place update."""
    from muscle_amd import ops
    from muscle_amd._lib import lib
    g = torch.Generator().manual_seed(9)
    shapes = [(130, 48), (64, 40), (1, 16), (200, 64), (129, 96), (7, 12), (128, 32)]
    Ws = [(torch.randn(n, k, generator=g) * 10.0 ** float(torch.randint(-3, 4, (1,), generator=g))).to(DEV) for n, k in shapes]
    Ws.append(torch.randn(64, 50, generator=g).to(DEV)[:, :32])          # not contiguous: no image
    plan = ops.PlanesPlan(Ws)
    for W, im in zip(Ws, plan.images):
        n, k = W.shape
        has = W.is_contiguous() and k % 16 == 0
        assert (im is not None) == has
        assert lib().mx_pw_planes_bytes(n, k) == gr.planes_bytes(n, k) and lib().mx_pw_planes_tiles(n, k) == gr.planes_tiles(n, k)

    def check():
        images = plan.run()
        torch.cuda.synchronize()
        raw = plan.buf.cpu().numpy()
        for W, im in zip(Ws, images):
            if im is None:
                continue
            n, k = W.shape
            off = im - plan.buf.data_ptr()
            img = raw[off:off + gr.planes_bytes(n, k)]
            w = W.cpu().numpy()
            gr.check_planes_image(img, w)
            assert np.array_equal(img, gr.planes_encode(w))
    plan.buf.fill_(0xEE)
    check()
    for W in Ws:
        if W.is_contiguous():
            W.mul_(-1.7).add_(0.01)
    check()


TRANSPOSE_SHAPES = [(1, 1), (31, 33), (32, 32), (200, 36)]


def test_transposes_are_exact():
    """mx_transpose and mx_transpose_batch (a table of matrices with different tile counts) against .t(), bit for bit."""
    from muscle_amd import ops
    g = torch.Generator().manual_seed(3)
    Ws = [torch.randn(r, c, generator=g).to(DEV) for r, c in TRANSPOSE_SHAPES + [(65, 1), (3, 97)]]
    for W in Ws:
        assert _bits_equal(ops.transpose(W), W.t().contiguous())
    plan = ops.TransposePlan(Ws)
    for d in plan.dst:
        d.fill_(float("nan"))
    for W, d in zip(Ws, plan.run()):
        assert _bits_equal(d, W.t().contiguous())


def test_zz_report_time_and_worst_ratios():
    """Prints the module's total time, its slowest case and the worst error-to-limit ratio per kernel family."""
    if not RESULTS:                          # (the cases were deselected: nothing to report)
        return
    total = sum(r[-1] for r in RESULTS)
    slow = max(RESULTS, key=lambda r: r[-1])
    print(f"\nGEMMUNIT total {total:.2f} s over {len(RESULTS)} cases, slowest {slow[0]} {slow[-1]:.2f} s")
    for fam in (1, 2, 3):
        rows = [r for r in RESULTS if _family(r[1]) == fam]
        if rows:
            w = max(rows, key=lambda r: r[5] / r[7])
            print(f"GEMMUNIT family {fam}: {len(rows)} cases, worst err/limit {w[5] / w[7]:.3f} ({w[0]}), worst err/e32 "
                  f"{max(r[5] / max(r[6], 1e-300) for r in rows):.2f}")
    assert math.isfinite(total)
