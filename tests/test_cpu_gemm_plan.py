"""The launch planner of the forward / data-gradient GEMMs seen through mx_pw_fwd_plan, without a GPU: the case table of
test_gpu_gemm_nt_units.py covers exactly the compiled instantiations of gemm_nt_kernel / gemm_nt_split_kernel / gemm_nt_split3_kernel
(read from the host stubs of the built library), every case's answer is still what the table stores, the argument contracts are
refused with MX_EARG and a message before any launch, and the restatements of tests/gemm_ref.py agree with themselves."""
import re

import numpy as np
import pytest
import torch

import gemm_ref as gr
import test_gpu_gemm_nt_units as units
from muscle_amd import _build, _lib

EARG = -1
P = 0x10000                 # a 16-byte aligned "pointer": every call below is refused before anything could read it


@pytest.fixture
def L():
    lib = _lib.lib()
    mode = lib.mx_get_gemm_mode()
    yield lib
    lib.mx_set_gemm_mode(mode)


def _compiled():
    """{(family, tile width, prologue)} of the built library"""
    blob = open(_build.LIB, "rb").read()
    got = set()
    for wm, wn, tm, tn, am in re.findall(rb"__device_stub__gemm_nt_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", blob):
        assert int(wm) * int(tm) * 16 == 128
        got.add((1, int(wn) * int(tn) * 16, int(am)))
    for am, nj in re.findall(rb"__device_stub__gemm_nt_split_kernelILi(\d+)ELi(\d+)EE", blob):
        got.add((2, 64 * int(nj), int(am)))
    for tn, am in re.findall(rb"__device_stub__gemm_nt_split3_kernelILi(\d+)ELi(\d+)EE", blob):
        got.add((3, 16 * int(tn), int(am)))
    return got


def test_the_compiled_instantiations_are_the_documented_40():
    got = _compiled()
    want = {(1, w, a) for w in (32, 48, 64, 80, 96, 128, 160) for a in (gr.PLAIN, gr.BNACT, gr.AFFINE)}
    want |= {(2, w, a) for w in (64, 128) for a in (gr.PLAIN, gr.BNACT, gr.AFFINE)}
    want |= {(3, w, a) for w in (64, 80, 96, 112, 128) for a in (gr.PLAIN, gr.BNBWD)} | {(3, w, gr.BNACT) for w in (64, 80, 96)}
    assert got == want, sorted(got ^ want)


def test_case_table_covers_exactly_the_compiled_instantiations(L):
    compiled = _compiled()
    covered, forms = set(), set()
    for cid, route, a_mode, gmode, M, K, N, batch, opts, rps, plan in units.CASES:
        L.mx_set_gemm_mode(gmode)
        got = L.mx_pw_fwd_plan(units.ENTRY[route], a_mode, M, K, N, batch)
        assert got == plan, (cid, got, plan)
        inst = (plan // 10000, plan // 10 % 1000, a_mode)
        assert inst in compiled, (cid, inst)                  # the answer names a kernel that exists
        covered.add(inst)
        forms.add((plan // 10000, plan % 10, (M + 127) // 128 % 8 != 0))
    assert covered == compiled, sorted(covered ^ compiled)    # an instantiation without a case, or no argument reaches it
    # every grid form of every family; the 1-D forms with a row-tile count that is no multiple of 8 (early-return tiles)
    assert {(1, 0), (2, 0), (3, 0)} <= {(f, g) for f, g, _ in forms}
    assert {(1, 1, True), (2, 1, True), (3, 1, True), (3, 2, True)} <= forms
    ids = [c[0] for c in units.CASES]
    assert len(set(ids)) == len(ids)


def test_case_table_covers_the_listed_paths():
    C = units.CASES
    fwd = [c for c in C if c[1] in ("fwd", "planes")]
    for fam in (1, 2, 3):
        opts = {c[8] for c in fwd if c[10] // 10000 == fam}
        assert any("stats" in o for o in opts) and any("res" in o for o in opts), (fam, opts)
        assert any("bias" in o and "res" in o and "relu" in o for o in opts), (fam, opts)      # forces the non-lean epilogue
    for fam in (1, 2, 3):
        rps = {(c[9], c[4]) for c in C if c[2] == gr.BNACT and c[10] // 10000 == fam}
        assert any(r == 49 for r, _ in rps) and any(r > m for r, m in rps), (fam, rps)
    rps1 = {c[9] for c in C if c[2] == gr.BNACT}
    assert {1, 49, 50} <= rps1                                              # 50: no divisor of 128, and the last sample is short
    assert {4, 8, 12} <= {c[5] % 16 for c in C if c[10] // 10000 == 1}       # K tails of gemm_nt_kernel
    assert any(c[5] % 32 == 16 for c in C if c[1] == "planes")              # the half K step of the planes kernel
    assert any(c[6] % 4 for c in C if c[10] // 10000 == 1) and any(c[6] % 4 for c in C if c[10] // 10000 == 2) and any(c[6] % 4 for c in C if c[10] // 10000 == 3)
    assert {c[10] // 10000 for c in C if c[1] == "bgemm" and c[7] == 3} == {1, 2}
    widths = [(c[6] + c[10] // 10 % 1000 - 1) // (c[10] // 10 % 1000) for c in C if c[1] == "bnbwd_planes"]
    assert 1 in widths and max(widths) > 1                                  # one N tile, and several
    # M is ragged everywhere: tile edge minus 5
    assert all(c[4] % 128 == 123 for c in C)


def test_plan_query_refuses_what_the_entries_refuse(L):
    ok = L.mx_pw_fwd_plan(0, 0, 128, 16, 32, 1)
    assert ok == 10320
    for args, word in [((2, 0, 128, 16, 32, 1), b"entry"), ((0, 4, 128, 16, 32, 1), b"a_mode"), ((0, 3, 251, 64, 130, 1), b"a_mode"),
                       ((0, 0, 0, 16, 32, 1), b"extents"),
                       ((0, 0, 128, 16, 32, 0), b"extents"), ((0, 0, 128, 18, 32, 1), b"multiple of 4"),
                       ((1, 0, 128, 24, 32, 1), b"multiple of 16"), ((1, 1, 128, 48, 32, 1), b"multiple of 32"),
                       ((1, 3, 128, 16, 32, 1), b"multiple of 32"), ((1, 2, 128, 32, 32, 1), b"affine"), ((1, 0, 128, 32, 32, 2), b"batched")]:
        assert L.mx_pw_fwd_plan(*args) == EARG, args
        assert word in L.mx_last_error(), (args, L.mx_last_error())
    # the modes change the family on the mx_pw_fwd route (which has no BNBWD form: refused above), never on the planes route
    for mode, fam in ((0, 1), (2, 2)):
        L.mx_set_gemm_mode(mode)
        assert L.mx_pw_fwd_plan(0, 0, 251, 64, 130, 1) // 10000 == fam
        assert L.mx_pw_fwd_plan(1, 0, 251, 64, 130, 1) // 10000 == 3
    # the activated planes form exists up to 96 columns
    assert L.mx_pw_fwd_plan(1, 0, 65531, 32, 128, 1) // 10 % 1000 == 128
    assert L.mx_pw_fwd_plan(1, 1, 65531, 32, 128, 1) // 10 % 1000 == 64
    assert L.mx_pw_fwd_plan(1, 1, 65531, 32, 192, 1) // 10 % 1000 == 96


def test_argument_contracts_are_refused_before_any_launch(L):
    """Every call passes made-up addresses: a contract that was not refused would have to launch to be noticed, so each one is held
    to MX_EARG and its message."""
    M, K, N = 64, 32, 32

    def fwd(A=P, W=P, C=P, K=K, lda=None, ldc=N, a_mode=0, res=None, N=N):
        return L.mx_pw_fwd(A, a_mode, None, None, None, 1, W, C, M, K, N, K if lda is None else lda, ldc, None, res, 0, None, None)

    def refused(rc, word):
        assert rc == EARG
        assert word in L.mx_last_error(), L.mx_last_error()

    refused(L.mx_bgemm(0, P, P, P, M, N, 30, 32, 32, N, 0, 0, 0, 1, 0, None), b"K=30 must be a multiple of 4")      # K % 4
    refused(fwd(lda=34), b"leading dims")                                   # lda % 4
    refused(L.mx_bgemm(0, P, P, P, M, N, K, K, K + 2, N, 0, 0, 0, 1, 0, None), b"leading dims")            # ldb % 4
    refused(fwd(A=P + 4), b"operand A not 16-byte aligned")
    refused(fwd(W=P + 8), b"operand B not 16-byte aligned")
    refused(fwd(a_mode=3), b"operand A bad mode 3")                         # the BNBWD prologue exists on the planes route only
    # (NT with a prologue on B is refused by gemm_common too, but no entry point of the ABI can pass one: mx_pw_fwd and mx_bgemm
    # both build a plain B)
    # C / residual: nt_epilogue and the first split kernel store C and load the residual 16 bytes at a time whenever ldc and N are
    # multiples of 4, so both must be 16-byte aligned then (and need not be otherwise: the scalar path)
    refused(fwd(C=P + 4), b"C and residual must be 16-byte aligned")
    refused(fwd(res=P + 8), b"C and residual must be 16-byte aligned")
    refused(L.mx_bgemm(0, P, P, P, M, N, K, K, K, N, 0, 0, M * N + 2, 2, 0, None), b"C and residual must be 16-byte aligned")
    refused(L.mx_bgemm(0, P, P, P, M, N, K, K, K, N, M * K + 1, 0, 0, 2, 0, None), b"batch strides")
    # the planes entries
    refused(L.mx_pw_fwd_planes(P, P, P, M, K, N, K - 4, N, None, None, 0, None, None), b"leading dimensions")         # lda < K
    refused(L.mx_pw_fwd_planes(P, P, P, M, K, N, K, N - 1, None, None, 0, None, None), b"leading dimensions")         # ldc < N
    refused(L.mx_pw_fwd_planes(P + 4, P, P, M, K, N, K, N, None, None, 0, None, None), b"16-byte aligned")
    refused(L.mx_pw_fwd_planes(P, P + 8, P, M, K, N, K, N, None, None, 0, None, None), b"16-byte aligned")
    refused(L.mx_pw_fwd_planes(P, P, P, M, K, N, K, N, None, P + 4, 0, None, None), b"16-byte aligned")
    refused(L.mx_pw_fwd_planes(P, P, P, M, 24, N, 24, N, None, None, 0, None, None), b"multiple of 16")               # K % 16
    refused(L.mx_pw_fwd_planes_act(P, P, P, P, 1, P, P, M, 48, N, 48, N, None, None), b"bad extents")                 # K % 32
    refused(L.mx_pw_fwd_planes_act(P, P, P, P, 1, P, P, M, K, N, K - 4, N, None, None), b"leading dimensions")
    refused(L.mx_pw_fwd_planes_act(P, P, P, P, 1, P, P, M, K, N, K, N - 4, None, None), b"leading dimensions")
    refused(L.mx_pw_dgrad_bnbwd_planes(P, P, P, P, P, M, 48, N, 48, N, None, None), b"multiple of 32")
    refused(L.mx_pw_dgrad_bnbwd_planes(P, P, P, P, P, M, K, N, K - 4, N, None, None), b"leading dimensions")
    refused(L.mx_pw_dgrad_bnbwd_planes(P, P, P, P, P, M, K, N, K, N - 4, None, None), b"leading dimensions")
    refused(L.mx_pw_dgrad_bnbwd_planes(P, P, P, P, P, M, K, N, K, N, P + 4, None), b"16-byte aligned")


def test_planes_layout_restated_round_trips():
    g = np.random.default_rng(1)
    for n, k in [(1, 16), (130, 48), (64, 32), (200, 64)]:
        w = (g.standard_normal((n, k)) * 10.0 ** g.integers(-3, 4)).astype(np.float32)
        img = gr.planes_encode(w)
        assert img.size == gr.planes_bytes(n, k)
        gr.check_planes_image(img, w)
        t = gr.planes_decode(img, n, k)
        assert not (t.view(np.uint32) & 0xFFFF).any()                       # three bf16 terms
        bad = img.copy()
        bad[5] ^= 0x10                                                      # one flipped bit of one term is noticed
        with pytest.raises(AssertionError):
            gr.check_planes_image(bad, w)
    assert gr.planes_bytes(8, 24) == -1 and gr.planes_tiles(130, 48) == 4 * 2


def test_reference_pieces():
    g = torch.Generator().manual_seed(0)
    A = torch.randn(40, 36, generator=g)
    # prologues against their formulas on one element
    sc, sh = torch.rand(36, generator=g) + 0.5, torch.randn(36, generator=g)
    gate = torch.rand(3, 36, generator=g)
    v = sc[5].double() * A[17, 5].double() + sh[5].double()
    assert gr.prologue(gr.AFFINE, A, scale=sc, shift=sh)[17, 5] == v
    want = v / (1 + torch.exp(-v)) * gate[17 // 15, 5].double()
    assert abs(float(gr.prologue(gr.BNACT, A, scale=sc, shift=sh, gate=gate, rps=15)[17, 5] - want)) <= 1e-15 * abs(float(want)) + 1e-300
    coef = torch.randn(3, 36, generator=g)
    X = torch.randn(40, 36, generator=g)
    assert gr.prologue(gr.BNBWD, A, X=X, coef=coef)[3, 7] == coef[0, 7].double() * A[3, 7].double() + coef[1, 7].double() * X[3, 7].double() + coef[2, 7].double()
    C = torch.randn(130, 5, generator=g)
    s, q, a = gr.tile_stats(C)
    assert s.shape == (2, 5) and torch.allclose(s[1], C[128:].double().sum(0)) and torch.allclose(q[0], (C[:128].double() ** 2).sum(0))
    assert torch.equal(gr.epilogue(torch.tensor([[-1.0, 2.0]]), torch.tensor([0.5, 0.5]), torch.tensor([[0.25, 0.25]]), True), torch.tensor([[0.0, 2.75]]))
