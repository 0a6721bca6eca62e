"""Host side of the fused stride-2 depthwise backward (no kernel is launched): the header declares mx_dwconv_bwd_fused_s2_parts /
mx_dwconv_bwd_fused_s2 and the library exports them, argument errors come back as MX_EARG before any launch, and the backward schedule
of engine.backbone_backward - run against a recording stand-in for muscle_amd.ops, as profiles/backward_schedule_refactor.txt
describes it - takes the new call once per stride-2 block with engine.DW_S2_FUSED on and makes the calls recorded in
tests/golden/dw_s2_calls_b0.txt (the schedule before the fused kernel existed) with it off."""
import ctypes
import os

import torch

from muscle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "dw_s2_calls_b0.txt")
ENTRIES = ("mx_dwconv_bwd_fused_s2_parts", "mx_dwconv_bwd_fused_s2")
QUERY = "bnbwd_fold_takes("             # how the golden log spells the query the engine made through `ops` when it was recorded


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_dwconv_bwd_fused_s2_parts"] == "iiiii"
    assert sigs["mx_dwconv_bwd_fused_s2"] == "p" * 17 + "i" * 8 + "p"
    if not os.path.exists(_lib.LIB_PATH):
        from muscle_amd import _build
        _build.build(verbose=False)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(L, name), name


def test_bad_arguments_before_any_launch():
    """MX_EARG (-1) with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    ok = dict(dA=p, D=p, gate=p, add=p, a1=p, b1=p, c1=p, c2=p, c3=p, X=p, a0=p, b0=p, W=p, gX=p, dW=p, scratch=p, part=p,
              N=2, H=8, Wd=8, C=8, K=3, pad_lo=0, Ho=4, Wo=4, stream=None)
    bad = [dict(a0=None), dict(a0=None, b0=None), dict(K=4), dict(K=7), dict(C=6), dict(H=0), dict(Wd=0), dict(N=0), dict(X=None),
           dict(part=None), dict(pad_lo=2), dict(K=5, pad_lo=0), dict(Ho=0), dict(Ho=9)]
    for b in bad:
        a = dict(ok, **b)
        assert L.mx_dwconv_bwd_fused_s2(*a.values()) == -1, b
        assert b"dwconv_bwd_fused_s2" in L.mx_last_error(), b
    for args in ((0, 8, 8, 8, 3), (2, 0, 8, 8, 3), (2, 8, 0, 8, 3), (2, 8, 8, 0, 3), (2, 8, 8, 8, 4)):
        assert L.mx_dwconv_bwd_fused_s2_parts(*args) == -1, args


def test_parts_bound():
    """At most 1024 partial rows (the one-launch BatchNorm finalise) for the stride-2 blocks of B7 / the decoder configuration at
    batch 32 and for the 224 px views, never more rows than tiles."""
    L = _lib.lib()
    for N, H, C, K in [(32, 224, 192, 3), (32, 112, 288, 5), (32, 56, 480, 3), (32, 28, 1344, 5),
                       (32, 112, 192, 3), (32, 56, 288, 5), (32, 28, 480, 3), (32, 14, 1344, 5), (1, 1, 4, 5), (2, 2, 8, 3)]:
        p = L.mx_dwconv_bwd_fused_s2_parts(N, H, H, C, K)
        assert 1 <= p <= min(1024, N * ((H + 7) // 8) * ((H + 31) // 32)), (N, H, C, K, p)


# ---- the backward schedule against a recording stand-in for muscle_amd.ops ------------------------------------------------------
def _describe(v):
    if isinstance(v, torch.Tensor):
        return "T" + str(list(v.shape))
    if isinstance(v, tuple) and hasattr(v, "_fields"):
        return type(v).__name__
    if isinstance(v, torch.nn.Module):
        return type(v).__name__
    if callable(v):
        return "<callable>"
    return repr(v)


class RecordingOps:
    """Every ops.* call logged with the shapes of its tensor arguments and its keyword arguments; results are empty CPU tensors of
    the shapes the real calls return.  It knows neither fused pointwise backward; the small fold takes a shape from 512 rows."""
    PLAIN, BNACT, AFFINE = 0, 1, 2

    def __init__(self):
        from muscle_amd.ops import BNState
        self.BNState = BNState
        self.calls = []

    def __getattr__(self, name):
        if name.startswith("_"):
            raise AttributeError(name)
        result = getattr(self, "_r_" + name)

        def fn(*args, **kw):
            line = name + "(" + ", ".join(_describe(a) for a in args) + ")"
            if kw:
                line += " " + ", ".join(f"{k}={_describe(v)}" for k, v in sorted(kw.items()))
            self.calls.append(line)
            return result(*args, **kw)
        return fn

    @staticmethod
    def _e(*shape):
        return torch.empty(*shape, dtype=torch.float32)

    def _r_bn_backward(self, G, X, *a, out=None, **kw):
        return out if out is not None else torch.empty_like(X)

    def _r_pw_wgrad(self, *a, **kw):
        return None

    _r_pw_wgrad_bnbwd = _r_dw_parts_reduce = _r_dwconv_bwd_weight = _r_pw_wgrad

    def _r_pw_dgrad(self, G, W, n_out, **kw):
        return self._e(G.shape[0], n_out)

    def _r_pw_dgrad_bnbwd_planes(self, G, G2, c, planes, n_out, **kw):
        return self._e(G.shape[0], n_out)

    def _r_se_bn1_pool(self, dA, X, st, hw):
        return self._e(5, X.shape[0] // hw, X.shape[1])

    def _r_se_bwd(self, pooled, gate, s, h, *a):
        return torch.empty_like(h)

    def _r_bn1_coeffs(self, pooled5, gate, *a):
        return self._e(3, gate.shape[1]), torch.empty_like(gate)

    def _r_dwconv_bwd_fused(self, dA, D, gate, add, st1, c1, X, st0, W, dW, K, pad_lo, *, residual=None, defer=None):
        if defer is not None:
            defer(self._e(4, W.numel()), dW)
        return torch.empty_like(X), (self._e(4, 2, X.shape[3]) if st0 is not None else None)

    def _r_dwconv_bwd_fused_s2(self, dA, D, gate, add, st1, c1, X, st0, W, dW, K, pad_lo, *, defer=None):
        if defer is not None:
            defer(self._e(4, W.numel()), dW)
        return torch.empty_like(X), self._e(4, 2, X.shape[3])

    def _r_bn_backward_from_coeffs(self, G, X, st, c, *, out, **kw):
        return out

    def _r_dwconv_bwd_data(self, dY, W, K, S, pad_lo, H, Wd, **kw):
        return self._e(dY.shape[0], H, Wd, dY.shape[3])

    def _r_bn_bwd_coeffs(self, part, *a):
        return self._e(3, part.shape[2])

    def _r_bn_bwd_apply_plain(self, G, X, c, out):
        return out

    # the queries engine.block_route makes: ordinary methods, not logged
    def pw_proj_bwd_fused_takes(self, R, Cout, Cexp, rows_per_sample):
        return False

    def pw_bwd_fused_takes(self, M, K, N):
        return False

    def bnbwd_fold_small_takes(self, M, K, N):
        return M >= 512


def _b0_tape(N=2, S=32):
    """Backbone, config and a hand-made tape of efficientnet-b0 (last_pooling off: 3 stride-2 blocks) with an S x S stem output:
    every tensor the backward reads exists with its real shape, on the CPU, uninitialised."""
    from muscle_amd import engine
    from muscle_amd.arch import net_cfg
    from muscle_amd.efficientnet import EfficientNet
    from muscle_amd.ops import BNState
    cfg = net_cfg("efficientnet-b0", False)
    backbone = EfficientNet(cfg)
    e = lambda *s: torch.empty(*s, dtype=torch.float32)
    st = lambda C: BNState(e(C), e(C), e(C), e(C))
    tape = engine.Tape(training=True, N=N)
    tape.H0 = tape.W0 = S
    tape.cols = e(N * S * S, 28)
    tape.stem_raw, tape.stem_bn = e(N, S, S, cfg.stem_out), st(cfg.stem_out)
    x, x_st, h = tape.stem_raw, tape.stem_bn, S
    expands = 0
    for b in cfg.blocks:
        ho = b.out_size(h)
        t = engine.BlockTape(cfg=b, H=h, W=h, Ho=ho, Wo=ho, x=x, x_st=x_st)
        m = backbone._blocks[b.index]
        if b.expand:
            t.e_raw, t.bn0 = e(N, h, h, b.cexp), st(b.cexp)
            if expands % 3 != 2:                        # pre-split W^T images for two expand convs in three
                tape.wtp[id(m._expand_conv.weight)] = 1
            expands += 1
        t.d_raw, t.bn1 = e(N, ho, ho, b.cexp), st(b.cexp)
        t.s, t.h, t.gate = e(N, b.cexp), e(N, b.se), e(N, b.cexp)
        if engine.project_materialises(b, N * ho * ho, True):
            t.a = e(N * ho * ho, b.cexp)
        t.p_raw, t.bn2 = e(N * ho * ho, b.cout), st(b.cout)
        t.out = e(N, ho, ho, b.cout)
        tape.blocks.append(t)
        x, x_st, h = t.out, None, ho
    taps = {i: torch.empty_like(tape.blocks[i].out) for i in cfg.taps}
    return backbone, cfg, tape, taps


def _routes(tape, backbone):
    """engine.block_route of every block of a fresh tape, asked as backbone_backward asks it (under the switches and the `engine.ops`
    in force)."""
    from muscle_amd import engine
    return [engine.block_route(t.cfg, tape.N, t.H, t.W, t.Ho, t.Wo, materialised=t.a is not None,
                               wt_planes=t.cfg.expand and id(backbone._blocks[t.cfg.index]._expand_conv.weight) in tape.wtp)
            for t in tape.blocks]


def _golden_calls():
    """(the kernel calls of tests/golden/dw_s2_calls_b0.txt, the arguments of its query lines).  The file was recorded when the engine
    asked `ops.bnbwd_fold_takes(M, K, N)` through the call log; queries are no longer `ops` calls the stand-in logs, so those eight
    lines are dropped before comparing - every other line, and its position among the others, must match exactly."""
    lines = open(GOLDEN).read().splitlines()
    asked = [tuple(int(v) for v in c[len(QUERY):-1].split(", ")) for c in lines if c.startswith(QUERY)]
    assert len(asked) == 8
    return [c for c in lines if not c.startswith(QUERY)], asked


def _record(monkeypatch, fused: bool):
    from muscle_amd import engine
    rec = RecordingOps()
    monkeypatch.setattr(engine, "ops", rec)
    monkeypatch.setattr(engine, "WGRAD_SIDE_STREAM", False)
    monkeypatch.setattr(engine, "DW_S2_FUSED", fused)
    backbone, cfg, tape, taps = _b0_tape()
    routes = _routes(tape, backbone)
    engine.backbone_backward(backbone, cfg, tape, taps, engine.GradSink())
    return rec.calls, cfg, tape, backbone, routes


def _want_expand(t, tape, backbone, dw_s2: bool):
    """BlockRoute.expand of the base stand-in (no fused expand backward, the small fold from 512 rows) with the default switches."""
    b, M = t.cfg, tape.N * t.H * t.W
    if not b.expand and b.index != 0:
        return "none"
    if b.stride == 2 and not dw_s2:
        return "plain"
    image = b.expand and id(backbone._blocks[b.index]._expand_conv.weight) in tape.wtp
    return "fold" if b.stride == 1 and image and M >= 512 else "apply"


def test_stride2_blocks_take_the_fused_call(monkeypatch):
    calls, cfg, tape, backbone, routes = _record(monkeypatch, True)
    s2 = [b for b in cfg.blocks if b.stride == 2]
    assert len(s2) == 3 and all(b.expand for b in s2)
    assert [r.depthwise for r in routes] == ["fused_s2" if b.stride == 2 else "fused" for b in cfg.blocks]
    assert [r.expand for r in routes] == [_want_expand(t, tape, backbone, True) for t in tape.blocks]
    assert {r.project for r in routes} == {"gemm"}
    names = [c.split("(")[0] for c in calls]
    assert names.count("dwconv_bwd_fused_s2") == 3
    got = sorted(c for c in calls if c.startswith("dwconv_bwd_fused_s2("))
    want = sorted(f"dwconv_bwd_fused_s2(T[2, {h // 2}, {h // 2}, {b.cexp}], T[2, {h // 2}, {h // 2}, {b.cexp}], T[2, {b.cexp}], T[2, {b.cexp}], "
                  f"BNState, T[3, {b.cexp}], T[2, {h}, {h}, {b.cexp}], BNState, T[{b.cexp}, 1, {b.kernel}, {b.kernel}], "
                  f"T[{b.cexp}, 1, {b.kernel}, {b.kernel}], {b.kernel}, {b.pad_lo}) defer=<callable>"
                  for b, h in zip(s2, (32, 16, 8)))
    assert got == want
    for gone in ("bn_backward_from_coeffs", "dwconv_bwd_weight", "dwconv_bwd_data"):
        assert gone not in names, gone
    assert not [c for c in calls if c.startswith("bn_backward(") and "act=BNState" in c]      # the BN0 reduction with swish' recomputed
    assert names.count("dwconv_bwd_fused") == len(cfg.blocks) - 3 and names.count("bn_bwd_coeffs") == len(cfg.blocks)
    assert names.count("dw_parts_reduce") == len(cfg.blocks)                                    # every weight gradient's rows are added


def test_flag_off_restores_the_previous_schedule(monkeypatch):
    """The call log with engine.DW_S2_FUSED off is tests/golden/dw_s2_calls_b0.txt, which stays as it was recorded: its eight
    `bnbwd_fold_takes(` lines are dropped before the comparison (_golden_calls), every other line and its position must match.  What
    those eight lines said is asserted on the routes instead: the blocks the engine asked about, in the order it asked, are the
    stride-1 expand blocks with an image of W^T - exactly the blocks that can take the fold - and each route is the answer's."""
    calls, cfg, tape, backbone, routes = _record(monkeypatch, False)
    want, asked = _golden_calls()
    assert calls == want
    assert [r.depthwise for r in routes] == ["unfused" if b.stride == 2 else "fused" for b in cfg.blocks]
    assert [r.expand for r in routes] == [_want_expand(t, tape, backbone, False) for t in tape.blocks]
    assert {r.project for r in routes} == {"gemm"}
    could_fold = [(tape.N * t.H * t.W, t.cfg.cexp, t.cfg.cin) for t, r in zip(tape.blocks, routes)
                  if t.cfg.expand and r.expand in ("fold", "apply") and id(backbone._blocks[t.cfg.index]._expand_conv.weight) in tape.wtp]
    assert could_fold[::-1] == asked                                                            # (the backward walks the blocks in reverse)
    assert [r.expand for r in routes].count("fold") == sum(M >= 512 for M, _, _ in asked) == 1
    names = [c.split("(")[0] for c in calls]
    assert "dwconv_bwd_fused_s2" not in names
    for back in ("bn_backward_from_coeffs", "dwconv_bwd_weight", "dwconv_bwd_data"):
        assert names.count(back) == 3, back
    assert len([c for c in calls if c.startswith("bn_backward(") and "act=BNState" in c]) == 3

