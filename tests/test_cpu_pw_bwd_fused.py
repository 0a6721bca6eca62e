"""Host side of the fused expand-conv backward (no kernel is launched): the header declares the entry points and the library exports
them, argument errors come back as MX_EARG before any launch, the planner queries answer for the two shapes only, and the backward
schedule of engine.backbone_backward - run against a recording stand-in for muscle_amd.ops whose pw_bwd_fused_takes answers yes -
issues exactly one pw_bwd_fused per eligible block of either stride and nothing else for that conv, as engine.block_route says for
those blocks; with engine.PW_BWD_FUSED off the call log is the one recorded before the kernel existed."""
import ctypes

import torch

from muscle_amd import _lib
from test_cpu_dwfused_s2 import RecordingOps, _b0_tape, _golden_calls, _routes


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_pw_bwd_small_fused_ok"] == "iii" and sigs["mx_pw_bwd_small_fused_groups"] == "iii"
    assert sigs["mx_pw_bwd_small_fused"] == "p" * 8 + "i" * 6 + "plp"
    assert sigs["mx_pw_parts_reduce"] == "piipp"
    L = _lib.lib()
    for name in ("mx_pw_bwd_small_fused_ok", "mx_pw_bwd_small_fused_groups", "mx_pw_bwd_small_fused", "mx_pw_parts_reduce"):
        assert hasattr(L, name), name


def test_planner_queries():
    L = _lib.lib()
    for Co, Ci in ((288, 48), (192, 32)):
        assert L.mx_pw_bwd_small_fused_ok(65536, Co, Ci) == 1 and L.mx_pw_bwd_small_fused_ok(1605632, Co, Ci) == 1
        assert L.mx_pw_bwd_small_fused_ok(65535, Co, Ci) == 0                   # the row threshold of the small-output kernels
        for R in (1, 21, 64, 199, 4133, 65536, 100352, 131071, 131072, 401408, 1605632):
            groups = L.mx_pw_bwd_small_fused_groups(R, Co, Ci)
            assert 1 <= groups <= max(512, (R + 63) // 64), (R, groups)
            ws = L.mx_pw_wgrad_small_ws(R, Co, Ci, 0)
            assert ws == 0 or groups * Co * Ci * 4 <= ws, (R, groups, ws)         # the existing scratch query covers it
        assert L.mx_pw_bwd_small_fused_groups(401408, Co, Ci) == 512             # one round of two workgroups per CU
    for R, Co, Ci in ((401408, 480, 80), (401408, 48, 288), (401408, 288, 32), (401408, 192, 48), (100352, 32, 32), (0, 288, 48)):
        assert L.mx_pw_bwd_small_fused_ok(R, Co, Ci) == 0 and L.mx_pw_bwd_small_fused_groups(R, Co, Ci) == 0, (R, Co, Ci)


def test_bad_arguments_before_any_launch():
    """MX_EARG (-1) with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    ok = dict(G=p, G2=p, coef=p, X=p, W=p, dW=p, dX=p, residual=p, R=100, Co=288, Ci=48, ldg=288, ldx=48, lddx=48, ws=p,
              ws_bytes=1 << 30, stream=None)
    bad = [dict(Co=480, Ci=80), dict(Co=48, Ci=288), dict(Co=288, Ci=32), dict(Co=192, Ci=48), dict(Co=32, Ci=32), dict(R=0), dict(R=-5),
           dict(ldg=290), dict(ldx=50), dict(lddx=49), dict(ldg=284), dict(ldx=44), dict(lddx=32), dict(G=None), dict(X=None),
           dict(W=None), dict(dX=None), dict(ws=None), dict(G2=None), dict(coef=None), dict(G=p + 4), dict(dX=p + 8), dict(residual=p + 4),
           dict(W=p + 4), dict(ws_bytes=1024), dict(Co=192, Ci=32, ldg=190)]
    for b in bad:
        a = dict(ok, **b)
        assert L.mx_pw_bwd_small_fused(*a.values()) == -1, b
        assert b"pw_bwd_small_fused" in L.mx_last_error(), b
    for args in ((None, 4, 16, p), (p, 0, 16, p), (p, 4, 0, p), (p, 4, 18, p), (p, 4, 16, None), (p + 4, 4, 16, p)):
        assert L.mx_pw_parts_reduce(args[0], args[1], args[2], args[3], None) == -1, args
        assert b"pw_parts_reduce" in L.mx_last_error(), args


# ---- the backward schedule against a recording stand-in whose pw_bwd_fused_takes answers yes ----------------------------------------
class FusedRecordingOps(RecordingOps):
    """RecordingOps whose fused expand-conv backward takes a shape from 512 rows - the rows from which the parent's small fold takes it
    too, so that every block the fused kernel takes is one the fold would take with the switch off."""

    def pw_bwd_fused_takes(self, M, K, N):
        return M >= 512

    def _r_pw_bwd_fused(self, G, G2, coef, X, W, dW, *, residual=None, defer=None):
        if defer is not None:
            defer(self._e(4, W.numel()), dW)
        return self._e(G.shape[0], X.shape[1])

    def _r_pw_parts_reduce(self, part, dW):
        return None


def _record(monkeypatch, rec, *, pw_fused: bool, dw_s2: bool = True):
    from muscle_amd import engine
    monkeypatch.setattr(engine, "ops", rec)
    monkeypatch.setattr(engine, "WGRAD_SIDE_STREAM", False)
    monkeypatch.setattr(engine, "DW_S2_FUSED", dw_s2)
    monkeypatch.setattr(engine, "PW_BWD_FUSED", pw_fused)
    backbone, cfg, tape, taps = _b0_tape()
    routes = _routes(tape, backbone)
    engine.backbone_backward(backbone, cfg, tape, taps, engine.GradSink())
    return rec.calls, cfg, tape, backbone, routes


def _eligible(cfg, tape, backbone):
    """(block, M) of the expand blocks the stand-in's fused kernel takes: part0 is there (every expand block with the stride-2 depthwise
    backward fused), 512 rows or more, and - stride 1 only, as before - a pre-split image of W^T."""
    out = []
    for t in tape.blocks:
        b = t.cfg
        M = tape.N * t.H * t.W
        if b.expand and M >= 512 and (b.stride == 2 or id(backbone._blocks[b.index]._expand_conv.weight) in tape.wtp):
            out.append((b, M))
    return out


def test_eligible_blocks_take_exactly_one_fused_call(monkeypatch):
    calls, cfg, tape, backbone, routes = _record(monkeypatch, FusedRecordingOps(), pw_fused=True)
    blocks = _eligible(cfg, tape, backbone)
    assert {b.stride for b, _ in blocks} == {1, 2} and any(b.skip for b, _ in blocks) and not all(b.skip for b, _ in blocks)
    # the route: "fused" for exactly those blocks, and the small fold - which takes the same rows - never ranks above it
    took = {b.index for b, _ in blocks}
    assert [r.expand for r in routes] == ["fused" if b.index in took else "apply" if b.expand or b.index == 0 else "none" for b in cfg.blocks]
    fused = [c for c in calls if c.startswith("pw_bwd_fused(")]
    assert len(fused) == len(blocks)
    for b, M in blocks:
        kw = "defer=<callable>, residual=" + (f"T[{M}, {b.cin}]" if b.skip else "None")      # the identity branch's gradient: skip blocks only
        want = (f"pw_bwd_fused(T[{M}, {b.cexp}], T[{M}, {b.cexp}], T[3, {b.cexp}], T[{M}, {b.cin}], T[{b.cexp}, {b.cin}], "
                f"T[{b.cexp}, {b.cin}]) {kw}")
        assert fused.count(want) == 1, want
        # nothing else for that conv: its dZ-wide operand [M, Cexp] opens no apply pass, data gradient or weight gradient
        for gone in ("bn_bwd_apply_plain", "pw_dgrad", "pw_dgrad_bnbwd_planes", "pw_wgrad", "pw_wgrad_bnbwd"):
            assert not [c for c in calls if c.startswith(f"{gone}(T[{M}, {b.cexp}], ")], (gone, b.index)
    names = [c.split("(")[0] for c in calls]
    assert names.count("pw_parts_reduce") == len(blocks)                          # every partial-matrix sum is added, through the lane
    assert not [n for n in names if n.endswith("_takes")]                         # the queries are not `ops` calls in the log
    # the other expand convs keep their calls
    others = [t for t in tape.blocks if t.cfg.expand and t.cfg.index not in took]
    assert others and names.count("pw_dgrad") + names.count("pw_dgrad_bnbwd_planes") == len(tape.blocks) + len(others)


def test_switch_off_restores_todays_log(monkeypatch):
    """With engine.PW_BWD_FUSED off the stand-in whose fused kernel takes a shape gives the call log - and the routes - of the one that
    knows only the small fold, and, with the stride-2 depthwise fusion off as well, the golden log recorded before either kernel
    existed (less its query lines: test_cpu_dwfused_s2._golden_calls)."""
    off, cfg, tape, backbone, r_off = _record(monkeypatch, FusedRecordingOps(), pw_fused=False)
    today, *_, r_today = _record(monkeypatch, RecordingOps(), pw_fused=False)
    assert off == today and not [c for c in off if c.startswith("pw_bwd_fused(") or c.startswith("pw_parts_reduce(")]
    assert r_off == r_today and "fused" not in {r.expand for r in r_off}
    # the stride-1 blocks the fused kernel took go back to the fold; the stride-2 ones, which never fold, to the plain apply
    for (b, _) in _eligible(cfg, tape, backbone):
        assert r_off[b.index].expand == ("fold" if b.stride == 1 else "apply"), b.index
    off2, *_, r_off2 = _record(monkeypatch, FusedRecordingOps(), pw_fused=False, dw_s2=False)
    assert off2 == _golden_calls()[0]
    # and the stand-in that knows no fused kernel is untouched by the switch
    on, *_, r_on = _record(monkeypatch, RecordingOps(), pw_fused=True, dw_s2=False)
    assert on == off2 and r_on == r_off2

