"""Host side of the fused project-conv backward (no kernel is launched): the header declares the three entry points and the library
exports them, the planner queries answer for the admitted shapes and thresholds only, argument errors come back as MX_EARG before any
launch, and the backward schedule of engine.backbone_backward - run against a recording stand-in for muscle_amd.ops that answers
"takes" - issues exactly one pw_proj_bwd_fused per eligible block, no pw_dgrad / pw_wgrad / se_bn1_pool for that conv and one parts
reduce through the lane; with engine.PW_PROJ_BWD_FUSED off the call log is the parent's."""
import ctypes

from muscle_amd import _lib
from test_cpu_dwfused_s2 import RecordingOps, _b0_tape, _routes

ADMITTED = ((48, 288), (48, 192))


def test_header_declares_and_library_exports():
    sigs = _lib.parse_header()
    assert sigs["mx_pw_proj_bwd_fused_ok"] == "iiii" and sigs["mx_pw_proj_bwd_fused_groups"] == "iiii"
    assert sigs["mx_pw_proj_bwd_fused"] == "p" * 5 + "i" + "p" * 4 + "i" * 6 + "plp"
    L = _lib.lib()
    for name in ("mx_pw_proj_bwd_fused_ok", "mx_pw_proj_bwd_fused_groups", "mx_pw_proj_bwd_fused"):
        assert hasattr(L, name), name


def test_planner_queries():
    L = _lib.lib()
    for Co, Ce in ADMITTED:
        assert L.mx_pw_proj_bwd_fused_ok(65536, Co, Ce, 16384) == 1 and L.mx_pw_proj_bwd_fused_ok(401408, Co, Ce, 12544) == 1
        assert L.mx_pw_proj_bwd_fused_ok(65520, Co, Ce, 16) == 0                  # the row threshold of the small-output kernels
        for R, rps in ((16, 16), (64, 16), (192, 48), (4144, 592), (65600, 16400), (131072, 16384), (401408, 12544), (1605632, 50176)):
            groups = L.mx_pw_proj_bwd_fused_groups(R, Co, Ce, rps)
            assert 1 <= groups <= max(512, (R + 63) // 64), (R, groups)
        assert L.mx_pw_proj_bwd_fused_groups(401408, Co, Ce, 12544) == 512        # one round of two workgroups per CU
        assert L.mx_pw_proj_bwd_fused_groups(1605632, Co, Ce, 50176) == 512
        # below 131 072 rows: the row groups of the small-output weight-gradient kernel (their partial matrices are the same)
        assert L.mx_pw_proj_bwd_fused_groups(65600, Co, Ce, 16400) * Co * Ce * 4 == L.mx_pw_wgrad_small_ws(65600, Co, Ce, 1)
        # rows_per_sample: a multiple of 16 that divides R, nothing else
        for R, rps in ((401408, 0), (401408, -16), (401408, 12543), (401408, 8), (401408, 401409), (401400, 12544), (0, 16)):
            assert L.mx_pw_proj_bwd_fused_ok(R, Co, Ce, rps) == 0 and L.mx_pw_proj_bwd_fused_groups(R, Co, Ce, rps) == 0, (R, rps)
    for Co, Ce in ((288, 48), (480, 80), (80, 288), (192, 48), (32, 32), (32, 64), (48, 144)):
        assert L.mx_pw_proj_bwd_fused_ok(401408, Co, Ce, 12544) == 0 and L.mx_pw_proj_bwd_fused_groups(401408, Co, Ce, 12544) == 0, (Co, Ce)


def test_bad_arguments_before_any_launch():
    """MX_EARG (-1) with a message naming the entry; the pointers are never dereferenced (they are not device memory)."""
    L = _lib.lib()
    buf = ctypes.create_string_buffer(64)
    p = (ctypes.addressof(buf) & ~15) + 16
    ok = dict(dp=p, d_raw=p, scale=p, shift=p, gate=p, rps=16, Wp=p, dW=p, dA=p, out5=p, R=64, Cout=48, Cexp=288, lddp=48, ldraw=288,
              ldda=288, ws=p, ws_bytes=1 << 30, stream=None)
    bad = [dict(Cout=288, Cexp=48), dict(Cout=480, Cexp=80), dict(Cout=80, Cexp=288), dict(Cout=32, Cexp=32), dict(R=0), dict(R=-16),
           dict(rps=0), dict(rps=8), dict(rps=24), dict(rps=48), dict(R=72), dict(lddp=50), dict(ldraw=290), dict(ldda=289), dict(lddp=44),
           dict(ldraw=284), dict(ldda=192), dict(dp=None), dict(d_raw=None), dict(scale=None), dict(shift=None), dict(gate=None),
           dict(Wp=None), dict(dA=None), dict(out5=None), dict(ws=None), dict(dp=p + 4), dict(dA=p + 8), dict(dW=p + 4), dict(out5=p + 4),
           dict(ws=p + 8), dict(ws_bytes=1024), dict(Cexp=192, ldraw=190)]
    for b in bad:
        a = dict(ok, **b)
        assert L.mx_pw_proj_bwd_fused(*a.values()) == -1, b
        assert b"pw_proj_bwd_fused" in L.mx_last_error(), b


# ---- the backward schedule against a recording stand-in that answers "takes" ------------------------------------------------------
class ProjRecordingOps(RecordingOps):
    """RecordingOps that knows the fused project-conv backward and takes it from 512 rows (the query itself is not logged)."""

    def pw_proj_bwd_fused_takes(self, R, Cout, Cexp, rows_per_sample):
        return R >= 512

    def _r_pw_proj_bwd_fused(self, dp, d_raw, st1, gate, rows_per_sample, Wp, dW, *, defer=None):
        if defer is not None:
            defer(self._e(4, Wp.numel()), dW)
        return self._e(dp.shape[0], d_raw.shape[1]), self._e(5, dp.shape[0] // rows_per_sample, d_raw.shape[1])

    def _r_pw_parts_reduce(self, part, dW):
        return None


def _record(monkeypatch, rec, *, proj_fused: bool):
    from muscle_amd import engine
    monkeypatch.setattr(engine, "ops", rec)
    monkeypatch.setattr(engine, "WGRAD_SIDE_STREAM", False)
    monkeypatch.setattr(engine, "PW_PROJ_BWD_FUSED", proj_fused)
    backbone, cfg, tape, taps = _b0_tape()
    routes = _routes(tape, backbone)
    materialised = [t.a is not None for t in tape.blocks]          # (the backward releases t.a)
    engine.backbone_backward(backbone, cfg, tape, taps, engine.GradSink())
    return rec.calls, tape, routes, materialised


def test_eligible_blocks_take_exactly_one_fused_call(monkeypatch):
    calls, tape, routes, materialised = _record(monkeypatch, ProjRecordingOps(), proj_fused=True)
    blocks = [(t.cfg, tape.N * t.Ho * t.Wo, t.Ho * t.Wo) for t, mat in zip(tape.blocks, materialised)
              if not mat and tape.N * t.Ho * t.Wo >= 512]
    others = [t for t in tape.blocks if t.cfg.index not in {b.index for b, _, _ in blocks}]
    assert blocks and others and any(materialised)
    # the route: "fused" for exactly those blocks; the expand and depthwise stages are the base stand-in's
    assert [t.cfg.index for t, r in zip(tape.blocks, routes) if r.project == "fused"] == [b.index for b, _, _ in blocks]
    assert {r.project for r in routes} == {"fused", "gemm"} and "fused" not in {r.expand for r in routes}
    fused = [c for c in calls if c.startswith("pw_proj_bwd_fused(")]
    assert len(fused) == len(blocks)
    for b, Mo, hw in blocks:
        want = (f"pw_proj_bwd_fused(T[{Mo}, {b.cout}], T[{Mo}, {b.cexp}], BNState, T[{tape.N}, {b.cexp}], {hw}, T[{b.cout}, {b.cexp}], "
                f"T[{b.cout}, {b.cexp}]) defer=<callable>")
        assert fused.count(want) == 1, (want, fused)
        # nothing else for that conv: no data gradient or weight gradient of dp [Mo, Cout], no pooling pass over dA [Mo, Cexp]
        for gone in ("pw_dgrad", "pw_wgrad"):
            assert not [c for c in calls if c.startswith(f"{gone}(T[{Mo}, {b.cout}], ") and f"T[{b.cout}, {b.cexp}]" in c], (gone, b.index)
        assert not [c for c in calls if c.startswith(f"se_bn1_pool(T[{Mo}, {b.cexp}], ")], b.index
    names = [c.split("(")[0] for c in calls]
    # one partial-matrix sum per fused project conv (the stand-in's fused expand convs add none: it knows only the small fold for those)
    assert names.count("pw_parts_reduce") == len(blocks)
    assert names.count("se_bn1_pool") == len(others)
    assert "pw_proj_bwd_fused_takes" not in names


def test_switch_off_restores_the_parents_log(monkeypatch):
    off, _, r_off, _ = _record(monkeypatch, ProjRecordingOps(), proj_fused=False)
    parent, _, r_parent, _ = _record(monkeypatch, RecordingOps(), proj_fused=False)
    assert off == parent and not [c for c in off if c.startswith("pw_proj_bwd_fused(")]
    assert r_off == r_parent and {r.project for r in r_off} == {"gemm"}
    # a stand-in whose kernel takes no shape is untouched by the switch
    on, _, r_on, _ = _record(monkeypatch, RecordingOps(), proj_fused=True)
    assert on == parent and r_on == r_parent

