"""engine.block_route decides each block's backward route in one place (no kernel is launched, no device is needed): it agrees with a
literal transcription of the `if` chain the three stage functions used to hold, over every combination of its inputs, and the call
log of engine.backbone_backward under all 16 switch settings, against each of the three recording stand-ins, hashes to what the commit
named in tests/bwd_schedule_hashes.json issued."""
import importlib.util
import itertools
import json
import os

from muscle_amd import engine
from muscle_amd.arch import BlockCfg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SWITCHES = ("FOLD_BN0_EARLY", "DW_S2_FUSED", "PW_BWD_FUSED", "PW_PROJ_BWD_FUSED")


class BoolOps:
    """Stands in for muscle_amd.ops in block_route: the three queries answer from three booleans."""

    def __init__(self, proj, fused, small):
        self.proj, self.fused, self.small = proj, fused, small

    def pw_proj_bwd_fused_takes(self, R, Cout, Cexp, rows_per_sample):
        return self.proj

    def pw_bwd_fused_takes(self, M, K, N):
        return self.fused

    def bnbwd_fold_small_takes(self, M, K, N):
        return self.small


def _old_chain(FOLD_BN0_EARLY, DW_S2_FUSED, PW_BWD_FUSED, PW_PROJ_BWD_FUSED, b, a_is_none, wtp, proj_ok, fused_ok, small_ok):
    """What _project_backward, _depthwise_backward, backbone_backward and _bn0_expand_backward decided between them before block_route
    existed, transcribed condition by condition - on purpose NOT simplified: it is the other side of the comparison.
    ops.bnbwd_fold_takes answered "fused" | "small" | None, ops.bnbwd_fold_takes_split "small" | None."""
    split = "small" if small_ok else None                      # ops.bnbwd_fold_takes_split(M, K, N)
    dw_st = b.expand or b.index == 0                           # _dw_input(t)[1] is not None: BN0, or the stem's BN for block 0
    project = "gemm"                                           # _project_backward
    if a_is_none and PW_PROJ_BWD_FUSED:
        if proj_ok:
            project = "fused"
    if b.stride == 1 and b.pad_lo == (b.kernel - 1) // 2:      # _depthwise_backward
        depthwise, part0 = "fused", (True if dw_st else None)
    elif DW_S2_FUSED and b.stride == 2 and dw_st:
        depthwise, part0 = "fused_s2", True
    else:
        depthwise, part0 = "unfused", None
    if not dw_st:                                              # backbone_backward
        return project, depthwise, "none"
    if part0 is not None:                                      # _bn0_expand_backward
        wtp = wtp if b.expand else None
        takes = None
        if FOLD_BN0_EARLY and b.expand and (wtp is not None if b.stride == 1 else PW_BWD_FUSED):
            takes = "fused" if fused_ok else split             # ops.bnbwd_fold_takes(M, K, N)
            if takes == "fused" and not PW_BWD_FUSED:
                takes = split
        if takes == "fused":
            return project, depthwise, "fused"
        if takes == "small" and b.stride == 1:
            return project, depthwise, "fold"
        return project, depthwise, "apply"
    return project, depthwise, "plain"


def _blocks():
    """Stride 1 and 2, with and without an expand conv, block 0 (behind the stem's BatchNorm) and a later block, 3 x 3 and 5 x 5 with
    the static pad centred, and one stride-1 block whose pad is not (the unfused depthwise backward at stride 1)."""
    out = []
    for index, expand, stride, kernel, centred in itertools.product((0, 5), (False, True), (1, 2), (3, 5), (True, False)):
        pad_lo, cin = ((kernel - 1) // 2 if centred else 0), 24
        out.append(BlockCfg(index=index, cin=cin, cexp=cin * 6 if expand else cin, cout=40, kernel=kernel, stride=stride, se=6,
                            expand=expand, skip=False, pad_lo=pad_lo, pad_hi=kernel - 1 - pad_lo, drop_rate=0.0))
    return out


def test_block_route_is_the_old_if_chain(monkeypatch):
    blocks = _blocks()
    assert {(b.stride, b.expand) for b in blocks} == {(1, False), (1, True), (2, False), (2, True)}
    seen, n = set(), 0
    for sw in itertools.product((False, True), repeat=4):
        for name, v in zip(SWITCHES, sw):
            monkeypatch.setattr(engine, name, v)
        for b, materialised, wt_planes, proj, fused, small in itertools.product(blocks, *[(False, True)] * 5):
            monkeypatch.setattr(engine, "ops", BoolOps(proj, fused, small))
            got = engine.block_route(b, 2, 16, 16, 16 // b.stride, 16 // b.stride, materialised=materialised, wt_planes=wt_planes)
            want = _old_chain(*sw, b, not materialised, 1 if wt_planes else None, proj, fused, small)
            assert tuple(got) == want, (dict(zip(SWITCHES, sw)), b, materialised, wt_planes, proj, fused, small)
            assert isinstance(got, engine.BlockRoute) and (got.project, got.depthwise, got.expand) == want
            seen.add(want)
            n += 1
    assert n == 16 * len(blocks) * 32 and len(blocks) == 32
    # every value of every field is reached, and the two quirks kept on purpose are in the table
    assert {r[0] for r in seen} == {"fused", "gemm"} and {r[1] for r in seen} == {"fused", "fused_s2", "unfused"}
    assert {r[2] for r in seen} == {"none", "plain", "apply", "fold", "fused"}
    s1 = next(b for b in blocks if b.expand and b.stride == 1 and b.pad_lo == (b.kernel - 1) // 2)
    s2 = next(b for b in blocks if b.expand and b.stride == 2)
    monkeypatch.setattr(engine, "ops", BoolOps(False, True, True))
    for name in SWITCHES:
        monkeypatch.setattr(engine, name, True)
    route = lambda b, image: engine.block_route(b, 2, 16, 16, 16 // b.stride, 16 // b.stride, materialised=False, wt_planes=image).expand
    assert (route(s1, True), route(s1, False), route(s2, False)) == ("fused", "apply", "fused")     # no image: stride 1 loses the fused kernel
    monkeypatch.setattr(engine, "FOLD_BN0_EARLY", False)
    assert (route(s1, True), route(s2, True)) == ("apply", "apply")                                 # the fold's switch gates the fused kernel too


def test_project_materialises_is_the_forward_rule(monkeypatch):
    """One function for the three places that asked `does this project conv read a materialised activated input?`."""
    b = lambda cout: BlockCfg(index=3, cin=24, cexp=144, cout=cout, kernel=3, stride=1, se=6, expand=True, skip=False, pad_lo=1, pad_hi=1,
                              drop_rate=0.0)
    monkeypatch.setattr(engine, "MATERIALISE_ABOVE", 128)
    monkeypatch.setattr(engine, "MATERIALISE_ABOVE_EVAL", 1 << 30)
    monkeypatch.setattr(engine, "EVAL_PROLOGUE_MIN_ROWS", 16384)
    for cout, Mo in itertools.product((40, 128, 129, 640), (64, 16383, 16384, 1 << 20)):
        assert engine.project_materialises(b(cout), Mo, True) == (cout > 128)
        assert engine.project_materialises(b(cout), Mo, False) == (Mo < 16384 and cout > 128)
    monkeypatch.setattr(engine, "MATERIALISE_ABOVE_EVAL", 200)
    assert engine.project_materialises(b(640), 1 << 20, False) and not engine.project_materialises(b(160), 1 << 20, False)


def _tool():
    spec = importlib.util.spec_from_file_location("gen_bwd_schedule_hashes", os.path.join(ROOT, "tools", "gen_bwd_schedule_hashes.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_the_schedule_is_the_pinned_one():
    """All 48 call logs (16 switch settings x 3 stand-ins) hash to tests/bwd_schedule_hashes.json.  The file holds hashes only, so a
    mismatch is shown against a regenerated log: one of a case pinned to the same hash that still matches, where there is one."""
    tool = _tool()
    pin = json.load(open(os.path.join(ROOT, "tests", "bwd_schedule_hashes.json")))
    assert pin["switches"] == list(tool.SWITCHES) == list(SWITCHES) and len(pin["generated_from"]) >= 40
    logs = {key: tool.schedule_log(stand_in, setting) for key, stand_in, setting in tool.cases()}
    assert len(logs) == 48 and set(logs) == set(pin["hashes"])
    assert len(set(pin["hashes"].values())) >= 8                              # the switches and the stand-ins do move the schedule
    good = {pin["hashes"][k]: k for k, log in logs.items() if tool.digest(log) == pin["hashes"][k]}
    for key, log in logs.items():
        want = pin["hashes"][key]
        if tool.digest(log) == want:
            continue
        msg = f"{key}: the call log ({len(log)} calls) no longer hashes to the one pinned at {pin['generated_from']}"
        if want in good:
            ref = logs[good[want]]
            i = next((i for i, (a, b) in enumerate(zip(log, ref)) if a != b), min(len(log), len(ref)))
            msg += (f"; against {good[want]} (pinned to the same hash, still matching, {len(ref)} calls) it first differs at call {i}:\n"
                    f"  now:    {log[i] if i < len(log) else '<end>'}\n  pinned: {ref[i] if i < len(ref) else '<end>'}")
        else:
            msg += "; no case pinned to the same hash still matches - its first calls now:\n  " + "\n  ".join(log[:5])
        raise AssertionError(msg)
