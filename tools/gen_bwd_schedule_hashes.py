#!/usr/bin/env python3
"""Pin the training backward schedule: one sha256 per call log of engine.backbone_backward on the hand-made B0 tape of
tests/test_cpu_dwfused_s2.py, under all 16 settings of the four schedule switches, against each of the three recording stand-ins
for muscle_amd.ops that the CPU schedule tests use.  No device is needed and no kernel is launched.

tests/bwd_schedule_hashes.json is this tool's output at the commit its header names; tests/test_cpu_bwd_route.py recomputes the
hashes on the current tree.  A schedule refactor leaves the file alone; a change that moves a kernel call regenerates it on purpose.
Lines that record a query of the stand-in (any call whose name holds "_takes") are dropped before hashing: what is pinned is the
kernel calls, their arguments and their order, not how the engine asked.

    python tools/gen_bwd_schedule_hashes.py > tests/bwd_schedule_hashes.json
"""
from __future__ import annotations

import hashlib
import itertools
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

SWITCHES = ("FOLD_BN0_EARLY", "DW_S2_FUSED", "PW_BWD_FUSED", "PW_PROJ_BWD_FUSED")
STAND_INS = (("test_cpu_dwfused_s2", "RecordingOps"), ("test_cpu_pw_bwd_fused", "FusedRecordingOps"),
             ("test_cpu_pw_proj_bwd_fused", "ProjRecordingOps"))


def schedule_log(stand_in, setting):
    """The kernel calls of one backward over the B0 tape: `stand_in` = (test module, class), `setting` = one bool per SWITCHES."""
    import importlib
    from muscle_amd import engine
    from test_cpu_dwfused_s2 import _b0_tape
    rec = getattr(importlib.import_module(stand_in[0]), stand_in[1])()
    names = ("ops", "WGRAD_SIDE_STREAM") + SWITCHES
    was = {n: getattr(engine, n) for n in names}
    try:
        engine.ops, engine.WGRAD_SIDE_STREAM = rec, False
        for n, v in zip(SWITCHES, setting):
            setattr(engine, n, v)
        backbone, cfg, tape, taps = _b0_tape()
        engine.backbone_backward(backbone, cfg, tape, taps, engine.GradSink())
    finally:
        for n, v in was.items():
            setattr(engine, n, v)
    return [c for c in rec.calls if "_takes" not in c.split("(")[0]]


def cases():
    """(key, stand-in, setting) of the 48 logs; the key is "<class>/<one digit per switch, in SWITCHES order>"."""
    for stand_in in STAND_INS:
        for setting in itertools.product((False, True), repeat=len(SWITCHES)):
            yield stand_in[1] + "/" + "".join(str(int(v)) for v in setting), stand_in, setting


def digest(lines):
    return hashlib.sha256("\n".join(lines).encode()).hexdigest()


def main():
    commit = subprocess.run(["git", "rev-parse", "HEAD"], cwd=ROOT, capture_output=True, text=True, check=True).stdout.strip()
    dirty = subprocess.run(["git", "status", "--porcelain", "--", "muscle_amd"], cwd=ROOT, capture_output=True, text=True,
                           check=True).stdout.strip()
    out = {"generated_from": commit + (" (muscle_amd/ modified)" if dirty else ""), "switches": list(SWITCHES),
           "hashes": {key: digest(schedule_log(stand_in, setting)) for key, stand_in, setting in cases()}}
    json.dump(out, sys.stdout, indent=1)
    print()


if __name__ == "__main__":
    main()
