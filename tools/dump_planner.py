#!/usr/bin/env python3
"""Dump what the native launch planners decide, as JSON: tests/planner_snapshot.json is this tool's output and
tests/test_cpu_planner.py replays it against the current library.

Only host queries are called (no device is needed).  Shapes: every pointwise convolution of B0 at 224^2 / batch 16, B3 at
448^2 / batch 8 and B7 at 448^2 / batch 32 (muscle_amd/arch.py), plus every (rows, a, b) literal of tests/test_gpu_split.py
and tests/test_gpu_wgrad.py; each in both orientations (a forward GEMM and its data gradient; a weight gradient and its
mirror), for mx_set_gemm_mode 0 / 1 / 2 and the plain / BN+activation operand.  The (R, Co, Ci, groups) rows of the
bit-for-bit test are also asked under mx_set_wgrad_kernel(0 | 2, groups).  A second section, "backward_routes", holds
engine.block_route for every block of the two training steps bench.py times, in both arithmetics (its values in the committed
snapshot were read off the call log of the commit before block_route existed, with a stand-in for muscle_amd.ops that forwarded the
queries to the library).

    python tools/dump_planner.py > tests/planner_snapshot.json
"""
from __future__ import annotations

import ctypes
import json
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from muscle_amd import _lib, arch  # noqa: E402

MODELS = (("efficientnet-b0", 224, 16), ("efficientnet-b3", 448, 8), ("efficientnet-b7", 448, 32))
TEST_FILES = ("tests/test_gpu_split.py", "tests/test_gpu_wgrad.py")
BIT_FOR_BIT = ((25088, 384, 2304, 16), (12544 + 7, 1344, 224, 9), (5003, 640, 384, 4), (3136, 256, 132, 2), (1536, 256, 256, 1),
               (6272, 2304, 384, 5))
PLAIN, BNACT = 0, 1

# query name -> arguments built from (rows, a, b, x_mode); a = the GEMM's K / the weight gradient's Ci, b = N / Co
QUERIES = {
    "mx_gemm_uses_split/0": lambda r, a, b, x: (0, r, b, a),
    "mx_gemm_uses_split/1": lambda r, a, b, x: (1, b, a, r),
    "mx_pw_fwd_uses_planes": lambda r, a, b, x: (r, a, b),
    "mx_pw_fwd_act_uses_planes": lambda r, a, b, x: (r, a, b),
    "mx_pw_wgrad_small_ws": lambda r, a, b, x: (r, b, a, x),
    "mx_pw_wgrad_tile_ws": lambda r, a, b, x: (r, b, a, x),
    "mx_wgrad_uses_split": lambda r, a, b, x: (r, b, a),
    "mx_pw_wgrad_small_bnbwd_ok": lambda r, a, b, x: (r, b, a),
}
WITH_X_MODE = ("mx_pw_wgrad_small_ws", "mx_pw_wgrad_tile_ws")          # the only queries that take x_mode
# the "backward_routes" section: the training steps bench.py times (the headline and configs[1]), in exact-fp32 and split arithmetic
ROUTE_RUNS = (("efficientnet-b7", 448, 32), ("efficientnet-b0", 448, 16))
ROUTE_MODES = (0, 1)
ROUTE_SWITCHES = ("FOLD_BN0_EARLY", "DW_S2_FUSED", "PW_BWD_FUSED", "PW_PROJ_BWD_FUSED")


def model_shapes():
    out = set()
    for name, size, batch in MODELS:
        for last_pooling in (False, True):
            cfg = arch.net_cfg(name, last_pooling)
            h = cfg.stem_out_size(size)
            for b in cfg.blocks:
                ho = b.out_size(h)
                if b.expand:
                    out.add((batch * h * h, b.cin, b.cexp))
                out.add((batch * ho * ho, b.cexp, b.cout))
                h = ho
    return out


def test_shapes():
    """(rows, a, b) from every tuple literal that starts with three integers (rows may be a sum or product: 12544 + 7)."""
    out = set()
    pat = re.compile(r"\(\s*(\d+(?:\s*[+*]\s*\d+)*)\s*,\s*(\d+)\s*,\s*(\d+)\s*[,)]")
    for f in TEST_FILES:
        for m in pat.finditer(open(os.path.join(ROOT, f)).read()):
            rows = eval(m.group(1), {"__builtins__": {}})          # digits, + and * only (see the pattern)
            if rows > 0:
                out.add((rows, int(m.group(2)), int(m.group(3))))
    return out


def query(L, name, args):
    """One host query; mx_wgrad_uses_split is exported but not declared in the header (it returns a C++ bool)."""
    fn = getattr(L, name.split("/")[0])
    if name == "mx_wgrad_uses_split":
        fn.restype, fn.argtypes = ctypes.c_bool, [ctypes.c_int] * 3
    return int(fn(*args))


def columns():
    """The snapshot's columns: (query, x_mode) in a fixed order."""
    return [(name, x) for name in QUERIES for x in ((PLAIN, BNACT) if name in WITH_X_MODE else (PLAIN,))]


def replay(L, row):
    """The library's answers for one snapshot row {gemm_mode, wgrad_kernel: [kernel, groups] | null, shape: [rows, a, b]}, one
    per column (the process-wide wgrad kernel setting is put back)."""
    if L.mx_set_gemm_mode(row["gemm_mode"]) != 0:
        raise RuntimeError(f"mx_set_gemm_mode({row['gemm_mode']}) failed")
    kern = row["wgrad_kernel"]
    if kern is not None and L.mx_set_wgrad_kernel(kern[0], kern[1]) != 0:
        raise RuntimeError(f"mx_set_wgrad_kernel{tuple(kern)} failed")
    try:
        r, a, b = row["shape"]
        return [query(L, name, QUERIES[name](r, a, b, x)) for name, x in columns()]
    finally:
        if kern is not None:
            L.mx_set_wgrad_kernel(2, 0)


def snapshot(L):
    shapes = set()
    for (r, a, b) in model_shapes() | test_shapes():
        shapes.add((r, a, b))
        shapes.add((r, b, a))
    rows = []
    for gemm_mode in (0, 1, 2):
        for shape in sorted(shapes):
            rows.append({"gemm_mode": gemm_mode, "wgrad_kernel": None, "shape": list(shape)})
        for (r, co, ci, groups) in BIT_FOR_BIT:
            for kern in (0, 2):
                rows.append({"gemm_mode": gemm_mode, "wgrad_kernel": [kern, groups], "shape": [r, ci, co]})
    for row in rows:
        row["results"] = replay(L, row)
    return {"columns": [f"{name}:x_mode={x}" for name, x in columns()], "rows": rows}


def backward_routes(L, model, size, batch, gemm_mode):
    """[project, depthwise, expand] of engine.block_route for every block of `model` (last_pooling off) in a training step at
    size x size, with the four schedule switches on and the library answering the queries in arithmetic `gemm_mode`.  What
    block_route is told about the tape is what engine.backbone_forward leaves there: the activated project input where
    project_materialises says so, an image of the expand weight's transpose where the step's WeightPlan builds one (split arithmetic,
    Cexp % 4 == 0, mx_pw_planes_bytes > 0)."""
    from muscle_amd import engine
    if L.mx_set_gemm_mode(gemm_mode) != 0:
        raise RuntimeError(f"mx_set_gemm_mode({gemm_mode}) failed")
    cfg = arch.net_cfg(model, False)
    was = {name: getattr(engine, name) for name in ROUTE_SWITCHES}
    try:
        for name in ROUTE_SWITCHES:
            setattr(engine, name, True)
        out, h = [], cfg.stem_out_size(size)
        for b in cfg.blocks:
            ho = b.out_size(h)
            image = b.expand and gemm_mode != 0 and b.cexp % 4 == 0 and L.mx_pw_planes_bytes(b.cin, b.cexp) > 0
            out.append(list(engine.block_route(b, batch, h, h, ho, ho, materialised=engine.project_materialises(b, batch * ho * ho, True),
                                               wt_planes=image)))
            h = ho
    finally:
        for name, v in was.items():
            setattr(engine, name, v)
    return out


def main():
    L = _lib.lib()
    was = L.mx_get_gemm_mode()
    try:
        snap = snapshot(L)
        routes = [{"model": m, "size": s, "batch": n, "gemm_mode": g, "routes": backward_routes(L, m, s, n, g)}
                  for m, s, n in ROUTE_RUNS for g in ROUTE_MODES]
    finally:
        L.mx_set_gemm_mode(was)
    print('{"columns": ' + json.dumps(snap["columns"]) + ',\n "rows": [')
    print(",\n".join(json.dumps(r, separators=(",", ":")) for r in snap["rows"]))
    print('],\n "backward_routes": [')
    print(",\n".join(json.dumps(r, separators=(",", ":")) for r in routes))
    print("]}")


if __name__ == "__main__":
    main()
