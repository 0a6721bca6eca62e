"""The native launch planners are frozen: tests/planner_snapshot.json (written by tools/dump_planner.py) records what the
host queries answered before the planners' environment switches became constants; the library must answer the same."""
import importlib.util
import json
import os

import pytest

from muscle_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    spec = importlib.util.spec_from_file_location("dump_planner", os.path.join(ROOT, "tools", "dump_planner.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.fixture
def restore_settings():
    L = _lib.lib()
    mode, kern = L.mx_get_gemm_mode(), L.mx_get_wgrad_kernel()
    yield L
    L.mx_set_gemm_mode(mode)
    L.mx_set_wgrad_kernel(kern, 0)


def test_planners_reproduce_the_snapshot(restore_settings):
    L, tool = restore_settings, _tool()
    snap = json.load(open(os.path.join(ROOT, "tests", "planner_snapshot.json")))
    cols = [f"{name}:x_mode={x}" for name, x in tool.columns()]
    assert snap["columns"] == cols
    assert len(snap["rows"]) >= 600
    # every pointwise convolution of the three models is recorded
    want = tool.model_shapes()
    have = {tuple(row["shape"]) for row in snap["rows"] if row["wgrad_kernel"] is None}
    assert want <= have, sorted(want - have)
    bad = []
    for row in snap["rows"]:
        got = tool.replay(L, row)               # a query that cannot be made raises: a failure, not a skip
        if got != row["results"]:
            bad.append({**row, "got": got, "differs": [c for c, g, w in zip(cols, got, row["results"]) if g != w]})
    assert not bad, f"{len(bad)} of {len(snap['rows'])} rows differ, first: {bad[:3]}"


def test_the_pipelined_wgrad_kernel_is_gone(restore_settings):
    L = restore_settings
    assert L.mx_set_wgrad_kernel(2, 0) == 0
    assert L.mx_set_wgrad_kernel(1, 0) == -1                      # MX_EARG
    assert b"set_wgrad_kernel" in L.mx_last_error()
    assert L.mx_get_wgrad_kernel() == 2
    for kern in (0, 2):
        assert L.mx_set_wgrad_kernel(kern, 0) == 0 and L.mx_get_wgrad_kernel() == kern
