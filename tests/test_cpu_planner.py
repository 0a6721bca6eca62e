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


def test_backward_routes_reproduce_the_snapshot(restore_settings):
    """engine.block_route, with the library answering its queries, gives every block of the two training steps bench.py times the
    route recorded in the snapshot's "backward_routes" section - which was read off the engine's call log before block_route existed."""
    from muscle_amd import arch
    L, tool = restore_settings, _tool()
    runs = json.load(open(os.path.join(ROOT, "tests", "planner_snapshot.json")))["backward_routes"]
    assert [(r["model"], r["size"], r["batch"], r["gemm_mode"]) for r in runs] == [(*run, g) for run in tool.ROUTE_RUNS for g in tool.ROUTE_MODES]
    for r in runs:
        assert len(r["routes"]) == len(arch.net_cfg(r["model"], False).blocks)
        got = tool.backward_routes(L, r["model"], r["size"], r["batch"], r["gemm_mode"])
        bad = [(i, g, w) for i, (g, w) in enumerate(zip(got, r["routes"])) if g != w]
        assert not bad, (r["model"], r["gemm_mode"], bad[:5])
    # not a table of defaults: B7 takes both fused pointwise backwards, in split arithmetic on more blocks than in exact fp32 (no
    # images of W^T there: the stride-1 quirk block_route keeps)
    b7 = {r["gemm_mode"]: r["routes"] for r in runs if r["model"] == "efficientnet-b7"}
    assert sum(x[0] == "fused" for x in b7[1]) >= 2 and {x[1] for x in b7[1]} == {"fused", "fused_s2"}
    assert sum(x[2] == "fused" for x in b7[1]) > sum(x[2] == "fused" for x in b7[0]) >= 1


def test_the_pipelined_wgrad_kernel_is_gone(restore_settings):
    L = restore_settings
    assert L.mx_set_wgrad_kernel(2, 0) == 0
    assert L.mx_set_wgrad_kernel(1, 0) == -1                      # MX_EARG
    assert b"set_wgrad_kernel" in L.mx_last_error()
    assert L.mx_get_wgrad_kernel() == 2
    for kern in (0, 2):
        assert L.mx_set_wgrad_kernel(kern, 0) == 0 and L.mx_get_wgrad_kernel() == kern


def test_the_lab_only_batchnorm_folds_are_gone():
    """The BatchNorm-0 backward folds into the first-generation data-gradient GEMM and into the tiled split weight gradient (with and
    without the stored dZ) were measured slower and removed: no entry point, no kernel.  Read from the host stubs' mangled names."""
    import re
    from muscle_amd import _build
    L = _lib.lib()
    for name in ("mx_pw_dgrad_bnbwd", "mx_pw_wgrad_tile_bnbwd", "mx_pw_wgrad_tile_bnbwd_ok", "mx_pw_wgrad_tile_bnbwd_dz",
                 "mx_pw_wgrad_tile_bnbwd_dz_ok"):
        assert not hasattr(L, name), name
    for name in ("mx_pw_dgrad_bnbwd_planes", "mx_pw_wgrad_small_bnbwd", "mx_pw_wgrad_small_bnbwd_ok"):      # the live folds
        assert hasattr(L, name), name
    blob = open(_build.LIB, "rb").read()
    assert b"wgrad_split_ws_kernelILb1E" not in blob and b"wgrad_split_ws_kernel" in blob
    assert not re.search(rb"wgrad_split_kernelILi\d+ELb1EE", blob) and re.search(rb"wgrad_split_kernelILi0E", blob)
    nt = re.findall(rb"__device_stub__gemm_nt_kernelILi\d+ELi\d+ELi\d+ELi\d+ELi(\d+)EE", blob)
    assert nt and b"3" not in set(nt), sorted(set(nt))


def test_only_the_gemm_kernels_a_planner_can_select_are_compiled():
    """The built library holds the first-generation gemm_kernel for exactly the (layout, tile) pairs its dispatch can reach,
    no 128 x 256 split tile, and reads no tile override from the environment.  Read from the host stubs' mangled names."""
    import re
    from muscle_amd import _build
    blob = open(_build.LIB, "rb").read()
    got = {tuple(int(x) for x in m) for m in
           re.findall(rb"__device_stub__gemm_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)EE", blob)}
    NN, TN = 1, 2                                   # (layout 0 is NT: the second-generation kernels)
    want = {(NN, 2, 2, 2, 2, 16), (NN, 4, 1, 1, 3, 16), (NN, 4, 1, 1, 2, 16), (NN, 4, 1, 1, 1, 16),       # 128x128, 128x96, 128x64, 128x32
            (TN, 2, 2, 2, 2, 16), (TN, 4, 1, 1, 3, 16), (TN, 4, 1, 1, 1, 16)}                             # 128x128, 128x96, 128x32
    assert got == want, sorted(got ^ want)
    assert b"gemm_kernelILi0E" not in blob
    split = {tuple(int(x) for x in m) for m in re.findall(rb"__device_stub__gemm_nt_split_kernelILi(\d+)ELi(\d+)EE", blob)}
    assert split and all(nj != 4 for _, nj in split), sorted(split)
    assert b"MX_GEMM_SPLIT" in blob
    assert b"MX_GEMM_CFG" not in blob and b"MX_GEMM_SPLIT_NJ" not in blob
