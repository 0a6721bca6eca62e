"""Writes the case table of tests/test_gpu_gemm_nt_units.py (tests/gemm_nt_cases.py): for every compiled instantiation of the
forward / data-gradient GEMM kernels, the smallest shape whose mx_pw_fwd_plan answer is that instantiation, by a search over the
query.  Needs the built library, no GPU.  Run it again after a planner change and review the diff of the table.  (The seven rows of
the removed BatchNorm-backward fold into gemm_nt_kernel were cut from the table by hand: a fresh run deals the option and K cycles
differently from the f1w*m2 rows on.)

    python tools/gemm_unit_cases.py > tests/gemm_nt_cases.py
"""
import itertools
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
from muscle_amd import _lib            # noqa: E402

PLAIN, BNACT, AFFINE, BNBWD = 0, 1, 2, 3
# route -> (entry of mx_pw_fwd_plan, a_mode, arithmetic mode the case sets)
ROUTES = {"fwd": 0, "bgemm": 0, "planes": 1, "planes_act": 1, "bnbwd_planes": 1}
MT = range(1, 700)                                      # row tiles searched: M = 128 * mt - 5 (ragged last tile)
NS = list(range(1, 420)) + list(range(420, 2200, 4))    # (the chunked grid of the planes kernel needs > 16 N tiles)


def nclass(N):
    return "n%4" if N % 4 else "n%16" if N % 16 else "full"


def search(L, entry, gmode, a_mode, K):
    """{(answer, N class, mt % 8 != 0): smallest (M * N, M, N)}"""
    L.mx_set_gemm_mode(gmode)
    best = {}
    for mt in MT:
        M = 128 * mt - 5
        for N in NS:
            ans = L.mx_pw_fwd_plan(entry, a_mode, M, K, N, 1)
            for odd in ((True, False) if mt % 8 else (False,)):
                key = (ans, nclass(N), odd)
                if key not in best or (M * N, M, N) < best[key]:
                    best[key] = (M * N, M, N)
    return best


def main():
    L = _lib.lib()
    before = L.mx_get_gemm_mode()
    rows = []
    any_opts = itertools.cycle(["bias+relu", "stats", "res", "bias+res+relu+stats", "", "res+stats"])
    lean_opts = itertools.cycle(["stats", "res", "", "res+stats"])
    rps_cycle = itertools.cycle([49, 1, 50, 3136])
    idx = 0
    try:
        for fam, gmode, widths, prologues in (
                (1, 0, (32, 48, 64, 80, 96, 128, 160), (("fwd", PLAIN), ("fwd", BNACT), ("fwd", AFFINE))),
                (2, 2, (64, 128), (("fwd", PLAIN), ("fwd", BNACT), ("fwd", AFFINE))),
                (3, 1, (64, 80, 96, 112, 128), (("planes", PLAIN), ("planes_act", BNACT), ("bnbwd_planes", BNBWD)))):
            kc = {1: itertools.cycle([16, 20, 24, 28, 32, 36]), 2: itertools.cycle([16, 36, 32, 24]), 3: itertools.cycle([32, 16, 48, 64])}[fam]
            for route, a_mode in prologues:
                K = 32 if route in ("planes_act", "bnbwd_planes") else None
                found = {}
                for w in widths:
                    if fam == 3 and a_mode == BNACT and w > 96:
                        continue                        # not compiled: the activated form exists up to 96 columns
                    k = K or next(kc)
                    if k not in found:
                        found[k] = search(L, ROUTES[route], gmode, a_mode, k)
                    best = found[k]
                    forms = [f for f in (0, 1, 2) if any(a == fam * 10000 + w * 10 + f for a, _, _ in best)]
                    form = forms[idx % len(forms)]
                    ans = fam * 10000 + w * 10 + form
                    classes = [c for c in ("n%4", "full", "n%16") if (ans, c, form > 0) in best]
                    cls = classes[idx % len(classes)]
                    _, M, N = best[(ans, cls, form > 0)]        # 1-D grids: a row-tile count that is no multiple of 8 (early-return tiles)
                    if route == "bnbwd_planes":
                        opts = "res" if idx % 2 else ""
                    elif route == "planes_act":
                        opts = "stats" if idx % 2 else ""
                    else:
                        opts = next(lean_opts) if cls == "full" else next(any_opts)
                    rps = next(rps_cycle) if a_mode == BNACT else 1
                    rows.append((f"f{fam}w{w}m{a_mode}", route, a_mode, gmode, M, k, N, 1, opts, rps, ans))
                    idx += 1
    finally:
        L.mx_set_gemm_mode(before)
    print('"""Case table of test_gpu_gemm_nt_units.py, written by tools/gemm_unit_cases.py: one row per compiled instantiation of gemm_nt_kernel (f1),')
    print('gemm_nt_split_kernel (f2) and gemm_nt_split3_kernel (f3) at the smallest shape mx_pw_fwd_plan sends there, for the row\'s N class')
    print('(N % 4 != 0, N % 16 != 0, whole tiles) and grid form.  plan = the query\'s answer when the table was written."""')
    print("# (id, route, a_mode, arithmetic mode, M, K, N, batch, epilogue options, rows_per_sample, plan)")
    print("SMALLEST = [")
    for r in rows:
        print(f"    {r!r},")
    print("]")


if __name__ == "__main__":
    main()
