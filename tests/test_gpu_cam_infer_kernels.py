"""The CAM inference kernels at the bottom of muscle_amd/csrc/head.hip (mx_infer_accum, mx_cam_infer, mx_infer_norm), each ALONE
against the float64 restatements of tests/cam_infer_ref.py, at the smallest shapes that reach each branch (the tables there;
tests/test_cpu_cam_infer_ref.py checks their input conditions, and that the bounds can see a wrong coordinate rule at all).
Every launch runs twice and must give the same bits; every output carries canaries behind it; the low-resolution maps hold NaN
in channel 0 and in the padding columns, and mx_cam_infer's outputs are NaN-filled before the launch.

Tolerances, by the rule of tests/test_gpu_head_kernels.py, in units of U = 2^-24 times the magnitude the reference returns:
  accumulated maps   per pass 2*BLEND_OPS*U*magnitude + the two slope terms of cam_infer_ref (absolute, from the actual arrays), the
                     sum rule over passes, and 2U(|base| + |ref|) for mx_infer_accum's += on a non-zero base;
  normalisation      NORM_OPS*U*magnitude; the zeroing decision is exact (one fp32 addition) and compared as a set, no pixel is
                     excused; the zeroed pixels' and the maximum's values are the fp32 formula's bits;
  exact              mx_cam_infer == mx_infer_accum from zeros in table order, torch.equal, on every case; both-outputs launches ==
                     single-output launches; the all-negative channel == -1.
No tolerance is taken from a kernel's output.  DEC_KERNELS_PROFILE=<file> records ref (the fp32 restatement) / allowed / kernel of
every case (profiles/cam_infer_kernels_error.txt).
"""
import numpy as np
import pytest
import torch

import cam_infer_ref as R
from dec_ref import U
from dec_gpu_util import CANARY, DEV, Profile, check_elementwise, twice

pytestmark = pytest.mark.gpu

PROF = Profile("tests/test_gpu_cam_infer_kernels.py")
TAIL = 64                                                    # canary elements behind every output
SINGLES = [(g, f) for g in R.GEOMS for f in (0, 1)]
NAN = float("nan")


@pytest.fixture(scope="module", autouse=True)
def _profile_file():
    yield
    PROF.write()


def _id(c):
    return "-".join(map(str, c[0])) + f"-flip{c[1]}"


def _call(name, *args):
    from muscle_amd._lib import call, ptr, stream
    call(name, *(ptr(a) if isinstance(a, torch.Tensor) else a for a in args), stream())


def _out(n, fill):
    """A flat output of n elements filled with `fill` (a number or a CPU tensor), TAIL canaries behind it."""
    buf = torch.full((n + TAIL,), CANARY, device=DEV)
    if isinstance(fill, torch.Tensor):
        buf[:n] = fill.reshape(-1).to(DEV)
    else:
        buf[:n] = fill
    return buf


def _split(buf, shape):
    n = int(np.prod(shape))
    assert bool((buf[n:] == CANARY).all()), "the canaries behind the output were written"
    return buf[:n].view(shape)


def _accum(case, which, base=None):
    """mx_infer_accum per pass in table order over all K-1 channels, from zeros or from `base`; the CPU result [K-1,H,W]."""
    K, lds, H, W = case["K"], case["lds"], case["H"], case["W"]
    maps = [m.to(DEV) for m in case[which]]

    def run():
        buf = _out((K - 1) * H * W, 0.0 if base is None else base)
        for m, (h, w, Hs, Ws, flip) in zip(maps, case["rows"]):
            _call("mx_infer_accum", m, buf, h, w, lds, K, Hs, Ws, H, W, flip)
        return buf
    return _split(twice(run), (K - 1, H, W))


def _cam_infer(case, keep, mode):
    """mx_cam_infer on NaN-filled outputs.  mode 'both' / 'cam' / 'sgc'.  Returns the CPU maps [nkeep,H,W] (None where not asked)."""
    K, lds, H, W = case["K"], case["lds"], case["H"], case["W"]
    cam, sgc = [m.to(DEV) for m in case["cam"]], [m.to(DEV) for m in case["sgc"]]
    tab = torch.tensor([[c.data_ptr(), s.data_ptr(), h, w, Hs, Ws, flip, 0] for c, s, (h, w, Hs, Ws, flip) in zip(cam, sgc, case["rows"])],
                       dtype=torch.int64).to(DEV)
    idx = torch.tensor(keep, dtype=torch.int32).to(DEV)
    n = len(keep) * H * W

    def run():
        oc = _out(n, NAN) if mode in ("both", "cam") else None
        os_ = _out(n, NAN) if mode in ("both", "sgc") else None
        _call("mx_cam_infer", tab, len(case["rows"]), lds, K, H, W, idx, len(keep), oc, os_)
        return tuple(o for o in (oc, os_) if o is not None)
    got = twice(run)
    got = [_split(g, (len(keep), H, W)) for g in (got if isinstance(got, tuple) else (got,))]
    return (got[0], got[1]) if mode == "both" else ((got[0], None) if mode == "cam" else (None, got[0]))


def _check(tag, case, which, got, sel=None, base=None):
    rule = case["rule_" + which]
    idx = slice(None) if sel is None else list(sel)
    ref, mag, extra = rule["ref"][idx], rule["mag"][idx], rule["extra"][idx]
    if base is not None:
        got = got.double() - base.double()
        extra = extra + 2.0 * (base.double().abs() + ref.abs())          # the final += rounds at |base + ref|
    check_elementwise(PROF, tag, got, ref, mag, rule["allowed"], ref_units=R.witness_units(case, which, sel), extra_abs=extra)


class _Zeros:
    """mx_infer_accum from zeros per (case, map), once per test: what every keep list's mx_cam_infer must equal bit for bit."""

    def __init__(self):
        self.got = {}

    def __call__(self, case, which):
        key = (case["rows"], case["H"], case["W"], case["K"], case["lds"], which)
        if key not in self.got:
            self.got[key] = _accum(case, which)
        return self.got[key]


def _cam_infer_case(tag, case, keep, zeros, unequal):
    """The three launches of one (table, keep list): bounds, single == both, and the bit equality with mx_infer_accum (collected in
    `unequal`, asserted by the caller at the end of its sweep so that one failure does not hide the rest)."""
    both_c, both_s = _cam_infer(case, keep, "both")
    only_c, _ = _cam_infer(case, keep, "cam")
    _, only_s = _cam_infer(case, keep, "sgc")
    assert torch.equal(both_c, only_c) and torch.equal(both_s, only_s), f"{tag}: the single-output launches differ from the both-outputs one"
    for which, got in (("cam", both_c), ("sgc", both_s)):
        _check(f"cam_infer {tag} {which}", case, which, got, sel=keep)
        acc = zeros(case, which)[list(keep)]
        if not torch.equal(got, acc):
            unequal.append(f"{tag} {which}: {int((got != acc).sum())} of {got.numel()} elements, max |d| {float((got - acc).abs().max()):.3g}")


# ---- mx_infer_accum ----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLES, ids=_id)
def test_infer_accum(case):
    """One pass over all K-1 channels at every (K, lds) of the channel table, from zeros and added to a random base."""
    geom, flip = case
    for K, lds in R.KLDS:
        c = R.single_case(geom, flip, K, lds)
        tag = f"infer_accum {geom} flip={flip} K={K} lds={lds}"
        _check(tag + " zeros", c, "cam", _accum(c, "cam"))
        base = R.base_for(K, c["H"], c["W"], flip)
        _check(tag + " base", c, "cam", _accum(c, "cam", base), base=base)


def test_infer_accum_above_the_grid_cap():
    a = R.ABOVE_CAP
    c = R.single_case(a["geom"], a["flip"], a["K"], a["lds"])
    assert (a["K"] - 1) * c["H"] * c["W"] > R.GRID_CAP
    base = R.base_for(a["K"], c["H"], c["W"])
    _check("infer_accum above_cap zeros", c, "cam", _accum(c, "cam"))
    _check("infer_accum above_cap base", c, "sgc", _accum(c, "sgc", base), base=base)


@pytest.mark.parametrize("name", list(R.MULTI))
def test_infer_accum_tables(name):
    """The += over the passes of a table, from zeros and from a base."""
    rows, HW = R.MULTI[name]
    c = R.table_case(tuple(rows), HW, 21, 24)
    _check(f"infer_accum {name} zeros", c, "cam", _accum(c, "cam"))
    base = R.base_for(21, c["H"], c["W"], 3)
    _check(f"infer_accum {name} base", c, "sgc", _accum(c, "sgc", base), base=base)


# ---- mx_cam_infer, and its bit equality with mx_infer_accum ------------------------------------------------------------------------
@pytest.mark.parametrize("case", SINGLES, ids=_id)
def test_cam_infer(case):
    geom, flip = case
    zeros, unequal = _Zeros(), []
    for K, lds, keep in R.CHANNELS:
        c = R.single_case(geom, flip, K, lds)
        _cam_infer_case(f"{geom} flip={flip} K={K} lds={lds} keep={list(keep) if len(keep) < 6 else len(keep)}", c, keep, zeros, unequal)
    assert not unequal, "mx_cam_infer != mx_infer_accum from zeros:\n" + "\n".join(unequal)


@pytest.mark.parametrize("name", list(R.MULTI))
def test_cam_infer_tables(name):
    rows, HW = R.MULTI[name]
    c = R.table_case(tuple(rows), HW, 21, 24)
    zeros, unequal = _Zeros(), []
    for keep in R.MULTI_KEEPS:
        _cam_infer_case(f"{name} keep={list(keep) if len(keep) < 6 else len(keep)}", c, keep, zeros, unequal)
    assert not unequal, "mx_cam_infer != mx_infer_accum from zeros:\n" + "\n".join(unequal)


def test_cam_infer_above_the_grid_cap():
    a = R.ABOVE_CAP
    c = R.single_case(a["geom"], a["flip"], a["K"], a["lds"])
    assert c["H"] * c["W"] > R.GRID_CAP
    unequal = []
    _cam_infer_case("above_cap", c, a["keep"], _Zeros(), unequal)
    assert not unequal, "mx_cam_infer != mx_infer_accum from zeros:\n" + "\n".join(unequal)


# ---- mx_infer_norm ------------------------------------------------------------------------------------------------------------------
def _norm_launch(a):
    """mx_infer_norm in place on the C channels of a [C, HW] CPU array, between a neighbouring channel in front and a canary row
    behind; returns the CPU result [C, HW]."""
    C, HW = a.shape
    front = torch.linspace(-3.0, 5.0, HW)

    def run():
        buf = torch.full((C + 2, HW), CANARY, device=DEV)
        buf[0] = front.to(DEV)
        buf[1:C + 1] = torch.from_numpy(np.array(a)).to(DEV)
        _call("mx_infer_norm", buf[1:], C, HW)
        return buf
    buf = twice(run)
    assert torch.equal(buf[0], front), "the channel in front of the launch's first was written"
    assert bool((buf[C + 1] == CANARY).all()), "the canaries behind the last channel were written"
    return buf[1:C + 1].numpy()


def _zeroed_value32(a):
    """[C] fp32: what the kernel's formula gives a zeroed pixel, (0 - mn - 1e-6f) / (mx - mn + 1e-6f), every operation in fp32."""
    v = np.maximum(a.reshape(a.shape[0], -1), np.float32(0.0))
    mn, mx = v.min(1), v.max(1)
    return (np.float32(0.0) - mn - R.EPS32) / (mx - mn + R.EPS32)


def _norm_checks(tag, a, got, ref, kinds):
    """a [C,HW] fp32 input, got [C,HW] the kernel's output, ref = cam_infer_ref.norm(a): the zeroed set, the exact values, the bound."""
    val, mag, zeroed, _ = ref
    want32, z32 = R.norm32(a), _zeroed_value32(a)
    assert np.array_equal(got == z32[:, None], zeroed), f"{tag}: the zeroed set differs from the restatement's"
    assert np.array_equal(got[zeroed], want32[zeroed]), f"{tag}: a zeroed pixel does not hold the formula's value"
    v = np.maximum(a, np.float32(0.0))
    at_max = v == v.max(1, keepdims=True)
    assert np.array_equal(got[at_max], want32[at_max]), f"{tag}: the maximum's pixel does not hold the formula's value"
    for c, kind in enumerate(kinds):
        w = float((np.abs(want32[c].astype(np.float64) - val[c]) / (U * mag[c])).max())
        check_elementwise(PROF, f"infer_norm {tag} {kind}", torch.from_numpy(got[c]), torch.from_numpy(val[c]), torch.from_numpy(mag[c]),
                          float(R.NORM_OPS), ref_units=w)


@pytest.mark.parametrize("HW", R.NORM_HW)
def test_infer_norm(HW):
    """Every channel kind in one launch (the per-channel offset), HW below, at and above the workgroup's 256 threads."""
    a, ref = R.norm_case(HW)
    got = _norm_launch(a)
    _norm_checks(f"HW={HW}", a, got, ref, R.NORM_KINDS)
    neg = R.NORM_KINDS.index("negative")
    assert np.array_equal(got[neg], np.full(HW, -1.0, np.float32)), "the all-negative channel is not exactly -1"


# ---- the pipeline -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("keep", R.MULTI_KEEPS[:2], ids=["all20", "tail"])
def test_cam_infer_then_norm(keep):
    """mx_cam_infer then mx_infer_norm on the script's eight-row table against norm(accum(...)): the discrete step (which pixels
    are zeroed) is fed the kernel's own fp32 sums, the continuous values come from the float64 sums.  The sums' tolerance t goes
    through the formula (v - mn - eps)/den: the numerator moves by at most t + max t (mn is a minimum of the same map), the
    denominator by at most 2 max t, relative to the value."""
    rows, HW = R.MULTI["script"]
    c = R.table_case(tuple(rows), HW, 21, 24)
    for which, sums in zip(("cam", "sgc"), _cam_infer(c, keep, "both")):
        a = sums.numpy()
        a2 = a.reshape(len(keep), -1)
        got = _norm_launch(a2)
        rule = c["rule_" + which]
        val, mag, zeroed, (mn, mx) = R.norm(a2, cont=rule["ref"][list(keep)].reshape(len(keep), -1).numpy())
        assert np.array_equal(got == _zeroed_value32(a2)[:, None], zeroed), "the zeroed set differs from the one of the kernel's own sums"
        t = R.tolerance(rule, list(keep)).reshape(len(keep), -1).numpy()
        tmax = t.max(1, keepdims=True)
        den = (mx - mn + float(R.EPS32))[:, None]
        tol = R.NORM_OPS * U * mag + (t + tmax) / den + np.abs(val) * 2.0 * tmax / den
        err = np.abs(got.astype(np.float64) - val)
        worst = float((err / tol).max())
        PROF.record(f"cam_infer+norm script keep={len(keep)} {which} (share of the tolerance)", ref=float("nan"), allowed=1.0, kernel=worst)
        assert worst <= 1.0, f"{which}: {worst:.3g} of the tolerance"
