"""What tests/test_gpu_dec_kernels.py and tests/test_gpu_head_kernels.py share: running an entry twice, canaries, the tolerance
checks of the rule in tests/test_gpu_bn_kernels.py (units of U = 2^-24 times the magnitude the float64 reference returns), and the
DEC_KERNELS_PROFILE record."""
import os

import torch

from dec_ref import U, units          # noqa: F401 (units: re-exported)

DEV = torch.device("cuda:0")
CANARY = -7777.25
FLUSH = 2.0 ** -126 / U      # in units of U: a result below the smallest normal fp32 number may be flushed to zero (exp paths)
_HEADER = ("# {name}: errors in units of 2^-24 * magnitude (elementwise: worst element; sums: worst output, relative to sum|term|).\n"
           "# ref = the plain fp32 torch restatement against float64, allowed = the test's bound, kernel = the HIP kernel against float64.\n")


class Profile:
    def __init__(self, name):
        self.name, self.records = name, []

    def record(self, tag, **figures):
        self.records.append(tag + "  " + "  ".join(f"{k}={v:.3g}" for k, v in figures.items()))

    _written = set()          # paths this session has started: the first write truncates, the pair's other file appends

    def write(self):
        path = os.environ.get("DEC_KERNELS_PROFILE")
        if path and self.records:
            mode = "a" if path in Profile._written else "w"
            Profile._written.add(path)
            with open(path, mode) as f:
                f.write(_HEADER.format(name=self.name) + "\n".join(self.records) + "\n")


def twice(fn, frugal=False):
    """fn() twice (it allocates its own outputs): the same bits both times; returns the first result on the CPU.
    frugal: the first result leaves the device before the second run, for outputs of hundreds of megabytes."""
    def tup(r):
        return r if isinstance(r, (tuple, list)) else (r,)
    a = tup(fn())
    if frugal:
        a = tuple(x.cpu() for x in a)
        torch.cuda.empty_cache()
        b = tuple(x.cpu() for x in tup(fn()))
    else:
        b = tup(fn())
    torch.cuda.synchronize()
    for x, y in zip(a, b):
        assert torch.equal(x, y) or bool(((x == y) | (x.isnan() & y.isnan())).all()), "two runs gave different bits"
    out = tuple(x.cpu() for x in a)
    return out if len(out) > 1 else out[0]


def check_elementwise(prof, tag, got, ref, mag, allowed, ref_units=float("nan"), extra_abs=0.0):
    """|got - ref| <= allowed * U * mag + extra_abs (extra_abs: an absolute term in units of U, e.g. the bilinear slope term)."""
    err = (got.double() - ref.double()).abs()
    tol = allowed * U * mag.double() + extra_abs * U
    worst = float((err / tol.clamp_min(1e-300)).max()) * allowed if err.numel() else 0.0
    prof.record(tag, ref=ref_units, allowed=allowed, kernel=worst)
    assert bool((err <= tol).all()), f"{tag}: {worst:.2f} units of 2^-24*magnitude, allowed {allowed:.2f}"


def check_sums(prof, tag, got, ref, mag, e_ref, rel, extra=None):
    """|got - ref| <= rel * sum|term| (+ extra, an absolute tensor: the rounding of a final += for instance)."""
    err = (got.double() - ref.double()).abs()
    tol = rel * mag.double() + (extra if extra is not None else 0.0) + torch.zeros_like(err)
    worst = float((err / tol.clamp_min(1e-300)).max()) * rel if err.numel() else 0.0      # the worst share of its tolerance, as units
    prof.record(tag, ref=e_ref / U, allowed=rel / U, kernel=worst / U)
    assert bool((err <= tol).all()), f"{tag}: {worst / U:.2f} units of 2^-24*sum|term|, allowed {rel / U:.2f} (fp32 restatement: {e_ref / U:.2f})"
