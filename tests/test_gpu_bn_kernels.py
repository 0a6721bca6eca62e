"""Every BatchNorm / pooling entry of muscle_amd/csrc/bn.hip ALONE against the float64 restatements of tests/bn_ref.py, at the
shapes where the launch geometry takes another branch (tests/test_cpu_bn_geometry.py pins where they land): fewer rows than
one pass, short last row blocks, a ragged last column chunk, more float4s than one sweep of the grid-stride loops (RowWalk::next
with row and sample carries), several row blocks per sample (the ordered join with its 4-at-a-time loop and tail, 1000 partials)
and the pipelined eight-row loop of the squeeze.  Every entry runs twice and must give the same bits.

Two input regimes:
  exact   small integers and powers of two everywhere, no swish: every intermediate and every sum is an integer multiple of 1/2
          below 2^23 (asserted from the reference's magnitudes), so float64 is representable and the assertion is torch.equal.
          One dropped or doubled row out of 130 001 fails.
  random  randn inputs, swish on, BN scales in [0.5, 1.5].  Tolerances, in units of u = 2^-24 times the magnitude bn_ref returns:
          - elementwise without swish: k*u*magnitude, k = the number of arithmetic operations on the path (one rounding each;
            contraction only removes some);
          - elementwise with swish: __expf and the reciprocal are not correctly rounded, so the error of the plain fp32 torch
            restatement of the same expression against float64 is MEASURED (a property of the expression and of the input
            distribution: measured once per option set on a fixed 4096 x 256 draw from the same distribution, so that a shape
            with four elements is not judged by the luck of four samples) and the kernel is allowed 4x that;
          - sums: per output (4*e_ref + 2u) * sum|term|, e_ref = the largest error of the fp32 restatement (fp32 terms, torch's
            fp32 .sum) relative to sum|term| on the SAME inputs; the margin 4 covers the other summation tree (chains of up
            to 45 rows, then an ordered join of up to 1000 partials).  Asserted with it: tolerance / sum|term| < 1 / (10 n) for
            n rows per sum, so a dropped row cannot hide (sums over more than 100 000 rows rely on the exact regime).
            Found by this rule: with an fp32 join the 1000-partial sums of one-signed terms (pool_sum with swish, planes 2 and 4 of
            se_bn1_pool at 22990x1024 and 40000x128) were off by 11.7-16.3 u where 9.2-12.1 u were allowed; ordered_sum4 now
            joins more than 64 partials in fp64 (0.6-1.0 u).
No tolerance is taken from a kernel's output.  With BN_KERNELS_PROFILE=<file> every case's e_ref / allowance and the kernel's
error are written there (profiles/bn_kernels_error.txt is one such run).
"""
import functools
import os

import pytest
import torch

import bn_ref
from bn_ref import U

pytestmark = pytest.mark.gpu

DEV = torch.device("cuda:0")
F64, F32 = torch.float64, torch.float32

# (rows, C, rows per sample)
FLAT = [(1, 4, 1), (3, 36, 2), (1000, 36, 333), (777, 1344, 49), (9, 2304, 9), (130001, 36, 1001), (5000, 1040, 784)]
POOL = [(32, 1152, 16), (600, 36, 300), (147, 960, 49), (6274, 1344, 3137), (22990, 1024, 22990), (40000, 128, 40000)]
CALIB = (4096, 256, 64)

APPLY_OPTS = {"plain": (), "act": ("act",), "act_gate": ("act", "gate"), "rs_res": ("rs", "R"), "all": ("act", "gate", "rs", "R")}
BWD_OPTS = {"none": (), "rs": ("rs",), "gate_add_act": ("gate", "act"), "act": ("act",), "all": ("rs", "gate", "act")}
POOL_OPTS = {"plain": (), "affine_act": ("affine", "act"), "G_affine_act": ("G", "affine", "act"), "G": ("G",)}


def _cases(shapes, opts):
    """(shape, option name, exact) - in the exact regime swish is off, and option sets that then coincide run once."""
    out = []
    for s in shapes:
        seen = set()
        for name, o in opts.items():
            out.append(pytest.param(s, name, False, id=f"{s[0]}x{s[1]}x{s[2]}-{name}-random"))
            key = tuple(x for x in o if x != "act")
            if key not in seen:
                seen.add(key)
                out.append(pytest.param(s, name, True, id=f"{s[0]}x{s[1]}x{s[2]}-{name}-exact"))
    return out


_RECORDS = []


def _record(tag, **figures):
    _RECORDS.append(tag + "  " + "  ".join(f"{k}={v:.3g}" for k, v in figures.items()))


@pytest.fixture(scope="module", autouse=True)
def _profile_file():
    yield
    _inputs.cache_clear()            # up to 0.6 GB of device memory: not kept for the rest of the session
    path = os.environ.get("BN_KERNELS_PROFILE")
    if path and _RECORDS:
        with open(path, "w") as f:
            f.write("# tests/test_gpu_bn_kernels.py: errors in units of 2^-24 * magnitude (elementwise: worst element; sums: worst output,\n"
                    "# relative to sum|term|).  ref = the plain fp32 torch restatement against float64, allowed = the test's bound,\n"
                    "# kernel = the HIP kernel against float64.\n")
            f.write("\n".join(_RECORDS) + "\n")


def _pick(table, shape, gen):
    t = torch.tensor(table, dtype=F32, device=DEV)
    return t[torch.randint(0, len(table), shape, device=DEV, generator=gen)]


@functools.lru_cache(maxsize=None)
def _inputs(shape, exact):
    """The operands every entry draws from, made once per (shape, regime) and never written to."""
    rows, C, rps = shape
    N = -(-rows // rps)
    gen = torch.Generator(device=DEV).manual_seed(rows * 7919 + C * 31 + rps + (1 << 20) * exact)
    if exact:
        def ints(lo, hi, *s):
            return torch.randint(lo, hi + 1, s, device=DEV, generator=gen).float()
        d = dict(X=ints(-3, 3, rows, C), G=ints(-3, 3, rows, C), R=ints(-3, 3, rows, C),
                 sc=_pick([-2.0, -1.0, 0.5, 1.0, 2.0], (C,), gen), sh=ints(-2, 2, C),
                 rs=_pick([1.0, 2.0], (N,), gen), gate=_pick([-1.0, 1.0, 2.0], (N, C), gen), add=ints(-2, 2, N, C),
                 c=ints(-2, 2, 3, C))
    else:
        def randn(*s):
            return torch.randn(s, device=DEV, generator=gen)

        def rand(lo, hi, *s):
            return torch.rand(s, device=DEV, generator=gen) * (hi - lo) + lo
        d = dict(X=randn(rows, C), G=randn(rows, C), R=randn(rows, C), sc=rand(0.5, 1.5, C), sh=randn(C) * 0.2,
                 rs=rand(0.5, 1.5, N), gate=rand(0.05, 0.95, N, C), add=randn(N, C) * 0.1,
                 c=torch.stack([rand(0.5, 1.5, C), randn(C) * 0.1, randn(C) * 0.1]))
    return d


def _twice(fn):
    a, b = fn(), fn()
    torch.cuda.synchronize()
    for x, y in zip(a if isinstance(a, (tuple, list)) else (a,), b if isinstance(b, (tuple, list)) else (b,)):
        assert torch.equal(x, y), "two runs gave different bits"
    return a


def _assert_exact(got, ref, mag):
    assert float(mag.max()) < 2 ** 23            # every intermediate is a multiple of 1/2 below 2^23: representable in fp32
    assert torch.equal(ref.float().double(), ref)
    bad = int((got.double() != ref).sum())
    assert bad == 0, f"{bad} of {ref.numel()} outputs differ from the exact result"


def _check_elementwise(tag, got, ref, mag, allowed, ref_units=float("nan")):
    worst = float(((got.double() - ref).abs() / (U * mag).clamp_min(1e-300)).max())
    _record(tag, ref=ref_units, allowed=allowed, kernel=worst)
    assert worst <= allowed, f"{tag}: {worst:.2f} units of 2^-24*magnitude, allowed {allowed:.2f}"


def _sum_rule(ref32, ref, mag):
    """(e_ref, relative tolerance) of the sum rule: both relative to sum|term|."""
    e_ref = float(((ref32.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    return e_ref, 4.0 * e_ref + 2.0 * U


def _check_sums(tag, got, ref, mag, ref32, n):
    e_ref, rel = _sum_rule(ref32, ref, mag)
    worst = float(((got.double() - ref).abs() / mag.clamp_min(1e-300)).max())
    _record(tag, ref=e_ref / U, allowed=rel / U, kernel=worst / U)
    if n <= 100000:
        assert rel < 1.0 / (10.0 * n), f"{tag}: a dropped row could hide ({rel:.3g} >= 1/(10*{n}))"
    assert bool(((got.double() - ref).abs() <= rel * mag).all()), \
        f"{tag}: {worst / U:.2f} units of 2^-24*sum|term|, allowed {rel / U:.2f} (fp32 restatement: {e_ref / U:.2f})"


# ---- option plumbing ------------------------------------------------------------------------------------------------------------
def _apply_kwargs(d, o):
    return dict(rs=d["rs"] if "rs" in o else None, R=d["R"] if "R" in o else None, gate=d["gate"] if "gate" in o else None,
                act="act" in o)


def _geff_kwargs(d, o):
    return dict(rs=d["rs"] if "rs" in o else None, gate=d["gate"] if "gate" in o else None, add=d["add"] if "gate" in o else None,
                a=d["sc"] if "act" in o else None, b=d["sh"] if "act" in o else None)


def _pool_kwargs(d, o):
    return dict(G=d["G"] if "G" in o else None, a=d["sc"] if "affine" in o else None, b=d["sh"] if "affine" in o else None,
                act="act" in o)


def _opts(table, name, exact):
    return tuple(x for x in table[name] if not (exact and x == "act"))


@functools.lru_cache(maxsize=None)
def _swish_units(kind, o):
    """Error of the plain fp32 torch restatement of an elementwise expression with swish against float64, in units of
    2^-24 * magnitude, on a fixed draw of the random regime's input distribution."""
    d = _inputs(CALIB, False)
    if kind == "apply":
        fn = lambda dt: bn_ref.bn_apply(d["X"], d["sc"], d["sh"], CALIB[2], dtype=dt, **_apply_kwargs(d, o))      # noqa: E731
    else:
        fn = lambda dt: bn_ref.bn_bwd_apply(d["G"], d["X"], CALIB[2], d["c"], dtype=dt, **_geff_kwargs(d, o))    # noqa: E731
    ref, mag = fn(F64)
    return float(((fn(F32)[0].double() - ref).abs() / (U * mag)).max())


def _call_bwd_reduce(d, shape, kw):
    from muscle_amd._lib import call, lib, ptr, stream
    rows, C, rps = shape
    part = torch.empty(lib().mx_colreduce_parts(rows, C), 2, C, device=DEV)
    call("mx_bn_bwd_reduce", ptr(d["G"]), ptr(d["X"]), ptr(kw["rs"]), ptr(kw["gate"]), ptr(kw["add"]), ptr(kw["a"]), ptr(kw["b"]),
         rows, C, rps, ptr(part), stream())
    return part


def _call_bwd_apply(G, d, shape, kw, out):
    from muscle_amd._lib import call, ptr, stream
    rows, C, rps = shape
    c = d["c"]
    call("mx_bn_bwd_apply", ptr(G), ptr(d["X"]), ptr(kw["rs"]), ptr(kw["gate"]), ptr(kw["add"]), ptr(kw["a"]), ptr(kw["b"]),
         ptr(c[0]), ptr(c[1]), ptr(c[2]), ptr(out), rows, C, rps, stream())
    return out


# ---- the flat family ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", FLAT, ids=lambda s: "x".join(map(str, s)))
@pytest.mark.parametrize("exact", [False, True], ids=["random", "exact"])
def test_colstats(shape, exact):
    """mx_colstats: partial rows [P, 2, C] of (sum x, sum x^2); their float64 total against the column sums."""
    from muscle_amd import ops
    d = _inputs(shape, exact)
    part = _twice(lambda: ops.colstats(d["X"]))
    assert part.shape[0] == ops.lib().mx_colreduce_parts(shape[0], shape[1])
    got = part.double().sum(0)
    ref, mag = bn_ref.colstats(d["X"])
    if exact:
        _assert_exact(got, ref, mag)
    else:
        _check_sums(f"colstats {shape}", got, ref, mag, bn_ref.colstats(d["X"], dtype=F32)[0], shape[0])


@pytest.mark.parametrize("shape,name,exact", _cases(FLAT, BWD_OPTS))
def test_bn_bwd_reduce(shape, name, exact):
    """mx_bn_bwd_reduce: partial rows of (sum g_eff, sum g_eff * x) for every GEff option."""
    d = _inputs(shape, exact)
    o = _opts(BWD_OPTS, name, exact)
    kw = _geff_kwargs(d, o)
    got = _twice(lambda: _call_bwd_reduce(d, shape, kw)).double().sum(0)
    ref, mag = bn_ref.bn_bwd_reduce(d["G"], d["X"], shape[2], **kw)
    if exact:
        _assert_exact(got, ref, mag)
    else:
        _check_sums(f"bn_bwd_reduce {shape} {name}", got, ref, mag, bn_ref.bn_bwd_reduce(d["G"], d["X"], shape[2], dtype=F32, **kw)[0],
                    shape[0])


@pytest.mark.parametrize("shape,name,exact", _cases(FLAT, APPLY_OPTS))
def test_bn_apply(shape, name, exact):
    """ops.bn_apply: (sc*P + sh) [swish] [* gate[n,c]] [* rs[n]] [+ R]."""
    from muscle_amd import ops
    d = _inputs(shape, exact)
    o = _opts(APPLY_OPTS, name, exact)
    kw = _apply_kwargs(d, o)
    st = ops.BNState(d["sc"], d["sh"], None, None)
    got = _twice(lambda: ops.bn_apply(d["X"], st, row_scale=kw["rs"], residual=kw["R"], gate=kw["gate"], rows_per_sample=shape[2],
                                      act=kw["act"]))
    ref, mag = bn_ref.bn_apply(d["X"], d["sc"], d["sh"], shape[2], **kw)
    if exact:
        _assert_exact(got, ref, mag)
    elif "act" in o:
        units = _swish_units("apply", o)
        _check_elementwise(f"bn_apply {shape} {name}", got, ref, mag, 4.0 * units, units)
    else:
        k = 2 + len(o)                      # multiply, add; one more per gate / row scale / residual
        _check_elementwise(f"bn_apply {shape} {name}", got, ref, mag, float(k))


@pytest.mark.parametrize("shape,name,exact", _cases(FLAT, BWD_OPTS))
def test_bn_bwd_apply(shape, name, exact):
    """mx_bn_bwd_apply: c1*g_eff + c2*x + c3 for every GEff option.  With gate + gate_add the output overwrites G, as the engine's
    BatchNorm-1 backward does (ops.bn_backward_from_coeffs in the random regime, where its swish is on)."""
    from muscle_amd import ops
    d = _inputs(shape, exact)
    o = _opts(BWD_OPTS, name, exact)
    kw = _geff_kwargs(d, o)
    alias = name == "gate_add_act"

    def run():
        if alias:
            G = d["G"].clone()
            if not exact:
                return ops.bn_backward_from_coeffs(G, d["X"], ops.BNState(d["sc"], d["sh"], None, None), d["c"], gate=d["gate"],
                                                   gate_add=d["add"], rows_per_sample=shape[2], out=G)
            return _call_bwd_apply(G, d, shape, kw, G)
        return _call_bwd_apply(d["G"], d, shape, kw, torch.empty_like(d["X"]))
    got = _twice(run)
    ref, mag = bn_ref.bn_bwd_apply(d["G"], d["X"], shape[2], d["c"], **kw)
    if exact:
        _assert_exact(got, ref, mag)
    elif "act" in o:
        units = _swish_units("bwd", o)
        _check_elementwise(f"bn_bwd_apply {shape} {name}", got, ref, mag, 4.0 * units, units)
    else:
        k = 4 + ("rs" in o) + 2 * ("gate" in o)      # c1*g, c2*x, two additions; the row scale; the gate's multiply and add
        _check_elementwise(f"bn_bwd_apply {shape} {name}", got, ref, mag, float(k))


def _bn_module(C, seed):
    g = torch.Generator(device="cpu").manual_seed(seed)
    bn = torch.nn.BatchNorm2d(C).to(DEV)
    with torch.no_grad():
        bn.weight.copy_(torch.rand(C, generator=g) + 0.5)
        bn.bias.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_mean.copy_(torch.randn(C, generator=g) * 0.1)
        bn.running_var.copy_(torch.rand(C, generator=g) + 0.5)
    return bn


@pytest.mark.parametrize("act", [False, True], ids=["plain", "act"])
@pytest.mark.parametrize("training", [True, False], ids=["train", "eval"])
@pytest.mark.parametrize("shape", [FLAT[2], FLAT[3], FLAT[5]], ids=lambda s: "x".join(map(str, s)))
def test_bn_backward_vs_float64_autograd(shape, training, act):
    """ops.bn_backward end to end (statistics -> finalise -> reduce -> finalise -> apply) against torch autograd of F.batch_norm on
    float64: dX, and dgamma / dbeta accumulating onto a non-zero base.

    Tolerances (S = 4*e_ref + 2u, the sum rule for the two backward sums on these inputs; magnitudes as in
    bn_ref.bn_backward_autograd, where the cancellation of x - mean is unravelled so that the fp32 rounding of mean and rstd and
    the error of the statistics are a few u of the same magnitude):
      dbeta   S * sum|g'|  + 2u (|base| + |value|)                       (the += and the fp32 result)
      dgamma  (S + 6u) * sum|g'| xh + 2u (|base| + |value|)              (3u for rstd, u for mean, two products)
      dX      (24u + 2S) * magnitude: 4 operations of the apply pass, and c2, c3 carry r^2, the division by the count, mean and
              the two sums (8 operations and S each)
      with swish: 8u more everywhere for the fp32 scale / shift inside swish' (|swish''| <= 1/2 of a z that is 4 operations
              from x; a systematic offset, it does not average out in the sums); dX also carries the error of g' itself, 4x the
              measured fp32 restatement of the act-only apply pass (in the sums that error is part of e_ref)."""
    from muscle_amd import ops
    rows, C, rps = shape
    d = _inputs(shape, False)
    X = d["X"] * 1.2 + 0.3
    G = d["G"]
    bn = _bn_module(C, 11)
    if training:
        st = ops.bn_finalize(ops.colstats(X), rows, bn, True)
        ops.flush_batch_counters()
    else:
        st = ops.bn_finalize(None, rows, bn, False)
    base = (d["c"][0].clone(), d["c"][1].clone())

    def run():
        dgamma, dbeta = base[0].clone(), base[1].clone()
        dX = ops.bn_backward(G, X, bn, st, dgamma, dbeta, training, act=st if act else None, rows_per_sample=rps)
        return dX, dgamma, dbeta
    dX, dgamma, dbeta = _twice(run)
    (rX, rgamma, rbeta), (mX, mgamma, mbeta) = bn_ref.bn_backward_autograd(G, X, bn.weight, bn.bias, bn.running_mean, bn.running_var,
                                                                          bn.eps, training, act)
    kw = dict(a=st.scale, b=st.shift) if act else {}
    s_ref, s_mag = bn_ref.bn_bwd_reduce(G, X, rps, **kw)
    e_ref, S = _sum_rule(bn_ref.bn_bwd_reduce(G, X, rps, dtype=F32, **kw)[0], s_ref, s_mag)
    shift_u = 8.0 * U if act else 0.0
    swish_u = shift_u + (4.0 * _swish_units("bwd", ("act",)) * U if act else 0.0)
    tag = f"bn_backward {shape} {'train' if training else 'eval'}{' act' if act else ''}"
    for what, got, b, ref, mag, rel in (("dbeta", dbeta, base[1], rbeta, mbeta, S + shift_u),
                                        ("dgamma", dgamma, base[0], rgamma, mgamma, S + 6 * U + shift_u)):
        want = b.double() + ref
        tol = rel * mag + 2 * U * (b.double().abs() + ref.abs())
        err = (got.double() - want).abs()
        _record(f"{tag} {what}", ref=e_ref / U, allowed=float((tol / (U * mag)).min()), kernel=float((err / (U * mag)).max()))
        assert bool((err <= tol).all()), (tag, what, float((err / tol).max()))
    _check_elementwise(f"{tag} dX", dX, rX, mX, 24.0 + 2.0 * S / U + swish_u / U, e_ref / U)


# ---- the per-sample family ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape,name,exact", _cases(POOL, POOL_OPTS))
def test_pool_sum(shape, name, exact):
    """ops.pool_sum: per (sample, channel) sum of [a*x + b] [swish] [* G]."""
    from muscle_amd import ops
    rows, C, rps = shape
    d = _inputs(shape, exact)
    o = _opts(POOL_OPTS, name, exact)
    kw = _pool_kwargs(d, o)
    st = ops.BNState(d["sc"], d["sh"], None, None) if "affine" in o else None
    got = _twice(lambda: ops.pool_sum(d["X"], rps, G=kw["G"], st=st, act=kw["act"]))
    assert got.shape == (rows // rps, C)
    ref, mag = bn_ref.pool_sum(d["X"], rps, **kw)
    if exact:
        _assert_exact(got, ref, mag)
    else:
        _check_sums(f"pool_sum {shape} {name}", got, ref, mag, bn_ref.pool_sum(d["X"], rps, dtype=F32, **kw)[0], rps)


@pytest.mark.parametrize("shape", POOL, ids=lambda s: "x".join(map(str, s)))
def test_se_bn1_pool_planes(shape):
    """ops.se_bn1_pool: each of the five planes against float64 (a plane that is wrong in the same way every run fails here)."""
    from muscle_amd import ops
    rows, C, rps = shape
    d = _inputs(shape, False)
    st = ops.BNState(d["sc"], d["sh"], None, None)
    got = _twice(lambda: ops.se_bn1_pool(d["G"], d["X"], st, rps))
    assert got.shape == (5, rows // rps, C)
    ref, mag = bn_ref.se_bn1_pool(d["G"], d["X"], d["sc"], d["sh"], rps)
    ref32 = bn_ref.se_bn1_pool(d["G"], d["X"], d["sc"], d["sh"], rps, dtype=F32)[0]
    for i in range(5):
        _check_sums(f"se_bn1_pool {shape} plane {i}", got[i], ref[i], mag[i], ref32[i], rps)


@pytest.mark.parametrize("shape", [POOL[2], POOL[3]], ids=lambda s: "x".join(map(str, s)))
def test_se_bn1_pool_feeds_bn1_coeffs_like_the_materialised_path(shape):
    """The five planes through ops.bn1_coeffs against the materialised path (mx_bn_bwd_reduce with gate + gate_add + act, then
    the finalisation): the pooled-path gradient `add` against float64, and dgamma / dbeta / c of BOTH paths against the
    float64 finalisation of the float64 sums.  The two sums carry the sum rule's tolerance S * sum|term| (the larger e_ref of
    the two restatements); it is propagated through bn_bwd_finalize_one's formulas term by term, plus 4u of each result."""
    from muscle_amd import ops
    rows, C, rps = shape
    N, SQ = rows // rps, 24
    d = _inputs(shape, False)
    gen = torch.Generator(device=DEV).manual_seed(rows + C)
    gh = torch.randn(N, SQ, device=DEV, generator=gen)
    W1 = torch.randn(SQ, C, device=DEV, generator=gen) / C ** 0.5
    bn = _bn_module(C, 13)
    mean, rstd = torch.randn(C, device=DEV, generator=gen) * 0.5, torch.rand(C, device=DEV, generator=gen) * 1.5 + 0.5
    st = ops.BNState(d["sc"], d["sh"], mean, rstd)
    base = (d["c"][0].clone(), d["c"][1].clone())
    inv_hw = 1.0 / rps

    def pooled_path():
        dgamma, dbeta = base[0].clone(), base[1].clone()
        p5 = ops.se_bn1_pool(d["G"], d["X"], st, rps)
        c, add = ops.bn1_coeffs(p5, d["gate"], gh, W1, inv_hw, rows, bn, st, dgamma, dbeta, True)
        return c, add, dgamma, dbeta
    c_p, add, dg_p, db_p = _twice(pooled_path)
    add64 = gh.double() @ W1.double() * inv_hw
    add_mag = gh.double().abs() @ W1.double().abs() * inv_hw
    assert bool(((add.double() - add64).abs() <= (SQ + 1) * U * add_mag).all())      # SQ products and additions, the scaling

    kw = dict(rs=None, gate=d["gate"], add=add, a=d["sc"], b=d["sh"])

    def materialised_path():
        dgamma, dbeta = base[0].clone(), base[1].clone()
        c = ops.bn_bwd_coeffs(_call_bwd_reduce(d, shape, kw), rows, bn, st, dgamma, dbeta, True)
        return c, dgamma, dbeta
    c_m, dg_m, db_m = _twice(materialised_path)

    s, smag = bn_ref.bn_bwd_reduce(d["G"], d["X"], rps, **kw)
    e1, _ = _sum_rule(bn_ref.bn_bwd_reduce(d["G"], d["X"], rps, dtype=F32, **kw)[0], s, smag)
    p_ref, p_mag = bn_ref.se_bn1_pool(d["G"], d["X"], d["sc"], d["sh"], rps)
    e2, _ = _sum_rule(bn_ref.se_bn1_pool(d["G"], d["X"], d["sc"], d["sh"], rps, dtype=F32)[0], p_ref, p_mag)
    S = 4.0 * max(e1, e2) + 2.0 * U
    t0, t1 = S * smag[0], S * smag[1]
    dg, db, c = bn_ref.bn_bwd_coeffs(s[0], s[1], float(rows), bn.weight.detach(), mean, rstd, True)
    gm, m, r = bn.weight.detach().double(), mean.double(), rstd.double()
    t_dg = r * (t1 + m.abs() * t0)
    t_k = gm * r * r * t_dg / rows
    tol_c = torch.stack([torch.zeros_like(t0), t_k, gm * r * t0 / rows + t_k * m.abs()])
    c_mag = torch.stack([c[0].abs(), c[1].abs(), (gm * r * s[0] / rows).abs() + (c[1] * m).abs()])
    for tag, cc, dgam, dbet in (("pooled", c_p, dg_p, db_p), ("materialised", c_m, dg_m, db_m)):
        err = (cc.double() - c).abs()
        assert bool((err <= tol_c + 4 * U * c_mag).all()), (tag, "c", float((err / (tol_c + 4 * U * c_mag)).max()))
        for what, got, b, ref, t in (("dgamma", dgam, base[0], dg, t_dg), ("dbeta", dbet, base[1], db, t0)):
            tol = t + 2 * U * (b.double().abs() + ref.abs())
            err = (got.double() - (b.double() + ref)).abs()
            _record(f"bn1_coeffs {shape} {tag} {what}", ref=max(e1, e2) / U, allowed=S / U, kernel=float((err / tol).max()) * S / U)
            assert bool((err <= tol).all()), (tag, what, float((err / tol).max()))
    assert torch.equal(c_p[0], c_m[0])            # gamma * rstd: the same expression in both


def test_arrival_counters_are_left_at_zero():
    """After the per-sample cases above: every launch of the ordered reductions has put its arrival counters back to zero."""
    from muscle_amd import ops
    assert ops._scratch_bufs, "no per-sample case with several row blocks ran before this test"
    for key, buf in ops._scratch_bufs.items():
        assert int(buf[:65536].view(torch.int32).abs().sum()) == 0, key


# ---- finalisers -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N,C,SQ", [(80, 96, 160), (76, 96, 160)])
def test_bn1_sums_finalize_at_the_staging_limit(N, C, SQ):
    """mx_bn1_sums_finalize where the gh table [N][SQ] no longer fits 64 KB of LDS beside the 16 KB of partial sums (N = 80: read
    from global memory) and at the largest batch that still does (N = 76): the float64 checks of test_gpu_se.py."""
    import test_gpu_se
    staged = N * SQ * 4 + 16384 <= 65536
    assert staged == (N == 76)
    test_gpu_se.test_bn1_sums_finalize_vs_fp64(N, C, SQ)


def test_bn1_sums_finalize_variants_agree_bit_for_bit():
    """The same 64 samples through the staged variant (N = 64) and as the first 64 of 80 through the global-memory variant:
    add[n, c] is owned per (n, c) and summed over the squeeze units in ascending order in both, so the bits are the same."""
    from muscle_amd import ops
    N, C, SQ, hw = 80, 96, 160, 784
    gen = torch.Generator(device=DEV).manual_seed(80)
    pooled5 = torch.randn(5, N, C, device=DEV, generator=gen) * 30.0
    gate = torch.rand(N, C, device=DEV, generator=gen) * 0.9 + 0.05
    gh = torch.randn(N, SQ, device=DEV, generator=gen)
    W1 = torch.randn(SQ, C, device=DEV, generator=gen) / C ** 0.5
    bn = _bn_module(C, 17)
    st = ops.BNState(None, None, torch.randn(C, device=DEV, generator=gen) * 0.5, torch.rand(C, device=DEV, generator=gen) + 0.5)

    def run(n):
        dgamma, dbeta = torch.zeros(C, device=DEV), torch.zeros(C, device=DEV)
        c, add = ops.bn1_coeffs(pooled5[:, :n].contiguous(), gate[:n].contiguous(), gh[:n].contiguous(), W1, 1.0 / hw, float(n * hw), bn,
                                st, dgamma, dbeta, True)
        return c, add, dgamma, dbeta
    assert 64 * SQ * 4 + 16384 <= 65536 < N * SQ * 4 + 16384
    full = _twice(lambda: run(N))
    part = _twice(lambda: run(64))
    assert torch.equal(full[1][:64], part[1])
    add64 = gh.double() @ W1.double() / hw
    assert bool(((full[1].double() - add64).abs() <= (SQ + 1) * U * (gh.double().abs() @ W1.double().abs() / hw)).all())


@pytest.mark.parametrize("C", [32, 48, 2304])
def test_bn_finalize_eval_mode(C):
    """mx_bn_finalize with training = 0 and no statistics: scale = gamma / sqrt(running_var + eps), shift = beta - mean * scale from
    the running statistics, which stay bit-unchanged; no batch counter is queued.  4u relative (shift: of |beta| + |mean*scale|):
    the addition, the square root, the division, the product."""
    from muscle_amd import ops
    bn = _bn_module(C, 19 + C)
    rm0, rv0, nbt0 = bn.running_mean.clone(), bn.running_var.clone(), bn.num_batches_tracked.clone()
    pending = len(ops._nbt_pending)
    st = _twice(lambda: tuple(ops.bn_finalize(None, 123.0, bn, False)))
    assert len(ops._nbt_pending) == pending
    assert torch.equal(bn.running_mean, rm0) and torch.equal(bn.running_var, rv0) and torch.equal(bn.num_batches_tracked, nbt0)
    gamma, beta = bn.weight.detach().double(), bn.bias.detach().double()
    rstd = 1.0 / torch.sqrt(rv0.double() + bn.eps)
    scale = gamma * rstd
    for tag, got, ref, mag in (("scale", st[0], scale, scale.abs()), ("shift", st[1], beta - rm0.double() * scale,
                                                                       beta.abs() + (rm0.double() * scale).abs()),
                               ("rstd", st[3], rstd, rstd)):
        _check_elementwise(f"bn_finalize eval C={C} {tag}", got, ref, mag, 4.0)
    assert torch.equal(st[2], rm0)


@pytest.mark.parametrize("cin,cexp,cout", [(16, 96, 24), (384, 2304, 384), (640, 3840, 640), (None, 32, 16)])
def test_fold_block(cin, cexp, cout):
    """ops.fold_block against the float64 folding; (640, 3840, 640) reaches the cap of 1024 workgroups, (None, 32, 16) has no expand
    convolution.  The error of rsqrtf is not documented: e_rs = the error of the one-line fp32 torch restatement
    torch.rsqrt(running_var + eps) against float64 on the same values (in u), and the kernel's s = gamma * rsqrtf(var + eps) is
    allowed 2 * e_rs + 1 (its product); a folded weight one more product; a folded bias beta - s * mean the same on |s * mean| plus
    one rounding of |beta| + |s * mean|.  The second call passes out= and must overwrite the first call's tensors in place."""
    from muscle_amd import ops
    gen = torch.Generator(device=DEV).manual_seed(cexp)
    We = torch.randn(cexp, cin, device=DEV, generator=gen) if cin else None
    Wp = torch.randn(cout, cexp, device=DEV, generator=gen)
    bn0, bn1, bn2 = (_bn_module(cexp, 1) if cin else None), _bn_module(cexp, 2), _bn_module(cout, 3)
    f = ops.fold_block(We, bn0, bn1, Wp, bn2)
    first = {k: f[k].clone() for k in ("We", "be", "Wp", "bp") if k in f}
    first["s1"], first["t1"] = f["bn1"].scale.clone(), f["bn1"].shift.clone()
    ptrs = {k: f[k].data_ptr() for k in ("We", "be", "Wp", "bp", "_vec") if k in f}
    for k in ptrs:
        f[k].fill_(float("nan"))
    f2 = ops.fold_block(We, bn0, bn1, Wp, bn2, out=f)
    torch.cuda.synchronize()
    assert f2 is f and all(f[k].data_ptr() == p for k, p in ptrs.items())
    got = {k: f[k] for k in ("We", "be", "Wp", "bp") if k in f}
    got["s1"], got["t1"] = f["bn1"].scale, f["bn1"].shift
    assert (cin is None) == ("We" not in got)
    for k in got:
        assert torch.equal(got[k], first[k]), k

    def five(bn):
        return (bn.weight, bn.bias, bn.running_mean, bn.running_var, bn.eps)
    ref, mag = bn_ref.fold_block(We, five(bn0) if cin else None, five(bn1), Wp, five(bn2))
    e_rs = 0.0
    for bn in (bn0, bn1, bn2):
        if bn is not None:
            true = 1.0 / torch.sqrt(bn.running_var.double() + bn.eps)
            e_rs = max(e_rs, float(((torch.rsqrt(bn.running_var + bn.eps).double() - true).abs() / (U * true)).max()))
    s_units = 2.0 * e_rs + 1.0
    biases = {"be": bn0, "t1": bn1, "bp": bn2}
    for k in got:
        tag = f"fold_block {(cin, cexp, cout)} {k}"
        if k in biases:
            bn = biases[k]
            s = bn.weight.detach().double() / torch.sqrt(bn.running_var.double() + bn.eps)
            tol = U * ((s_units + 1.0) * (s * bn.running_mean.double()).abs() + mag[k])
            err = (got[k].double() - ref[k]).abs()
            _record(tag, ref=e_rs, allowed=float((tol / (U * mag[k])).min()), kernel=float((err / (U * mag[k])).max()))
            assert bool((err <= tol).all()), (k, float((err / tol).max()))
        else:
            _check_elementwise(tag, got[k], ref[k], mag[k], s_units + (k in ("We", "Wp")), e_rs)
