"""The ER top-k loss kernels (mx_er_fwd / mx_er_bwd, the low-resolution family mx_er_lr_*), mx_softmaxnorm and the
classification-loss kernel (mx_cls_loss) of muscle_amd/csrc/losses.hip, called directly so that the parked values and the
select's state can be read back, against the references of tests/er_ref.py:

  values   |softmaxnorm(cam) - softmaxnorm(sgc)| * mask in fp64                           max-abs <= 1e-5 max|ref|
  state    prefix (tau bits), krem, cnt_eq, sum_gt == select_oracle(read-back values)     exactly, as integers
  loss     the oracle's fp64 sum rounded to fp32                                          <= 1 ulp
  gradient fp64 autograd with the oracle's weights (1 above tau, krem / cnt_eq at tau)    <= max(2e-5, 4 x fp32-torch error)
  run to run, vals == NULL, k on the device                                               identical bits

The shapes are the smallest that reach each code path: several histogram chunks with an uneven tail, the chunk caps (512
and 256), the grid-stride second trip of the 8192-workgroup cap, H*W % 4 != 0, a second 256-column segment, the band cap
of 32 rows, K != 21 (gather kernel), k at / beyond the non-zero count, thresholds on shared ties.

Ties: the three-class sample of a case holds duplicated pixels (full resolution: a block of rows copied onto another) or a
duplicated class plane (low resolution, where no two pixels interpolate alike), so every value there occurs at least twice;
the k of a "tie" run is the first k from half the production count on at which the read-back values put the threshold on such a
pair (0 < krem < cnt_eq, asserted).  The 41 x 41 case also has 341 identical pixels and a k inside them.

Measured on an MI355X (max-abs error / max|ref|; "fp32" is the same gradient expression in plain fp32 torch on the CPU, and
"bound" = max(2e-5, 4 x fp32) is what the gradient is held to; the values bound is 1e-5 throughout):

  path   case     k-kind  k        values    gradient  fp32      bound     loss ulps
  full   41x41    one     1        2.546e-07 3.017e-08 4.379e-08 2.000e-05 0
  full   41x41    tie     1011     2.546e-07 1.469e-07 1.469e-07 2.000e-05 0
  full   41x41    prod    2017     2.546e-07 1.830e-07 1.830e-07 2.000e-05 1
  full   41x41    nnz     6724     2.546e-07 1.345e-07 1.448e-07 2.000e-05 1
  full   41x41    nnz+5   6729     2.546e-07 1.692e-07 1.692e-07 2.000e-05 0
  full   41x41    all     35301    2.546e-07 1.254e-07 1.381e-07 2.000e-05 0
  full   41x41    const   483      2.546e-07 1.188e-07 1.149e-07 2.000e-05 0
  full   28x28    prod    627      1.927e-07 1.933e-07 1.933e-07 2.000e-05 0
  full   28x28    tie     313      1.927e-07 1.916e-07 1.916e-07 2.000e-05 0
  full   28x28    nnz     3136     1.927e-07 1.654e-07 1.654e-07 2.000e-05 0
  full   8x8      prod    38       2.838e-07 8.823e-08 8.823e-08 2.000e-05 0
  full   kmax     prod    79       2.137e-07 5.471e-08 5.471e-08 2.000e-05 0
  full   kmax     tie     47       2.137e-07 7.479e-08 6.357e-08 2.000e-05 0
  full   kmax     nnz     396      2.137e-07 9.863e-08 9.863e-08 2.000e-05 0
  full   zeros    prod    14       exact 0   exact 0   -         -         0
  full   zeros    all     70       exact 0   exact 0   -         -         0
  full   big      prod    839200   2.348e-07 4.743e-07 4.434e-07 2.000e-05 0
  lowres 35x35    free    980      5.492e-07 1.420e-07 3.436e-07 2.000e-05 0
  lowres 35x35    tie     1963     5.492e-07 1.029e-07 4.404e-07 2.000e-05 0
  lowres 36x36    free    777      5.935e-07 1.656e-07 1.895e-07 2.000e-05 0
  lowres 36x36    tie     1980     5.935e-07 1.689e-07 3.899e-07 2.000e-05 0
  lowres 4x257    free    616      4.085e-07 1.772e-08 2.421e-07 2.000e-05 0
  lowres 4x257    tie     1843     4.085e-07 4.124e-08 3.796e-07 2.000e-05 0
  lowres 12x300   free    2880     2.991e-06 8.451e-07 7.987e-07 2.000e-05 1
  lowres 12x300   tie     2142     2.991e-06 7.734e-07 7.147e-07 2.000e-05 0
  lowres 67x20    free    804      6.211e-07 5.156e-08 6.065e-08 2.000e-05 0
  lowres 67x20    tie     2500     6.211e-07 2.066e-08 3.403e-07 2.000e-05 1
  lowres 9x9      free    48       2.338e-07 6.020e-08 4.178e-07 2.000e-05 0
  lowres 9x9      tie     82       2.338e-07 1.018e-07 4.512e-07 2.000e-05 1
  lowres 6x6      free    21       1.553e-07 5.097e-08 4.742e-08 2.000e-05 0
  lowres 6x6      tie     55       1.553e-07 6.796e-08 5.117e-08 2.000e-05 0
  lowres k5       free    720      4.159e-07 1.138e-07 1.835e-07 2.000e-05 0
  lowres k5       tie     364      4.159e-07 1.140e-07 2.288e-07 2.000e-05 0
  lowres 520x520  free    54080    2.834e-06 1.570e-07 1.313e-06 2.000e-05 0
  lowres 520x520  tie     27289    2.834e-06 1.564e-07 9.838e-07 2.000e-05 1

  softmaxnorm N=1 K=3 HW=2097929 fwd_err=9.984e-08 bwd_err=3.077e-07   (bounds 1e-5 / 2e-5)
  softmaxnorm N=3 K=21 HW=99 fwd_err=1.186e-07 bwd_err=1.397e-07   (bounds 1e-5 / 2e-5)
  cls losses, worst of the 30 (N, C) cases: focal 7.89e-07, soft margin 6.99e-07, pairwise 2.26e-07 (bound 1e-5); d/dlogit 8.77e-07 (bound 2e-5)

Before lr_coord / lr_pixel were compiled without contraction (losses.hip, BIT INVARIANT), the 21-class band kernel dropped
the threshold element and the gradient column read 2.07e-2 (35x35 free), 4.6e-3 (36x36 free), 5.6e-3 / 3.7e-3 (12x300
free / tie) and 1.9e-4 (520x520 tie); the other cases were as above.
"""
import functools

import numpy as np
import pytest
import torch

import er_ref as R
import golden_util as gu
from muscle_amd import synth
from oracle import mcl_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0
RBINS = 2048
TWIN_BIAS = 3.0
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


def _lwb(N, K, sets):
    m = np.zeros((N, K), np.float32)
    m[:, 0] = 1.0
    for n, cls in enumerate(sets):
        m[n, list(cls)] = 1.0
    return m


def _state(N):
    return {"st_u": torch.zeros(3, N, dtype=torch.int32, device=DEV),             # krem, prefix, cnt_eq
            "sum_gt": torch.zeros(N, dtype=torch.int64, device=DEV),
            "hcnt": torch.empty(N * RBINS, dtype=torch.int32, device=DEV),
            "hsum": torch.empty(N * RBINS, dtype=torch.int64, device=DEV),
            "loss": torch.full((1,), float("nan"), dtype=torch.float32, device=DEV)}


def _read(s, **more):
    torch.cuda.synchronize()
    u = s["st_u"].cpu().numpy().view(np.uint32)
    out = {"krem": u[0], "prefix": u[1], "cnt_eq": u[2], "sum_gt": s["sum_gt"].cpu().numpy().view(np.uint64),
           "loss": s["loss"].cpu().numpy()}
    out.update({k: v.cpu() for k, v in more.items() if v is not None})
    return out


def same_bits(a, b, keys=("krem", "prefix", "cnt_eq", "sum_gt", "loss", "grad")):
    for k in keys:
        x, y = a[k], b[k]
        if torch.is_tensor(x):
            assert torch.equal(x.view(torch.int32), y.view(torch.int32)), k
        else:
            assert np.array_equal(x.view(np.uint32), y.view(np.uint32)), k


def check_select(tag, out, rows, k):
    """State exactly the oracle's on the read-back values, loss within 1 ulp of the oracle's.  Returns the oracles."""
    want, os_ = R.select_loss(rows, k)
    for n, o in enumerate(os_):
        got = (int(out["prefix"][n]), int(out["krem"][n]), int(out["sum_gt"][n]))
        assert got == (o["tau_bits"], o["krem"], o["sum_gt_fix"]), (tag, n, got, o)
        if o["tau_bits"] != 0:
            assert int(out["cnt_eq"][n]) == o["cnt_eq"], (tag, n, int(out["cnt_eq"][n]), o)
    got = np.float32(out["loss"][0])
    ulps = abs(int(got.view(np.int32)) - int(want.view(np.int32)))
    print(f"ER_FIG {tag} k={k} loss={got!r} oracle={want!r} ulps={ulps} "
          f"krem/cnt_eq={[(o['krem'], o['cnt_eq']) for o in os_]}")
    assert ulps <= 1, (tag, got, want)
    return os_


def check_values(tag, got, ref):
    sc = float(ref.abs().max())
    if sc == 0.0:
        assert not got.any(), tag
        return
    err = float((T(got).double() - ref).abs().max()) / sc
    print(f"ER_FIG {tag} values_err={err:.3e}")
    assert err <= 1e-5, (tag, err)


def check_grad(tag, g, ref64, ref32):
    """<= max(2e-5 [the bound of test_er_golden], 4 x the error of the same expression in fp32 torch) of max|ref|."""
    sc = float(ref64.abs().max())
    if sc == 0.0:
        assert not g.any(), tag
        return
    err = float((g.double() - ref64).abs().max()) / sc
    e32 = float((ref32.double() - ref64).abs().max()) / sc
    print(f"ER_FIG {tag} grad_err={err:.3e} fp32_torch_err={e32:.3e} bound={max(2e-5, 4 * e32):.3e}")
    assert err <= max(2e-5, 4 * e32), (tag, err, e32)


# ---------------------------------------------------------------------------------------------------------------------
# full-resolution path
# ---------------------------------------------------------------------------------------------------------------------
FULL = {
    # 3 histogram chunks of 11767 = 7 planes each; the three-class sample labels the planes that END a chunk (6, 13, 20), so an
    # element lost at a chunk's tail is a non-zero one and the runs that count every non-zero value notice; every kind of k
    "41x41": dict(N=4, K=21, H=41, W=41, seed=11, labels=[(5,), (6, 13, 20), (), "synth"], tie_n=1, const_n=0,
                  ks=("one", "tie", "prod", "nnz", "nnz+5", "all", "const")),
    # row_len 16464, just over one chunk: 2 chunks of 8232, ending inside plane 10 and with plane 20
    "28x28": dict(N=2, K=21, H=28, W=28, seed=12, labels=[(4, 10, 20), (13,)], tie_n=0, ks=("prod", "tie", "nnz")),
    "8x8": dict(N=3, K=21, H=8, W=8, seed=13, labels="synth", ks=("prod",)),
    "kmax": dict(N=2, K=32, H=9, W=11, seed=14, labels=[(1, 17, 31), (31,)], tie_n=0, ks=("prod", "tie", "nnz")),
    "zeros": dict(N=2, K=2, H=7, W=5, seed=15, labels=[(1,), (1,)], ks=("prod", "all")),      # one foreground class: softmax == 1
    # N*HW > 8192 * 256 (grid-stride second trip), row_len 10.49 M: 512 chunks
    "big": dict(N=1, K=5, H=1049, W=2000, seed=16, labels=[(1, 3)], repair=True, ks=("prod",)),
}


def _labels(c):
    N, K = c["N"], c["K"]
    lab = c["labels"]
    if lab == "synth":
        return np.concatenate([np.ones((N, 1), np.float32), synth.synth_labels(N, c["seed"])], 1)
    sets = [tuple(np.nonzero(synth.synth_labels(N, c["seed"])[n])[0] + 1) if s == "synth" else s for n, s in enumerate(lab)]
    return _lwb(N, K, sets)


@functools.lru_cache(maxsize=1)         # the tests of a case run back to back; the next case releases it
def full_inputs(name):
    """Inputs and the fp64 value reference of a case (CPU only), with the case's input condition asserted."""
    c = FULL[name]
    N, K, H, W = c["N"], c["K"], c["H"], c["W"]
    cams = synth.normal(c["seed"], f"er.{name}.cam", (N, K, H, W)).astype(np.float32)
    sgcs = synth.normal(c["seed"], f"er.{name}.sgc", (N, K, H, W)).astype(np.float32)
    lwb = _labels(c)
    for a in (cams, sgcs):
        if c.get("tie_n") is not None:                    # a block of rows copied onto another: every value there twice
            a[c["tie_n"], :, H // 2:H // 2 + H // 4] = a[c["tie_n"], :, :H // 4]
        if c.get("const_n") is not None:                  # 341 identical pixels
            f = a[c["const_n"]].reshape(K, -1)
            f[:, 1000:1340] = f[:, :1]
    ref = R.er_values_ref(cams, sgcs, lwb)
    if c.get("repair"):
        # 6 M active values: some |a - b| fall below 1e-6 whatever the seed.  Those pixels take the vectors of pixel 0.
        bad = ((ref > 0) & (ref < 1e-5)).any(dim=1).reshape(N, -1).numpy()
        assert not bad[:, 0].any()
        for a in (cams, sgcs):
            f = a.reshape(N, K, -1)
            for n in range(N):
                f[n][:, bad[n]] = f[n][:, :1]
        print(f"ER_FIG full {name} repaired_pixels={int(bad.sum())}")
        ref = R.er_values_ref(cams, sgcs, lwb)
    nz = ref[ref > 0]
    assert nz.numel() == 0 or float(nz.min()) > 1e-6, float(nz.min())       # an fp32 sign can differ from fp64 below that
    return {"N": N, "K": K, "HW": H * W, "cams": cams, "sgcs": sgcs, "lwb": lwb, "ref": ref}


def run_full(c, k):
    N, K, HW = c["N"], c["K"], c["HW"]
    from muscle_amd._lib import call, ptr, stream
    s = _state(N)
    d = torch.full((N * K * HW,), SENT, dtype=torch.float32, device=DEV)
    u = s["st_u"]
    call("mx_er_fwd", ptr(c["dc"]), ptr(c["ds"]), ptr(c["dm"]), N, K, HW, int(k), ptr(d), ptr(u[0]), ptr(u[1]), ptr(s["sum_gt"]),
         ptr(u[2]), ptr(s["hcnt"]), ptr(s["hsum"]), ptr(s["loss"]), stream())
    g = torch.full((N, K, HW), SENT, dtype=torch.float32, device=DEV)
    call("mx_er_bwd", ptr(c["dc"]), ptr(c["ds"]), ptr(c["dm"]), ptr(u[1]), ptr(u[0]), ptr(u[2]), None, 1.0 / (N * int(k)), ptr(g),
         N, K, HW, stream())
    return _read(s, d=d.reshape(N, K * HW), grad=g)


@functools.lru_cache(maxsize=1)         # the tests of a case run back to back; the next case releases it
def full_case(name):
    c = dict(full_inputs(name))
    N, K, HW = c["N"], c["K"], c["HW"]
    c["dc"], c["ds"], c["dm"] = T(c["cams"]).to(DEV), T(c["sgcs"]).to(DEV), T(c["lwb"]).to(DEV)
    d0 = run_full(c, 1)["d"].numpy()                      # the values do not depend on k
    f, tn = FULL[name], FULL[name].get("tie_n")
    prod = int(0.2 * int(c["lwb"][:, 1:].sum()) * HW)     # train_mcl.py:178 (valid_channel is summed over the batch)
    nnz = int((c["ref"][tn if tn is not None else 0] > 0).sum())
    ks = {"one": 1, "prod": prod, "nnz": nnz, "nnz+5": nnz + 5, "all": K * HW}
    if tn is not None:
        ks["tie"] = R.tie_k(d0[tn], prod // 2, odd=True)
    if f.get("const_n") is not None:                      # inside the 341 copies of pixel 0's value of the labelled class
        cn = f["const_n"]
        v = d0[cn].reshape(K, HW)[f["labels"][cn][0], 0]
        ks["const"] = int((d0[cn] > v).sum()) + 120
    c["ks"] = ks
    return c


@pytest.mark.parametrize("name,kname", [(n, kn) for n, c in FULL.items() for kn in c["ks"]])
def test_er_full(name, kname):
    c = full_case(name)
    N, K, HW = c["N"], c["K"], c["HW"]
    k, tag = c["ks"][kname], f"full {name} {kname}"
    a, b = run_full(c, k), run_full(c, k)
    d = a["d"].numpy()
    check_values(tag, d.reshape(c["ref"].shape), c["ref"])                                   # a.
    os_ = check_select(tag, a, d, k)                                                         # b. c.
    same_bits(a, b)                                                                          # d.
    f = FULL[name]
    if kname == "tie":
        o = os_[f["tie_n"]]
        assert o["cnt_eq"] >= 2 and 0 < o["krem"] < o["cnt_eq"] and k % 2 == 1, o
    if kname == "const":
        o = os_[f["const_n"]]
        assert o["cnt_eq"] >= 300 and 0 < o["krem"] < o["cnt_eq"], o
    if kname in ("nnz+5", "all"):                           # beyond the non-zero count (of the tie sample / of every sample)
        assert all(o["tau_bits"] == 0 and o["krem"] > 0 for o in (os_ if kname == "all" else [os_[f["tie_n"]]]))
    if kname == "nnz":
        assert os_[f["tie_n"]]["tau_bits"] != 0 and R.select_oracle(d[f["tie_n"]], k + 1)["tau_bits"] == 0
    if name == "zeros":
        assert not a["prefix"].any() and float(a["loss"][0]) == 0.0 and not a["grad"].any()
    w = R.select_weights(d, os_)                                                             # e.
    g64 = R.er_grad_ref(c["cams"], c["sgcs"], c["lwb"], w, k)
    g32 = R.er_grad_ref(c["cams"], c["sgcs"], c["lwb"], w, k, dtype=torch.float32)
    g = a["grad"].reshape(g64.shape)
    assert not g[:, 0].any()
    check_grad(tag, g, g64, g32)


def test_er_loss_wrapper_matches_direct_call():
    import muscle_amd as M
    c = full_case("8x8")
    vc = int(c["lwb"][:, 1:].sum())
    want = run_full(c, c["ks"]["prod"])
    s = c["ds"].reshape(c["cams"].shape).clone().requires_grad_()
    got = M.er_loss(c["dc"].reshape(c["cams"].shape), s, c["dm"], vc)
    got.backward()
    assert torch.equal(got.detach().cpu().reshape(1), T(want["loss"]))
    assert torch.equal(s.grad.cpu().reshape(want["grad"].shape), want["grad"])


@pytest.mark.parametrize("N,K,HW", [(1, 3, 8192 * 256 + 777), (3, 21, 99)])
def test_softmaxnorm_direct(N, K, HW):
    """Forward and backward against fp64 autograd of the oracle; the first shape takes the grid-stride loop's second trip
    (8192 workgroups x 256 pixels) with a ragged tail."""
    from muscle_amd._lib import call, ptr, stream
    x = T(synth.normal(21, f"smn.x{K}", (N, K, HW, 1)).astype(np.float32))
    gy = T(synth.normal(21, f"smn.g{K}", (N, K, HW, 1)).astype(np.float32))
    x64 = x.double().requires_grad_()
    y64 = O.cam_softmaxnorm(x64)
    y64.backward(gy.double())
    xd, gd = x.to(DEV), gy.to(DEV)
    outs = []
    for _ in range(2):
        y, gx = torch.full_like(xd, SENT), torch.full_like(xd, SENT)
        call("mx_softmaxnorm", ptr(xd), None, ptr(y), N, K, HW, 0, stream())
        call("mx_softmaxnorm", ptr(xd), ptr(gd), ptr(gx), N, K, HW, 1, stream())
        torch.cuda.synchronize()
        outs.append((y.cpu(), gx.cpu()))
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1])
    ef, eb = gu.rel_err(outs[0][0], y64.detach()), gu.rel_err(outs[0][1], x64.grad)
    print(f"ER_FIG softmaxnorm N={N} K={K} HW={HW} fwd_err={ef:.3e} bwd_err={eb:.3e}")
    assert ef <= 1e-5 and eb <= 2e-5, (ef, eb)
    assert not outs[0][1][:, 0].any()


# ---------------------------------------------------------------------------------------------------------------------
# low-resolution path
# ---------------------------------------------------------------------------------------------------------------------
LR = {
    # name: N, h, w, L, K, H, W; labels per sample (the first sample's last class is a copy of the one before it)
    "35x35": dict(N=2, h=5, w=5, L=24, K=21, H=35, W=35, seed=31, labels=[(3, 7, 12), (5,)]),      # 2 chunks, H*W % 4 = 1
    "36x36": dict(N=2, h=5, w=5, L=24, K=21, H=36, W=36, seed=32, labels=[(3, 7, 12), ()]),        # 2 chunks, 16-byte loads
    "4x257": dict(N=1, h=3, w=4, L=24, K=21, H=4, W=257, seed=33, labels=[(3, 7, 12)]),            # per 514 -> 516; 1-pixel segment
    "12x300": dict(N=2, h=3, w=20, L=24, K=21, H=12, W=300, seed=49, labels=[(3, 7, 12), (5,)]),   # two column segments, xb > 0
    "67x20": dict(N=1, h=2, w=3, L=24, K=21, H=67, W=20, seed=35, labels=[(3, 7, 12)]),            # ty 66 -> 32
    "9x9": dict(N=1, h=1, w=1, L=24, K=21, H=9, W=9, seed=36, labels=[(3, 7, 12)]),                # scale 0: every pixel alike
    "6x6": dict(N=1, h=6, w=6, L=24, K=21, H=6, W=6, seed=37, labels=[(3, 7, 12)]),                # identity
    "k5": dict(N=2, h=4, w=4, L=8, K=5, H=30, W=30, seed=38, labels=[(1, 2, 4), (3,)]),            # gather kernel
    # 256 chunks (cap).  One class, so no twin plane: the "tie" run takes one of the chance collisions among the 540 k fp32
    # values (thousands are expected; tie_k asserts that it found one).  Which pair that is moves with the kernel's arithmetic.
    "520x520": dict(N=1, h=17, w=17, L=24, K=21, H=520, W=520, seed=39, labels=[(7,)], shifted=True),
}


@functools.lru_cache(maxsize=1)         # the tests of a case run back to back; the next case releases it
def lr_inputs(name):
    c = LR[name]
    N, h, w, L, K, H, W = (c[k] for k in ("N", "h", "w", "L", "K", "H", "W"))
    cam = synth.normal(c["seed"], f"erlr.{name}.cam", (N, h, w, L)).astype(np.float32)
    sgc = synth.normal(c["seed"], f"erlr.{name}.sgc", (N, h, w, L)).astype(np.float32)
    lwb = _lwb(N, K, c["labels"])
    if len(c["labels"][0]) == 3:                          # twin class planes: every value of the two occurs at least twice
        t1, t2 = c["labels"][0][1:]
        for m in (cam, sgc):
            m[0, :, :, t1] -= TWIN_BIAS
            m[0, :, :, t2] = m[0, :, :, t1]
            # ... and the twins are nowhere the largest class: the background's 1 - max has one gradient, not a choice of two
            u = R.upsample_lr(m[:1], K, H, W)[0].numpy()
            rest = np.delete(u, [0, t1, t2], axis=0).max(axis=0)
            assert float((rest - u[t1]).min()) > 0.25, float((rest - u[t1]).min())
    if c.get("shifted"):
        # 540 k active values of two random fields have differences below 1e-6 whatever the seed.  Here the SGC is the CAM with
        # the labelled class raised by 2, and that class is never the largest (- 3 in both): its probability grows and every
        # other one, the background's maximum included, shrinks at every pixel, so no difference changes sign.
        j = c["labels"][0][0]
        cam[0, :, :, j] -= 3.0
        sgc[0] = cam[0]
        sgc[0, :, :, j] += 2.0
    ref = R.er_values_lr_ref(cam, sgc, lwb, K, H, W)
    nz = ref[ref > 0]
    assert float(nz.min()) > 1e-6, float(nz.min())
    return {"dims": (N, h, w, L, K, H, W), "cam": cam, "sgc": sgc, "lwb": lwb, "ref": ref}


def run_lr(c, k, park=True, k_on_device=False):
    from muscle_amd._lib import call, lib, ptr, stream
    N, h, w, L, K, H, W = c["dims"]
    s = _state(N)
    u = s["st_u"]
    vals = torch.full((N * K * H * W,), SENT, dtype=torch.float32, device=DEV) if park else None
    kd = torch.tensor([k], dtype=torch.int32, device=DEV) if k_on_device else None
    call("mx_er_lr_fwd", ptr(c["dc"]), ptr(c["ds"]), ptr(c["dm"]), N, h, w, L, K, H, W, 0 if k_on_device else int(k), ptr(kd),
         ptr(u[0]), ptr(u[1]), ptr(s["sum_gt"]), ptr(u[2]), ptr(s["hcnt"]), ptr(s["hsum"]), ptr(vals), ptr(s["loss"]), stream())
    need = lib().mx_er_lr_bwd_ws(N, h, w, L, K)
    assert need == (N * h * w * L * 8 if K == 21 else 0)
    ws = torch.empty(max(need, 8), dtype=torch.uint8, device=DEV)
    g = torch.full((N, h, w, L), SENT, dtype=torch.float32, device=DEV)
    call("mx_er_lr_bwd", ptr(c["dc"]), ptr(c["ds"]), ptr(c["dm"]), ptr(u[1]), ptr(u[0]), ptr(u[2]), None,
         0.0 if k_on_device else 1.0 / (N * int(k)), ptr(kd), ptr(g), N, h, w, L, K, H, W, ws.data_ptr(), need, stream())
    return _read(s, vals=None if vals is None else vals.reshape(N, K, H * W), grad=g)


@functools.lru_cache(maxsize=1)         # the tests of a case run back to back; the next case releases it
def lr_case(name):
    c = dict(lr_inputs(name))
    N, h, w, L, K, H, W = c["dims"]
    c["dc"], c["ds"], c["dm"] = T(c["cam"]).to(DEV), T(c["sgc"]).to(DEV), T(c["lwb"]).to(DEV)
    v0 = run_lr(c, 1)["vals"].numpy()
    row0 = np.where(c["lwb"][0][:, None] != 0, v0[0], 0.0).astype(np.float32)
    prod = int(0.2 * int(c["lwb"][:, 1:].sum()) * H * W)
    free = R.free_k(row0, prod)
    c["ks"] = {"prod": prod, "free": free if free is not None else prod, "tie": R.tie_k(row0, prod // 2)}
    return c


@pytest.mark.parametrize("kname", ["free", "tie"])
@pytest.mark.parametrize("name", list(LR))
def test_er_lowres(name, kname):
    c = lr_case(name)
    N, h, w, L, K, H, W = c["dims"]
    k, tag = c["ks"][kname], f"lowres {name} {kname}"
    a = run_lr(c, k)
    vals = a["vals"].numpy()
    act = np.broadcast_to(c["lwb"][:, :, None] != 0, vals.shape)
    assert (vals[~act] == np.float32(SENT)).all()                                            # a.
    rows = np.where(act, vals, np.float32(0)).reshape(N, K * H * W)
    check_values(tag, rows.reshape(c["ref"].shape), c["ref"])                                # b.
    os_ = check_select(tag, a, rows, k)                                                      # c.
    if kname == "tie":
        assert os_[0]["cnt_eq"] >= 2 and 0 < os_[0]["krem"] < os_[0]["cnt_eq"], os_[0]
    elif name != "9x9":
        assert os_[0]["cnt_eq"] == 1, os_[0]
    same_bits(a, run_lr(c, k, park=False))                                                   # d.
    same_bits(a, run_lr(c, k, k_on_device=True))                                             # e.
    same_bits(a, run_lr(c, k))                                                               # g.
    wts = R.select_weights(rows, os_)                                                        # f.
    g64 = R.er_grad_ref(c["cam"], c["sgc"], c["lwb"], wts, k, lr=(K, H, W))
    g32 = R.er_grad_ref(c["cam"], c["sgc"], c["lwb"], wts, k, lr=(K, H, W), dtype=torch.float32)
    g = a["grad"]
    assert not g[..., 0].any() and not g[..., K:].any()
    check_grad(tag, g, g64, g32)


def test_er_loss_lowres_wrapper_matches_direct_calls():
    """The public autograd function, with the host count and with the device count, on three calls of different size: the
    parked-values buffer grows at the second call and is reused, stale contents and all, at the third."""
    from muscle_amd.train_step import er_loss_lowres
    for name in ["4x257", "36x36", "6x6"]:
        c = lr_case(name)
        N, h, w, L, K, H, W = c["dims"]
        vc = int(c["lwb"][:, 1:].sum())
        want = run_lr(c, c["ks"]["prod"])
        for valid in (vc, torch.tensor(float(vc), device=DEV)):
            s = c["ds"].clone().requires_grad_()
            got = er_loss_lowres(c["dc"], s, c["dm"], valid, H, W)
            got.backward()
            assert torch.equal(got.detach().cpu().reshape(1), T(want["loss"])), name
            assert torch.equal(s.grad.cpu(), want["grad"]), name


# ---------------------------------------------------------------------------------------------------------------------
# classification losses: the one-workgroup kernel takes 1024 threads, samples strided over 16 waves, from N = 16
# ---------------------------------------------------------------------------------------------------------------------
def _cls_inputs(N, C):
    lab = np.tile(synth.synth_labels(N, 40 + C), (1, (C + 19) // 20))[:, :C].copy()
    if N >= 3:
        lab[N - 1], lab[N - 2] = 0.0, 1.0
    logit = synth.normal(41, f"cls.{N}.{C}", (N, C)).astype(np.float32) * 2
    return T(logit), T(lab)


@pytest.mark.parametrize("C", [1, 20, 64, 65, 200])
@pytest.mark.parametrize("N", [1, 15, 16, 17, 33, 1024])
def test_cls_losses_vs_fp64(N, C):
    import muscle_amd as M
    logit, lab = _cls_inputs(N, C)
    x64 = logit.double().requires_grad_()
    p64 = torch.sigmoid(x64)
    r1, r2, r3 = O.focal_loss(p64, lab.double()), O.multilabel_soft_margin(x64, lab.double()), O.log_sum_exp_pairwise(p64, lab.double())
    (r1 + r2 + r3.mean()).backward()
    r1, r2, r3 = r1.detach(), r2.detach(), r3.detach()
    outs = []
    for _ in range(2):
        x = logit.to(DEV).requires_grad_()
        p = M.loss_multilabel.sigmoid(x)
        l1, l2 = M.FocalLoss()(p, lab.to(DEV)), M.MultiLabelSoftMarginLoss()(x, lab.to(DEV))
        l3 = M.Log_Sum_Exp_Pairwise_Loss(p, lab.to(DEV))
        (l1 + l2 + l3.mean()).backward()
        outs.append((torch.stack([l1, l2]).detach().cpu(), l3.detach().cpu(), x.grad.cpu()))
    for a, b in zip(*outs):
        assert torch.equal(a, b)
    e = [abs(float(outs[0][0][0]) - float(r1)) / abs(float(r1)), abs(float(outs[0][0][1]) - float(r2)) / abs(float(r2)),
         gu.rel_err(outs[0][1], r3), gu.rel_err(outs[0][2], x64.grad)]
    print(f"ER_FIG cls N={N} C={C} focal={e[0]:.2e} softmargin={e[1]:.2e} pairwise={e[2]:.2e} dlogit={e[3]:.2e}")
    assert max(e[:3]) <= 1e-5 and e[3] <= 2e-5, e


@pytest.mark.parametrize("mode", [0, 1])
def test_cls_scalar_losses_reject_more_than_1024_samples(mode):
    from muscle_amd._lib import MuscleHipError, call, ptr, stream
    x, y = torch.full((1025, 4), 0.5, device=DEV), torch.ones(1025, 4, device=DEV)
    loss, grad = torch.zeros(1, device=DEV), torch.full((1025, 4), SENT, device=DEV)
    with pytest.raises(MuscleHipError):
        call("mx_cls_loss", mode, ptr(x), 4, ptr(y), 4, ptr(loss), ptr(grad), 4, 1025, 4, stream())
    torch.cuda.synchronize()
    assert (grad == SENT).all()


@pytest.mark.parametrize("mode", [0, 1, 2, 3, 4])
def test_cls_loss_row_strides(mode):
    """ldx, ldy, ldg > C: rows of wider buffers; the same bits as the dense call, and the padding columns of grad untouched."""
    from muscle_amd._lib import call, ptr, stream
    N, C, ldx, ldy, ldg = 17, 65, 70, 67, 72
    logit, lab = _cls_inputs(N, C)
    x = torch.sigmoid(logit) if mode in (0, 2, 4) else logit              # probabilities for focal / pairwise / sigmoid-backward
    y = T(synth.normal(42, "cls.g", (N, C)).astype(np.float32)) if mode == 4 else lab

    def run(lx, ly, lg):
        bx, by = torch.full((N, lx), SENT, device=DEV), torch.full((N, ly), SENT, device=DEV)
        bx[:, :C], by[:, :C] = x.to(DEV), y.to(DEV)
        loss = torch.full((N,), SENT, device=DEV)
        grad = torch.full((N, lg), SENT, device=DEV)
        call("mx_cls_loss", mode, ptr(bx), lx, ptr(by), ly, ptr(loss) if mode < 3 else None, ptr(grad), lg, N, C, stream())
        torch.cuda.synchronize()
        return loss.cpu(), grad.cpu()

    (l0, g0), (l1, g1) = run(C, C, C), run(ldx, ldy, ldg)
    assert torch.equal(l0, l1) and torch.equal(g0, g1[:, :C])
    assert (g1[:, C:] == SENT).all() and not (g1[:, :C] == SENT).any()
    nl = {0: 1, 1: 1, 2: N}.get(mode, 0)
    assert not (l1[:nl] == SENT).any() and (l1[nl:] == SENT).all()
