"""The image-level contrast (IMC) kernels of muscle_amd/csrc/losses.hip alone - imc_gram_kernel + imc_grad_kernel (MFMA pair)
and imc_kernel (one-workgroup fallback), behind mx_imc - called directly so that the workspace, the output buffers and the
pointers are the test's own, against the float64 reference of tests/imc_ref.py.

  loss      |got - ref| <= 2e-5 |ref|
  gradient  max_i ( max_d |got - ref|_i / (max_d |ref_i| + 0.01 max |ref|) ) <= 5e-5      (imc_ref.row_err: per row)
  n_valid   exactly; with no valid row the loss and the whole gradient are exactly 0
  every call: workspace (the wrapper's N*D + 2*N*N + 4*N + 16 floats), gemb and out start as NaN, each followed by a 256-float
            tail that must keep its bits; the results must be finite; a second call must give the same bits

The two bounds are those of test_gpu_model.py::test_imc_mfma_vs_oracle, here against float64 and per row.  They are checked
against the error of the oracle's closed form evaluated in plain fp32 torch on the CPU ("fp32" below): a case whose fp32
figure exceeds a quarter of a bound would be held to 4 x that figure instead (bound()); no case needs it.

Inputs (imc_ref.py): labels repeat GROUPS with period 6, so identical sets recur at stride 3 and 6, up to 20 positives in a
row spread over all four column tiles, and every block of 16 anchor rows has valid rows (BLOCK_TABLE, asserted per case);
embeddings are 1.5 base[i % 6] + noise with rows negated, cosines from about -0.8 to 0.9.

Low-norm cases: rows 1 and 20 are zero and row 4 has norm 1e-8; their gradient is g / 1e-6, about 1e5 times the others, so
under the metric above the ordinary rows vanish.  Those cases are therefore also held to the same bound with the low-norm
rows left out of both the error and the scale ("rest").  Rows 1 and 4 are valid anchors with positives (asserted; with 7 rows
only row 1 is: row 4's next positive would be row 7, so low13x36 repeats the fallback case with 13 rows, where both are).

D = 1: the true gradient is 0 (a unit vector of one component cannot turn), and the reference's is rounding noise.  The
kernel's is held to 5e-5 of the two terms that cancel, max_i |dloss/de_i| / |x_i|.

Measured on an MI355X / in fp32 torch on the CPU (loss: relative; grad: the row metric).  The fp32 gradient figures move with
the host's CPU and BLAS (64x1024: 3.9e-6 on one host, 5.6e-6 on another); all seen stay below 1e-5, a fifth of the bound:

  case              valid  loss     fp32      grad     fp32      rest     fp32
  15x64                10  7.49e-08 7.49e-08  1.71e-06 3.17e-06
  16x64                11  1.42e-08 1.42e-08  1.66e-06 3.03e-06
  17x64                12  3.44e-08 3.44e-08  1.96e-06 1.33e-06
  33x64                28  2.40e-08 2.40e-08  2.03e-06 2.65e-06
  48x64                43  8.49e-08 1.43e-08  2.13e-06 3.52e-06
  49x64                44  1.58e-07 4.07e-08  2.88e-06 3.23e-06
  63x64                58  3.59e-08 5.71e-08  2.22e-06 3.40e-06
  64x64                59  6.07e-08 1.92e-08  4.19e-06 4.11e-06
  64x16                59  6.02e-10 6.02e-10  1.44e-06 2.19e-06
  17x16                12  7.66e-08 3.20e-08  1.69e-06 7.09e-07
  33x32                28  1.42e-08 1.42e-08  3.05e-06 4.06e-06
  17x48                12  5.92e-10 8.63e-08  8.29e-07 1.69e-06
  49x1008              44  7.55e-09 6.48e-08  4.39e-06 3.74e-06
  64x1024              59  1.74e-08 7.89e-08  5.22e-06 3.88e-06
  7x36                  2  2.86e-08 8.72e-08  2.92e-06 6.96e-07
  33x20                28  8.00e-08 8.00e-08  1.08e-06 9.47e-07
  64x1000              59  1.46e-07 5.07e-08  4.46e-06 4.99e-06
  5x1                   1  3.16e-08 3.16e-08  0.00e+00 0.00e+00
  L1                   31  6.65e-08 6.65e-08  2.60e-06 2.36e-06
  L32                  27  5.32e-08 1.05e-07  2.07e-06 2.73e-06      (L32, L33, L70: the values of 33x64 under labels whose
  L33                  27  5.32e-08 1.05e-07  2.08e-06 2.73e-06       last column decides pairs; without it 28 rows are valid)
  L70                  27  5.32e-08 1.05e-07  2.08e-06 2.73e-06
  low33x64             28  1.96e-10 9.16e-08  2.80e-07 1.85e-07  3.16e-06 2.38e-06
  low7x36               2  9.94e-08 9.94e-08  1.07e-07 9.18e-08  6.09e-06 9.47e-06
  low13x36              8  2.64e-08 2.64e-08  1.48e-07 2.11e-07  1.66e-06 1.71e-06
  33x64 misaligned     28  2.40e-08 2.40e-08  2.23e-06 2.65e-06
  AABC D=16             1  4.81e-08 6.32e-08  3.98e-07 2.51e-07
  AABC D=36             1  8.66e-08 1.25e-07  1.63e-07 2.53e-07
  two D=16              1  4.81e-08 6.32e-08  3.98e-07 2.51e-07
  two D=36              1  8.66e-08 1.25e-07  1.63e-07 2.53e-07

  no valid row (2x64; AAB, AAA', N1, alleq at D = 16 and 36): loss, n_valid and every gradient entry exactly 0
  worst: loss 1.6e-07 (fp32 1.3e-07) of 2e-5; gradient 5.2e-06 (fp32 about 5e-06) of 5e-5; rest 6.1e-06 (fp32 about 1e-05)
"""
import functools

import numpy as np
import pytest
import torch

import imc_ref as R
from oracle import mcl_oracle as O

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
SENT = -7.0
TAIL = 256
LOSS_TOL, GRAD_TOL = 2e-5, 5e-5
T = lambda a: torch.from_numpy(np.asarray(a))  # noqa: E731


def bound(base, e32):
    """The issue's rule: the project's bound, unless plain fp32 already uses more than a quarter of it."""
    return base if e32 <= base / 4 else 4 * e32


def ws_floats(n, d):
    return n * d + 2 * n * n + 4 * n + 16          # loss_multilabel._IMC.forward


def mfma_path(d, L, misalign=False):
    return d % 16 == 0 and L <= 32 and not misalign   # mx_imc's dispatch


# ---- cases -------------------------------------------------------------------------------------------------------------------
def _groups(n, d):
    return lambda: (R.imc_emb(n, d, seed=n + d), R.imc_labels(n, 20))


def _wide(L):
    return lambda: (R.imc_emb(33, 64, seed=97), R.last_column_labels(33, L))


def _low(n, d):
    return lambda: (R.low_norm(R.imc_emb(n, d, seed=n + d))[0], R.imc_labels(n, 20))


CASES = {f"{n}x{d}": _groups(n, d) for n, d in
         [(2, 64), (15, 64), (16, 64), (17, 64), (33, 64), (48, 64), (49, 64), (63, 64), (64, 64),            # MFMA, every block count
          (64, 16), (17, 16), (33, 32), (17, 48), (49, 1008), (64, 1024),                                     # nt = 1, 2, 3; 63, 64 tiles
          (7, 36), (33, 20), (64, 1000), (5, 1)]}                                                              # fallback: D % 16 != 0
CASES["L1"] = lambda: (R.imc_emb(33, 64, seed=1), (np.arange(33) % 2).astype(np.float32).reshape(33, 1))  # 0-rows: alike AND disjoint
# the values of 33x64 under labels whose P and G masks (and count of valid rows) depend on column L - 1 alone (asserted in case())
CASES["L32"] = _wide(32)           # column 31 fills lab_s
CASES["L33"] = _wide(33)           # first width of the fallback
CASES["L70"] = _wide(70)           # column 69: the only one in the second trip of the fallback's lane loop
LAST_COLUMN = {"L32": 31, "L33": 32, "L70": 64}
CASES["low33x64"] = _low(33, 64)
CASES["low7x36"] = _low(7, 36)     # with 7 rows, row 4 has no positive after it; row 1 does
CASES["low13x36"] = _low(13, 36)   # ... here rows 1 and 4 both have, on the fallback
FALLBACK = {"7x36", "33x20", "64x1000", "5x1", "L33", "L70", "low7x36", "low13x36"}


def fp32_restatement(emb, lab):
    """(loss, gradient) of the oracle's closed form in plain fp32 torch on the CPU."""
    x = T(emb).clone().requires_grad_()
    loss = O.image_level_contrast(x, T(lab))
    if not torch.is_tensor(loss):
        return 0.0, np.zeros_like(emb)
    loss.backward()
    return float(loss.detach()), x.grad.numpy()


@functools.lru_cache(maxsize=None)
def case(name):
    """Inputs, the float64 reference and the fp32-torch figures of a case (CPU only, computed once)."""
    emb, lab = CASES[name]()
    n, d = emb.shape
    assert mfma_path(d, lab.shape[1]) == (name not in FALLBACK)
    ref = R.imc_ref(emb, lab)
    if name in LAST_COLUMN:                          # a kernel blind to the last column(s) sees other pairs and another count
        P, G = R.pair_masks(lab)
        blind = R.imc_ref(emb, R.without_columns(lab, LAST_COLUMN[name]))
        P0, G0 = R.pair_masks(R.without_columns(lab, LAST_COLUMN[name]))
        assert (P != P0).any() and (G != G0).any() and blind.n_valid != ref.n_valid
        assert abs(blind.loss - ref.loss) > 100 * LOSS_TOL * ref.loss and R.valid_per_block(ref.valid)[1] > 0
    elif n in R.BLOCK_TABLE and name != "L1":
        assert R.valid_per_block(ref.valid) == R.BLOCK_TABLE[n], name            # anchors with positives in blocks 1..3
    l32, g32 = fp32_restatement(emb, lab)
    c = {"emb": emb, "lab": lab, "ref": ref, "l32": l32, "g32": g32, "low": []}
    if name.startswith("low"):
        c["low"] = R.low_norm(emb)[1]
        assert ref.vp[1] >= 1 and ref.valid[1] and (n <= 7 or (ref.vp[4] >= 1 and ref.valid[4]))    # anchors with positives
    return c


def errors(c, loss, grad):
    """(loss error, gradient error, gradient error over the rows of ordinary norm) against the float64 reference."""
    ref = c["ref"]
    el = abs(loss - ref.loss) / abs(ref.loss) if ref.loss else abs(loss)
    if c["emb"].shape[1] == 1:
        x = T(c["emb"]).double()
        e = (x / x.abs().clamp_min(1e-6)).requires_grad_()
        P, G = (T(m) for m in R.pair_masks(c["lab"]))
        s = torch.exp(e @ e.t() / 0.1)
        sp, sn = 1e-6 + (s * P).sum(1), 1e-6 + (s * G).sum(1)
        ((-torch.log(sp / (sp + sn))) * T(ref.valid)).sum().div(len(x)).backward()
        sc = float((e.grad.abs() / x.abs()).max())
        assert sc > 0 and np.abs(ref.grad).max() <= 1e-12 * sc
        return el, float(np.abs(grad).max()) / sc, None
    eg = R.row_err(grad, ref.grad) if ref.n_valid else float(np.abs(grad).max())
    rest = None
    if c["low"]:
        keep = np.setdiff1d(np.arange(len(grad)), c["low"])
        rest = R.row_err(grad[keep], ref.grad[keep])
    return el, eg, rest


def check(tag, c, got):
    ref = c["ref"]
    el, eg, er = errors(c, got["loss"], got["grad"])
    fl, fg, fr = errors(c, c["l32"], c["g32"])
    print(f"IMC_FIG {tag:<22} valid={ref.n_valid:<3} loss_err={el:.2e} fp32={fl:.2e}  grad_err={eg:.2e} fp32={fg:.2e}"
          + (f"  rest={er:.2e} fp32={fr:.2e}" if er is not None else ""))
    assert got["n_valid"] == ref.n_valid, (tag, got["n_valid"], ref.n_valid)
    if ref.n_valid == 0:
        assert got["loss"] == 0.0 and not got["grad"].any(), tag
        return
    assert el <= bound(LOSS_TOL, fl), (tag, el, fl)
    assert eg <= bound(GRAD_TOL, fg), (tag, eg, fg)
    if er is not None:
        assert er <= bound(GRAD_TOL, fr), (tag, er, fr)


# ---- the call ----------------------------------------------------------------------------------------------------------------
def _bits(t):
    return t.view(torch.int32)


def run_imc(emb, lab, misalign=False):
    """One direct mx_imc call on NaN-filled workspace and outputs; the tails must survive and the results be finite."""
    from muscle_amd._lib import call, ptr, stream
    n, d = emb.shape
    need = ws_floats(n, d)
    nan = float("nan")
    ws = torch.full((need + TAIL,), nan, device=DEV)
    gemb = torch.full((n * d + TAIL,), nan, device=DEV)
    out = torch.full((2 + TAIL,), nan, device=DEV)
    gemb[n * d:], out[2:] = SENT, SENT
    buf = torch.zeros(n * d + 4, device=DEV)
    off = 1 if misalign else 0
    e = buf[off:off + n * d]
    e.copy_(T(emb).reshape(-1))
    assert (e.data_ptr() % 16 != 0) == misalign and ws.data_ptr() % 16 == 0
    dl = T(lab).to(DEV)
    call("mx_imc", ptr(e), ptr(dl), n, d, lab.shape[1], ptr(out), ptr(gemb), ptr(ws), stream())
    torch.cuda.synchronize()
    assert torch.equal(_bits(ws[need:]), _bits(torch.full((TAIL,), nan, device=DEV))), "workspace tail"
    assert (gemb[n * d:] == SENT).all() and (out[2:] == SENT).all(), "output tails"
    o, g = out[:2].cpu(), gemb[:n * d].cpu().reshape(n, d)
    assert torch.isfinite(o).all() and torch.isfinite(g).all()
    return {"loss": float(o[0]), "n_valid": float(o[1]), "grad": g.numpy(), "bits": (_bits(o).clone(), _bits(g).clone())}


def run_twice(emb, lab, **kw):
    a, b = run_imc(emb, lab, **kw), run_imc(emb, lab, **kw)
    assert torch.equal(a["bits"][0], b["bits"][0]) and torch.equal(a["bits"][1], b["bits"][1]), "run to run"
    return a


# ---- tests -------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(CASES))
def test_imc_vs_float64(name):
    """Every shape, label width and low-norm case: both kernels, each block count, nt < 4, L = 32 / 33 / 70, D = 1000 / 1024."""
    c = case(name)
    check(name, c, run_twice(c["emb"], c["lab"]))


def test_imc_misaligned_emb_falls_back_and_agrees():
    """emb one float into its buffer: not 16-byte aligned, so the one-workgroup kernel runs on the values of the 33x64 case."""
    c = case("33x64")
    a, b = run_twice(c["emb"], c["lab"]), run_twice(c["emb"], c["lab"], misalign=True)
    check("33x64 aligned", c, a)
    check("33x64 misaligned", c, b)
    ref = c["ref"]
    fl, fg, _ = errors(c, c["l32"], c["g32"])
    assert abs(a["loss"] - b["loss"]) <= 2 * bound(LOSS_TOL, fl) * abs(ref.loss)
    rows = np.abs(ref.grad).max(1)
    assert (np.abs(a["grad"] - b["grad"]).max(1) <= 2 * bound(GRAD_TOL, fg) * (rows + 0.01 * rows.max())).all()
    # A heuristic, not a proof of dispatch: today the two kernels add in different orders, so equal bits would mean the same
    # kernel ran twice.  A change that makes the two paths bit-identical may drop this line.
    assert not np.array_equal(a["grad"], b["grad"])


@pytest.mark.parametrize("d", [16, 36])
@pytest.mark.parametrize("name", list(R.HAND))
def test_imc_validity_boundary(name, d):
    """vn == vp, vn == vp + 1, vn == 0 with positives, one row, all alike, 2 & 1 == 0 - on the MFMA pair and the fallback."""
    emb, lab, n_valid = R.hand_case(name, d)
    assert mfma_path(d, lab.shape[1]) == (d == 16)
    ref = R.imc_ref(emb, lab)
    assert ref.n_valid == n_valid
    l32, g32 = fp32_restatement(emb, lab)
    c = {"emb": emb, "lab": lab, "ref": ref, "l32": l32, "g32": g32, "low": []}
    got = run_twice(emb, lab)
    check(f"{name} D={d}", c, got)
    if n_valid == 0:
        assert got["loss"] == 0.0 and got["n_valid"] == 0.0 and np.isfinite(got["grad"]).all() and not got["grad"].any()


def test_imc_wrapper_returns_python_zero_when_all_labels_are_equal():
    import muscle_amd as M
    emb, lab, _ = R.hand_case("alleq", 16)
    got = M.image_level_contrast(T(emb).to(DEV), T(lab).to(DEV))
    assert type(got) is float and got == 0.0


def test_imc_upstream_gradient_and_info():
    import muscle_amd as M
    c = case("33x64")
    ref = c["ref"]
    x = T(c["emb"]).to(DEV).requires_grad_()
    loss, info = M.loss_multilabel.image_level_contrast_nosync(x, T(c["lab"]).to(DEV))
    (3.5 * loss).backward()
    info = info.cpu()
    assert torch.equal(_bits(info[0]), _bits(loss.detach().cpu())) and float(info[1]) == ref.n_valid
    assert abs(float(loss.detach()) - ref.loss) <= LOSS_TOL * abs(ref.loss)
    err = R.row_err(x.grad.cpu().numpy(), 3.5 * ref.grad)
    print(f"IMC_FIG upstream 3.5x          grad_err={err:.2e}")
    assert err <= GRAD_TOL, err
    want = run_imc(c["emb"], c["lab"])                          # ... and the wrapper's own workspace gives the direct call's bits
    assert np.array_equal(x.grad.cpu().numpy(), np.float32(3.5) * want["grad"])


@pytest.mark.parametrize("n,d,L", [(65, 64, 20), (4, 1040, 20), (4, 64, 0), (4, 0, 20)])
def test_imc_rejects(n, d, L):
    from muscle_amd._lib import MuscleHipError, call, ptr, stream
    emb = torch.ones(max(n * d, 16), device=DEV)
    lab = torch.ones(max(n * L, 16), device=DEV)
    ws = torch.full((ws_floats(n, d),), SENT, device=DEV)
    gemb, out = torch.full((max(n * d, 16),), SENT, device=DEV), torch.full((2,), SENT, device=DEV)
    with pytest.raises(MuscleHipError):
        call("mx_imc", ptr(emb), ptr(lab), n, d, L, ptr(out), ptr(gemb), ptr(ws), stream())
    torch.cuda.synchronize()
    assert (gemb == SENT).all() and (out == SENT).all() and (ws == SENT).all()       # nothing was launched
