"""The device sampler of the BEACON boundary points on the GPU: mx_field_count, mx_field_sample and mx_field_terms_masked alone
against tests/field_sample_ref.py / dec_ref.py (each run twice for equal bits), edge.FieldLoss(sampler="device") and muscle_step
against the host criterion replaying the device-drawn points, the step without host synchronisation, and
muscle_amd.GraphedMuscleStep against eager steps."""
import contextlib

import numpy as np
import pytest
import torch

import dec_ref as R
import field_sample_ref as FS
import golden_util as gu
from dec_gpu_util import DEV, twice
from dec_ref import U
from muscle_amd import synth

pytestmark = pytest.mark.gpu

SEED = 20261021
BIG_SEED = 0xF00DFACE12345678          # above 2^63: crosses the C ABI as a negative long
NAN = float("nan")
T = lambda a: torch.from_numpy(np.asarray(a))   # noqa: E731


def _call(name, *args):
    from muscle_amd._lib import call, stream
    call(name, *args, stream())


def _p(t):
    from muscle_amd._lib import ptr
    return ptr(t)


def _signed(seed):
    return seed - 2 ** 64 if seed >= 2 ** 63 else seed


# ---- 1. mx_field_count --------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step", R.SELECT_STEPS)
@pytest.mark.parametrize("hw", R.SELECT_HW, ids=lambda c: "x".join(map(str, c)))
def test_field_count(hw, step):
    """All N*F slots in one launch equal dec_ref.field_select's counts exactly; the plane whose label is cleared counts {0,0,0}."""
    H, W = hw
    mag, orient, mx, _ = R.select_inputs(H, W)
    N, F = mag.shape[:2]
    lab = torch.ones(N, F)
    lab[1, 0] = 0.0
    d = mag.to(DEV), orient.to(DEV), mx.view(torch.int32).to(DEV), lab.to(DEV)

    def run():
        cnt = torch.full((N * F + 1, 3), -1, dtype=torch.int32, device=DEV)
        _call("mx_field_count", _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), step, _p(cnt), N, F, H, W)
        return cnt
    cnt = twice(run)
    slots = [(n, f) for n in range(N) for f in range(F)]
    want = R.field_select(mag.numpy(), orient.numpy(), mx.numpy(), slots, step, H, W)[2].copy()
    want[3] = 0
    assert cnt[:N * F].tolist() == want.tolist()
    assert cnt[N * F].tolist() == [-1, -1, -1], "the row after the counts was written"


# ---- 2. mx_field_sample -------------------------------------------------------------------------------------------------------
def _sample_gpu(mag, orient, mx, lab, step, k, seed, draw, H, W, calls=1):
    """[(counts, active, n_active, pts_out, pts_in, state)] of `calls` consecutive launches from counter value `draw`; the tables
    and the flags are allocated with canary rows behind them."""
    N, F = lab.shape
    S = N * F
    d = T(mag).to(DEV), T(orient).to(DEV), T(mx).view(torch.int32).to(DEV), T(lab).to(DEV)
    state = torch.tensor([draw, -1], dtype=torch.int64, device=DEV)
    out = []
    for _ in range(calls):
        cnt = torch.empty(S, 3, dtype=torch.int32, device=DEV)
        act = torch.full((S + 2,), -77, dtype=torch.int32, device=DEV)
        nact = torch.full((2,), -77, dtype=torch.int32, device=DEV)
        po, pi = (torch.full((S * k + 3, 2), -1234567, dtype=torch.int32, device=DEV) for _ in (0, 1))
        _call("mx_field_count", _p(d[0]), _p(d[1]), _p(d[2]), _p(d[3]), step, _p(cnt), N, F, H, W)
        _call("mx_field_sample", _p(d[0]), _p(d[1]), _p(d[2]), _p(cnt), step, k, _signed(seed), _p(state), _p(act), _p(nact), _p(po), _p(pi),
              N, F, H, W)
        out.append((cnt, act, nact, po, pi, state.clone()))
    return out


def _check_sample(got, ref, S, k, draw_after):
    cnt, act, nact, po, pi, state = (t.cpu() for t in got)
    assert cnt.tolist() == ref["counts"].tolist()
    assert act[:S].tolist() == ref["active"].tolist()
    assert int(nact[0]) == ref["n_active"]
    assert act[S:].tolist() == [-77, -77] and int(nact[1]) == -77, "a canary behind the flags was written"
    for tab, want in ((po, ref["pts_out"]), (pi, ref["pts_in"])):
        assert np.array_equal(tab[:S * k].numpy(), want)
        assert bool((tab[S * k:] == -1234567).all()), "a canary behind a point table was written"
    assert int(state[0]) == draw_after


@pytest.mark.parametrize("case", FS.SAMPLE_CASES, ids=lambda c: "x".join(map(str, c)))
def test_field_sample(case):
    """Flags, n_active and both point tables equal the restatement exactly (active slots: the k smallest keys in ascending source
    pixel; inactive ones: the filler rows); two launches in a row advance the counter by one each and draw different points."""
    H, W, k = case
    mag, orient, mx, lab = FS.sample_inputs(H, W)
    seed = BIG_SEED if k == 8 else SEED
    step = 7 if (H, W) == (40, 33) else 1

    def run():
        return tuple(t for call in _sample_gpu(mag, orient, mx, lab, step, k, seed, 5, H, W, calls=2) for t in call)
    flat = twice(run)
    first, second = flat[:6], flat[6:]
    S = lab.size
    r0, r1 = (FS.sample(mag, orient, mx, lab, step, k, seed, dr, H, W) for dr in (5, 6))
    _check_sample(first, r0, S, k, 6)
    _check_sample(second, r1, S, k, 7)
    if (H, W) == (3, 3):
        assert r0["n_active"] == 0                              # 9 positives in total: nothing is active
    else:
        assert r0["n_active"] >= 1 and not np.array_equal(r0["pts_out"], r1["pts_out"])
        assert not torch.equal(first[3], second[3]) and not torch.equal(first[4], second[4])
    if k == 128:
        assert r0["counts"][5, 0] > 128 and r0["counts"][5, 1] > 128


@pytest.mark.parametrize("n_out,active", [(FS.EDGE_CASE[2], 0), (FS.EDGE_CASE[2] + 1, 1)], ids=["k", "k+1"])
def test_field_sample_active_edge(n_out, active):
    """The all-positive plane shrunk (magnitudes zeroed) to n_out == k: inactive; to n_out == k + 1 with n_in > k: active."""
    H, W, k, step = FS.EDGE_CASE
    mag, orient, mx, lab = FS.sample_inputs(H, W)
    reached = FS.fit_plane(mag, orient, mx, 1, 2, step, H, W, n_out)
    assert reached[0] == n_out and reached[1] > k
    got = twice(lambda: _sample_gpu(mag, orient, mx, lab, step, k, SEED, 0, H, W)[0])
    ref = FS.sample(mag, orient, mx, lab, step, k, SEED, 0, H, W)
    assert ref["active"][5] == active and ref["counts"][5, 0] == n_out
    _check_sample(got, ref, lab.size, k, 1)


def test_field_sample_refuses_what_does_not_fit():
    from muscle_amd._lib import MuscleHipError
    x = torch.zeros(16, dtype=torch.int32, device=DEV)
    with pytest.raises(MuscleHipError):          # H*W = 2^32: refused before any launch
        _call("mx_field_sample", _p(x), _p(x), _p(x), _p(x), 1, 4, 0, _p(x.view(torch.int64)), _p(x), _p(x), _p(x), _p(x), 1, 1, 65536, 65536)
    with pytest.raises(MuscleHipError):
        _call("mx_field_count", _p(x), _p(x), _p(x), _p(x), 1, _p(x), 1, 1, 65536, 65536)


# ---- 3. mx_field_terms_masked -------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("S", R.TERMS_S)
@pytest.mark.parametrize("k", R.TERMS_K)
def test_field_terms_masked(k, S):
    """All slots active: mx_field_terms bit for bit.  Slots 1 and 4 of 5 inactive: exact zeros in their gsim and slot_loss, and
    loss[0] is what the unmasked entry gives on the active slots alone (0.75 to start with, in both)."""
    sim, simm = R.terms_inputs(k, S)
    d_sim, d_simm = sim.to(DEV), simm.to(DEV)

    def run(entry, a, b, flags, n):
        def fn():
            loss = torch.full((1,), 0.75, device=DEV)
            gsim, slot = torch.full((n, k, k), NAN, device=DEV), torch.full((n,), NAN, device=DEV)
            if flags is None:
                _call(entry, _p(a), _p(b), n, k, 0.5, _p(loss), _p(gsim), _p(slot))
            else:
                _call(entry, _p(a), _p(b), _p(flags), n, k, 0.5, _p(loss), _p(gsim), _p(slot))
            return loss, gsim, slot
        return twice(fn)
    plain = run("mx_field_terms", d_sim, d_simm, None, S)
    ones = torch.ones(S, dtype=torch.int32, device=DEV)
    for a, b in zip(plain, run("mx_field_terms_masked", d_sim, d_simm, ones, S)):
        assert torch.equal(a, b)
    if S < 5:
        return
    flags = torch.tensor([1, 0, 1, 1, 0], dtype=torch.int32)
    keep = flags.bool()
    poison = d_sim.clone()
    poison[~keep.to(DEV)] = NAN                       # the rows of an inactive slot are not read
    loss, gsim, slot = run("mx_field_terms_masked", poison, d_simm, flags.to(DEV), S)
    assert bool((gsim[~keep] == 0).all()) and bool((slot[~keep] == 0).all())
    sub = run("mx_field_terms", d_sim[keep.to(DEV)].contiguous(), d_simm[keep.to(DEV)].contiguous(), None, int(keep.sum()))
    assert torch.equal(loss, sub[0]) and torch.equal(gsim[keep], sub[1]) and torch.equal(slot[keep], sub[2])


# ---- 4-7: the criterion, the step, the graph ----------------------------------------------------------------------------------
def _fixture():
    G = gu.load("muscle_step_b3_beacon.npz")
    name = str(G["name"])
    n, size, seed, tseed, kk, step = (int(v) for v in G["meta"])
    return G, name, n, size, seed, kk, step


def _batch(n, size, seed):
    lab = synth.synth_labels(n, seed)
    return {"img": T(synth.normal(seed, "img", (n, 3, size, size)).astype(np.float32)).to(DEV), "label": T(lab).to(DEV),
            "mask": T(synth.synth_soft_mask(lab, size, seed)).to(DEV)}


def _model(name, seed):
    from test_gpu_decoder import build_dec
    return build_dec(name, seed)[2]


def _replay_of(crit, F):
    """(sample index, out pixels, in pixels) of the active slots of the criterion's latest device draw, in slot order."""
    ls = crit.last_sample
    act = ls["active"].cpu().bool()
    S, k = act.numel(), crit.k
    rb = (torch.arange(S) // F)[act]
    return rb, ls["pts_out"].cpu().view(S, k, 2)[act][:, :, 1], ls["pts_in"].cpu().view(S, k, 2)[act][:, :, 1]


_HEADS = {}


def _head_outputs(fused):
    """seg_map, the dense (or 1/8-resolution) features, mask and label_with_bg of the fixture's batch: one forward per mode."""
    if fused not in _HEADS:
        G, name, n, size, seed, kk, step = _fixture()
        model = _model(name, seed)
        b = _batch(n, size, seed)
        du = {int(i): T(u).to(DEV) for i, u in zip(G["drop_idx"], G["drop_u"])}
        model.train()
        with torch.no_grad():
            seg, ft = model(b["img"], cam="seg_p3" if fused else "seg", drop_u=du)
        lwb = torch.cat((torch.ones(n, 1, device=DEV), b["label"].float()), 1)
        _HEADS[fused] = (seg.detach().clone(), ft.detach().clone(), b["mask"], lwb)
    return _HEADS[fused]


@pytest.mark.parametrize("fused", [True, False], ids=["fused", "unfused"])
def test_device_sampler_equals_replay_of_its_points(fused):
    """FieldLoss(sampler="device") against FieldLoss(sampler="host") replaying the device-drawn points of the active slots, on the
    inputs of muscle_step_b3_beacon.npz.  Fused (ordered tile gather): loss and dense gradient equal (==): the inactive slots add
    zeros, the active points keep their order.  Unfused (float atomics in both runs): each result is within (m-1) roundings of
    the exact sum of its m terms, so |difference| <= 2 * m * U * sum |term| per element, m = the largest number of points on one
    pixel and sum |term| from the float64 restatement (dec_ref) - the rule of test_field_scatter_fullres_atomics."""
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    seg, ft, mask, lwb = _head_outputs(fused)
    F = seg.shape[1] - 1
    crit_d = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device", seed=SEED)
    fd = ft.clone().requires_grad_()
    loss_d, edge_d = crit_d(seg, fd, mask, lwb, step, dense_is_lowres_nhwc=fused)
    assert torch.is_tensor(loss_d) and loss_d.dim() == 0 and loss_d.is_cuda
    n_active = int(crit_d.last_sample["n_active"][0])
    print("active slots", n_active, "of", n * F, "counts of the active", crit_d.last_sample["counts"][crit_d.last_sample["active"].bool()].tolist())
    assert n_active >= 1, "no slot of the fixture is active at its k"
    assert crit_d.draws == 1
    loss_d.backward()
    crit_h = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="host")
    crit_h.replay_points = _replay_of(crit_d, F)
    fh = ft.clone().requires_grad_()
    loss_h, edge_h = crit_h(seg, fh, mask, lwb, step, dense_is_lowres_nhwc=fused)
    loss_h.backward()
    assert torch.equal(edge_d, edge_h)
    diff = (fd.grad.double() - fh.grad.double()).abs()
    print("loss", float(loss_d.detach()), float(loss_h.detach()), "largest gradient difference", float(diff.max()), "of", float(fh.grad.abs().max()))
    assert bool((loss_d == loss_h).all())
    assert float(fh.grad.abs().max()) > 0
    if fused:
        assert bool((fd.grad == fh.grad).all())
        return
    rb, rout, rin = crit_h.replay_points
    S, H, W = rb.numel(), seg.shape[2], seg.shape[3]
    pts = [torch.stack((rb.repeat_interleave(kk), t.reshape(-1).long()), 1) for t in (rout, rin)]
    m = int(torch.unique(pts[0][:, 0] * H * W + pts[0][:, 1], return_counts=True)[1].max())
    fo, mo = R.field_gather(ft.cpu(), 0, mask.cpu(), pts[0], 21, 24, H, W)
    fi, mi = R.field_gather(ft.cpu(), 0, mask.cpu(), pts[1], 21, 24, H, W)
    CH = fo.shape[1]
    sim = torch.bmm(fo.view(S, kk, CH), fi.view(S, kk, CH).transpose(1, 2))
    simm = torch.bmm(mo.view(S, kk, 24), mi.view(S, kk, 24).transpose(1, 2))
    gsim = R.field_terms(sim, simm, 1.0 / n)["gsim"]
    gfeat = torch.bmm(gsim, fi.view(S, kk, CH)).view(S * kk, CH)
    ref, mag = R.field_scatter(fo, gfeat, pts[0], 0, tuple(ft.shape), 1.0, H, W)
    tol = 2.0 * m * U * mag
    worst = float((diff.cpu() / tol.clamp_min(1e-300)).max())
    print("unfused: m =", m, "worst share of the tolerance", worst)
    assert bool((diff.cpu() <= tol).all()), worst
    assert gu.rel_err(fh.grad.cpu().flatten(), ref.float().flatten()) <= 1e-3      # the restatement is the same gradient


def test_device_sampler_without_active_slots_is_zero():
    """No labelled class: the loss is a 0-dim device tensor, exactly 0, with an all-zero gradient; any other sampler is refused."""
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    seg, ft, mask, lwb = _head_outputs(True)
    crit = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device", seed=1)
    f = ft.clone().requires_grad_()
    none = torch.cat((torch.ones(n, 1), torch.zeros(n, 20)), 1).to(DEV)
    loss, _ = crit(seg, f, mask, none, step, dense_is_lowres_nhwc=True)
    loss.backward()
    assert torch.is_tensor(loss) and loss.dim() == 0 and float(loss) == 0.0 and int(crit.last_sample["n_active"][0]) == 0
    assert bool((f.grad == 0).all())
    with pytest.raises(ValueError):
        M.edge.FieldLoss(sobel_size=5, k=kk, sampler="gpu")


def _params(model):
    return torch.cat([p.detach().reshape(-1) for p in model.parameters()]).clone()


@pytest.mark.both_arith
def test_muscle_step_device_sampler_equals_replay():
    """One muscle_step with the device sampler equals one step from the same start with the host criterion replaying those
    points: all parameters and the three returned scalars bit for bit."""
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    b = _batch(n, size, seed)
    du = {int(i): T(u).to(DEV) for i, u in zip(G["drop_idx"], G["drop_u"])}
    runs = []
    replay = None
    for sampler in ("device", "host"):
        model = _model(name, seed)
        opt = M.FusedAdam(model.parameters(), lr=float(G["lr"]), weight_decay=1e-5)
        crit = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler=sampler, seed=SEED)
        if sampler == "host":
            crit.replay_points = replay
        out = M.muscle_step(model, opt, b, lamb=float(G["lamb"]), step=step, k=kk, drop_u=du, fused=True, criterion2=crit)
        if sampler == "device":
            replay = _replay_of(crit, 20)
            assert replay[0].numel() >= 1
        runs.append((np.array([float(out[k]) for k in ("loss_seg", "loss_beacon", "grad_norm")], dtype=np.float32), _params(model)))
    assert np.array_equal(runs[0][0], runs[1][0]), (runs[0][0], runs[1][0])
    assert torch.equal(runs[0][1], runs[1][1]), float((runs[0][1].double() - runs[1][1].double()).abs().max())


@contextlib.contextmanager
def _no_sync():
    """torch.cuda.set_sync_debug_mode("error") where this build raises on a deliberate .item(); otherwise Tensor.cpu / .item /
    .tolist / .numpy raise for the duration."""
    probe = torch.ones(1, device=DEV)
    torch.cuda.synchronize()
    before = torch.cuda.get_sync_debug_mode()
    torch.cuda.set_sync_debug_mode("error")
    try:
        try:
            probe.item()
            flags = False
        except RuntimeError:
            flags = True
        if flags:
            yield "sync_debug_mode"
        else:
            torch.cuda.set_sync_debug_mode(before)
            saved = {name: getattr(torch.Tensor, name) for name in ("cpu", "item", "tolist", "numpy")}

            def refuse(name):
                def fn(self, *a, **kw):
                    if self.is_cuda:
                        raise RuntimeError(f"Tensor.{name} on a device tensor: a host synchronisation")
                    return saved[name](self, *a, **kw)
                return fn
            for name in saved:
                setattr(torch.Tensor, name, refuse(name))
            try:
                yield "patched"
            finally:
                for name, fn in saved.items():
                    setattr(torch.Tensor, name, fn)
    finally:
        torch.cuda.set_sync_debug_mode(before)


def test_muscle_step_device_sampler_does_not_synchronise():
    """After two ordinary steps - GraphedStep's warm-up: lazily created workspaces and the sampler's counter exist after the first,
    and the weight-transpose plan is rebuilt (its tables uploaded) in the second, once the optimizer's first step has moved the
    parameters into its arena - a step with the device sampler runs with host synchronisation made an error; the same guard
    does stop the host sampler's read-back."""
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    b = _batch(n, size, seed)
    model = _model(name, seed)
    opt = M.FusedAdam(model.parameters(), lr=float(G["lr"]), weight_decay=1e-5)
    crit = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device", seed=SEED)
    kw = dict(lamb=float(G["lamb"]), step=step, k=kk, fused=True)
    for _ in range(2):
        M.muscle_step(model, opt, b, criterion2=crit, **kw)
    torch.cuda.synchronize()
    with _no_sync() as how:
        out = M.muscle_step(model, opt, b, criterion2=crit, **kw)
    print("guard:", how)
    torch.cuda.synchronize()
    assert crit.draws == 3 and np.isfinite(float(out["loss_beacon"].detach()))
    host = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="host")
    with pytest.raises(RuntimeError):
        with _no_sync():
            M.muscle_step(model, opt, b, criterion2=host, **kw)
    torch.cuda.synchronize()


def test_graphed_muscle_step_equals_eager():
    """GraphedMuscleStep on the fixture's shapes - two eager warm-up steps, the capture, three replays on three different batches -
    against five eager device-sampler steps from the same start with the same seed and batches (the optimizer in device-scalar
    mode in both, as GraphedMuscleStep sets it): parameters and every returned scalar bit for bit; the replays draw different
    points."""
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    bs = [_batch(n, size, seed + i) for i in range(5)]
    kw = dict(lamb=float(G["lamb"]), step=step, k=kk)
    keys = ("loss_seg", "loss_beacon", "grad_norm")
    ref, gra = _model(name, seed), _model(name, seed)
    o_ref = M.FusedAdam(ref.parameters(), lr=float(G["lr"]), weight_decay=1e-5).use_device_scalars(True)
    o_gra = M.FusedAdam(gra.parameters(), lr=float(G["lr"]), weight_decay=1e-5)
    c_ref = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device", seed=SEED)
    c_gra = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device", seed=SEED)
    torch.manual_seed(99)
    want, want_pts = [], []
    for b in bs:
        o_ref.sync_lr()
        out = M.muscle_step(ref, o_ref, b, criterion2=c_ref, **kw)
        want.append([float(out[k]) for k in keys])
        want_pts.append(c_ref.last_sample["pts_out"].clone())
    torch.manual_seed(99)                       # same drop_connect draws: the graph takes its Philox offset at replay
    got, got_pts = [], []
    with M.GraphedMuscleStep(gra, o_gra, c_gra, warmup=2, **kw) as gstep:
        for b in bs:
            out = gstep(b)
            got.append([float(out[k]) for k in keys])
            got_pts.append(c_gra.last_sample["pts_out"].clone())
        assert gstep.replays == 3 and c_gra.draws == 5
        with pytest.raises(ValueError):
            gstep(_batch(n + 1, size, seed))
        with pytest.raises(ValueError):
            gstep(dict(bs[0], mask=torch.zeros(n, size, size, dtype=torch.uint8, device=DEV)))
    assert int(c_gra._state[0]) == 5 and int(c_ref._state[0]) == 5
    print("eager ", want)
    print("graph ", got)
    for i in range(5):
        assert torch.equal(want_pts[i], got_pts[i]), i
    assert not torch.equal(got_pts[2], got_pts[3]) and not torch.equal(got_pts[3], got_pts[4]) and not torch.equal(got_pts[2], got_pts[4])
    assert np.array_equal(np.array(want, dtype=np.float32), np.array(got, dtype=np.float32))
    assert torch.equal(_params(ref), _params(gra)), float((_params(ref).double() - _params(gra).double()).abs().max())
    sa, sb = o_ref.state_dict()["state"], o_gra.state_dict()["state"]
    assert {k: v["step"] for k, v in sa.items()} == {k: v["step"] for k, v in sb.items()}


def test_graphed_muscle_step_refusals():
    import muscle_amd as M
    G, name, n, size, seed, kk, step = _fixture()
    model = _model(name, seed)
    opt = M.FusedAdam(model.parameters(), lr=1e-4)
    dev_c = M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk, sampler="device")
    kw = dict(lamb=0.05, step=step, k=kk)
    with pytest.raises(ValueError):
        M.GraphedMuscleStep(model, opt, M.edge.FieldLoss(sobel_size=5, beta=1e2, k=kk), **kw)
    with pytest.raises(ValueError):
        M.GraphedMuscleStep(model, opt, dev_c, grad_hook=lambda m, p: None, **kw)
    with pytest.raises(ValueError):
        M.GraphedMuscleStep(model, opt, dev_c, energy=object(), **kw)
