"""The fused backward of the small project convs (ops.pw_proj_bwd_fused / mx_pw_proj_bwd_fused: dW += dp^T (swish(bn1(d_raw)) gate),
dA = dp Wp and the five SE / BN1 sums of se_bn1_pool from one pass over dp and d_raw) against float64, beside the unfused chain in
exact-fp32 arithmetic (pw_dgrad, pw_wgrad with the BNACT prologue, se_bn1_pool on the same inputs) under the project's rule
e_got <= 1.5 e_ref + 3e-7 scale - for the sums with scale = the largest sum of |terms| over (sample, channel), because they cancel;
dp and d_raw row views with a leading dimension larger than their width, dW pre-filled, guard rows and columns around dA, bit-identical
from run to run, dW bit for bit what pw_wgrad gives where the two kernels cut the rows into the same groups (below 131 072 rows), the
deferred reduce, and one B7 backward with the engine's switch on and off.

rows_per_sample is a multiple of 16 in every case: the kernel handles nothing else (include/muscle_hip.h)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
DEV = "cuda"
SENTINEL = -7.25
SHAPES = [(48, 288), (48, 192)]                      # the admitted (Cout, Cexp)
# one slab; four samples inside one workgroup (a flush every slab); 64-row groups that straddle sample boundaries; many groups with a
# shorter last one over seven samples
ROWS = [(16, 16), (64, 16), (192, 48), (4144, 592)]


def _inputs(R, rps, Co, Ce, seed):
    from muscle_amd.ops import BNState
    g = torch.Generator(device=DEV).manual_seed(seed)
    N = R // rps
    dp = torch.randn(R, Co + 8, device=DEV, generator=g)[:, :Co]
    x = torch.randn(R, Ce + 4, device=DEV, generator=g)[:, :Ce]
    scale = torch.rand(Ce, device=DEV, generator=g) + 0.5
    shift = torch.randn(Ce, device=DEV, generator=g) * 0.3
    gate = torch.sigmoid(torch.randn(N, Ce, device=DEV, generator=g))              # every sample its own gate row
    W = torch.randn(Co, Ce, device=DEV, generator=g) * (Co ** -0.5)
    dW0 = torch.randn(Co, Ce, device=DEV, generator=g)
    return dp, x, BNState(scale, shift, torch.zeros_like(scale), torch.ones_like(scale)), gate, W, dW0


def _fp64(dp, x, st, gate, rps, W, dW0):
    """(dA, dW, the five sums [5, N, Ce], the largest sum of |terms| of each of the five) in float64."""
    R, Ce = x.shape
    N = R // rps
    x64, d64 = x.double(), dp.double()
    z = st.scale.double() * x64 + st.shift.double()
    sg = torch.sigmoid(z)
    act, sp = z * sg, sg * (1 + z * (1 - sg))
    dA = d64 @ W.double()
    dW = dW0.double() + d64.t() @ (act * gate.double().repeat_interleave(rps, 0))
    terms = [dA * act, dA * sp, sp, dA * sp * x64, sp * x64]
    sums = torch.stack([t.view(N, rps, Ce).sum(1) for t in terms])
    scales = [float(t.abs().view(N, rps, Ce).sum(1).max()) for t in terms]
    return dA, dW, sums, scales


def _chain(dp, x, st, gate, rps, W, dW0):
    """The unfused chain in exact-fp32 arithmetic (GEMM mode 0): the yardstick."""
    import muscle_amd
    from muscle_amd import ops
    before = muscle_amd.get_gemm_mode()
    muscle_amd.set_gemm_mode(0)
    try:
        dpc, xc = dp.contiguous(), x.contiguous()
        dA = ops.pw_dgrad(dpc, W, x.shape[1])
        dW = dW0.clone()
        ops.pw_wgrad(dpc, xc, dW, x_mode=ops.BNACT, x_scale=st.scale, x_shift=st.shift, x_gate=gate, rows_per_sample=rps)
        pooled = ops.se_bn1_pool(dA, xc, st, rps)
    finally:
        muscle_amd.set_gemm_mode(before)
    return dA, dW, pooled


def _run(dp, x, st, gate, rps, W, dW0, **kw):
    from muscle_amd import ops
    R, Ce = x.shape
    buf = torch.full((R + 3, Ce + 12), SENTINEL, device=DEV)              # three guard rows and twelve guard columns of a sentinel
    dW = dW0.clone()
    dA, pooled = ops.pw_proj_bwd_fused(dp, x, st, gate, rps, W, dW, out=buf[:R, :Ce], **kw)
    assert dA.data_ptr() == buf.data_ptr() and tuple(pooled.shape) == (5, R // rps, Ce)
    return buf, dW, pooled


@pytest.mark.parametrize("R,rps", ROWS)
@pytest.mark.parametrize("Co,Ce", SHAPES)
def test_fused_backward_matches_fp64(Co, Ce, R, rps):
    args = _inputs(R, rps, Co, Ce, 1000 * Ce + R)
    assert R // rps >= 2 or R == 16
    want_dA, want_dW, want_sums, scales = _fp64(args[0], args[1], args[2], args[3], rps, args[4], args[5])
    ref_dA, ref_dW, ref_sums = _chain(args[0], args[1], args[2], args[3], rps, args[4], args[5])
    (buf, dW, pooled), (buf2, dW2, pooled2) = _run(args[0], args[1], args[2], args[3], rps, args[4], args[5]), \
        _run(args[0], args[1], args[2], args[3], rps, args[4], args[5])
    assert torch.equal(buf, buf2) and torch.equal(dW, dW2) and torch.equal(pooled, pooled2)       # two runs, equal bits
    assert bool((buf[R:] == SENTINEL).all()) and bool((buf[:, Ce:] == SENTINEL).all())            # nothing behind row R - 1 or beside the rows
    checks = [("dA", buf[:R, :Ce], ref_dA, want_dA, float(want_dA.abs().max())), ("dW", dW, ref_dW, want_dW, float(want_dW.abs().max()))]
    checks += [(f"sum{i}", pooled[i], ref_sums[i], want_sums[i], scales[i]) for i in range(5)]
    for name, got, ref, want, scale in checks:
        e_got, e_ref = float((got.double() - want).abs().max()), float((ref.double() - want).abs().max())
        print(f"{name} Co={Co} Ce={Ce} R={R} rps={rps}: e_got={e_got:.3e} e_ref={e_ref:.3e} scale={scale:.3e}")
        assert e_got <= 1.5 * e_ref + 3e-7 * scale, (name, e_got, e_ref, scale)


@pytest.mark.parametrize("Co,Ce", SHAPES)
def test_deferred_reduce_gives_the_same_bits(Co, Ce):
    from muscle_amd import ops
    args = _inputs(192, 48, Co, Ce, 7 + Ce)
    buf, dW, pooled = _run(args[0], args[1], args[2], args[3], 48, args[4], args[5])
    handed = []
    buf2, dW2, pooled2 = _run(args[0], args[1], args[2], args[3], 48, args[4], args[5], defer=lambda part, dw: handed.append((part, dw)))
    assert len(handed) == 1 and torch.equal(dW2, args[5])                 # the kernel left dW alone
    part, dw = handed[0]
    assert part.shape[1] == Co * Ce and dw.data_ptr() == dW2.data_ptr()
    ops.pw_parts_reduce(part, dw)
    assert torch.equal(buf, buf2) and torch.equal(dW, dW2) and torch.equal(pooled, pooled2)


@pytest.mark.parametrize("Co,Ce", SHAPES)
def test_weight_gradient_half_is_bit_identical_to_pw_wgrad(Co, Ce):
    """65 600 rows in four samples: the engine's query takes it, and the fused kernel, mx_pw_wgrad_small (BNACT) and its planner cut
    the rows into the same groups - same MFMAs in the same order, same partial matrices, same reduce."""
    from muscle_amd import ops, _lib
    R, rps = 65600, 16400
    L = _lib.lib()
    assert L.mx_pw_proj_bwd_fused_ok(R, Co, Ce, rps) == 1
    groups = L.mx_pw_proj_bwd_fused_groups(R, Co, Ce, rps)
    assert groups * Co * Ce * 4 == L.mx_pw_wgrad_small_ws(R, Co, Ce, ops.BNACT)
    dp, x, st, gate, W, dW0 = _inputs(R, rps, Co, Ce, Ce)
    dp, x = dp.contiguous(), x.contiguous()
    want = dW0.clone()
    ops.pw_wgrad(dp, x, want, x_mode=ops.BNACT, x_scale=st.scale, x_shift=st.shift, x_gate=gate, rows_per_sample=rps)
    got = dW0.clone()
    dA, pooled = ops.pw_proj_bwd_fused(dp, x, st, gate, rps, W, got)
    assert torch.equal(got, want)
    # the data gradient of a long reduction: the first row, a slab edge, a group edge, a sample edge and the last row against float64
    rows_per_wg = -(-R // groups)
    rows_per_wg += -rows_per_wg % 16
    assert -(-R // rows_per_wg) == groups
    idx = torch.tensor([0, 1, 15, 16, rows_per_wg - 1, rows_per_wg, rps - 1, rps, R - 17, R - 1], device=DEV)
    want_dA = dp[idx].double() @ W.double()
    # exact-fp32 chains of Cout products of magnitude <= |dp| |W|: 1.5e-7 sum |a b| bounds a k-ordered fp32 chain of this length
    bound = 1.5e-7 * float((dp[idx].double().abs() @ W.double().abs()).max()) + 1e-7 * float(want_dA.abs().max())
    assert float((dA[idx].double() - want_dA).abs().max()) <= bound
    # and the sums of these long samples against the unfused pass over the fused kernel's own dA
    ref = ops.se_bn1_pool(dA, x, st, rps)
    _, _, want_sums, scales = _fp64(dp, x, st, gate, rps, W, dW0)
    for i in range(5):
        e_got, e_ref = float((pooled[i].double() - want_sums[i]).abs().max()), float((ref[i].double() - want_sums[i]).abs().max())
        print(f"sum{i} Co={Co} Ce={Ce} R={R}: e_got={e_got:.3e} e_ref={e_ref:.3e} scale={scales[i]:.3e}")
        assert e_got <= 1.5 * e_ref + 3e-7 * scales[i], (i, e_got, e_ref, scales[i])


# ---- engine level: one B7 backward with the switch on and off ----------------------------------------------------------------------
def _early_grads(model):
    """The gradients of the parameters of blocks 0-10, concatenated."""
    out = []
    for k, p in model.named_parameters():
        parts = k.split(".")
        if "_blocks" in parts and int(parts[parts.index("_blocks") + 1]) <= 10:
            assert p.grad is not None, k
            out.append(p.grad.detach().reshape(-1).clone())
    assert out
    return torch.cat(out)


def test_engine_switch_on_and_off(monkeypatch):
    """MuSCLe(B7), batch 4, 512 x 512: stage 2 (blocks 4-10: 48 x 192 once, 48 x 288 six times) has 65 536 rows, the kernel's threshold.
    The on-vs-off difference of the early blocks' gradients, in relative norm, may be at most twice the difference between GEMM modes
    0 and 1 of the switch-off schedule on the same inputs (both are roundings the project accepts; two of them stacked)."""
    import golden_util as gu
    import muscle_amd
    from muscle_amd import engine, ops, synth
    from muscle_amd.arch import net_cfg
    name, n, size, seed = "efficientnet-b7", 4, 512, 23
    cfg = net_cfg(name, False)
    sd = synth.synth_state_dict(cfg, seed)
    model = muscle_amd.MuSCLe(21, name, layers=3, last_pooling=False)
    model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    model = model.to(DEV).train()
    g = torch.Generator(device=DEV).manual_seed(seed)
    x = torch.randn(n, 3, size, size, device=DEV, generator=g)
    du = {k: v.to(DEV) for k, v in gu.drop_draws(cfg, n, 5).items()}
    probes = None
    calls = []
    real = ops.pw_proj_bwd_fused

    def counted(dp, d_raw, *a, **kw):
        calls.append((dp.shape[0], dp.shape[1], d_raw.shape[1]))
        return real(dp, d_raw, *a, **kw)

    monkeypatch.setattr(ops, "pw_proj_bwd_fused", counted)

    def run(fused, mode):
        nonlocal probes
        monkeypatch.setattr(engine, "PW_PROJ_BWD_FUSED", fused)
        before = muscle_amd.get_gemm_mode()
        muscle_amd.set_gemm_mode(mode)
        try:
            model.zero_grad(set_to_none=True)
            got = model(x, cam="cam", drop_u=du)
            if probes is None:
                probes = [torch.randn(o.shape, device=DEV, generator=g) for o in got]
            sum((o * p).sum() for o, p in zip(got, probes)).backward()
            return _early_grads(model)
        finally:
            muscle_amd.set_gemm_mode(before)

    off = run(False, 1)
    assert not calls
    assert torch.equal(run(False, 1), off)                                   # the switch-off schedule, bit for bit from run to run
    on = run(True, 1)
    assert sorted(calls) == [(n * 128 * 128, 48, 192)] + [(n * 128 * 128, 48, 288)] * 6, calls
    calls.clear()
    off0 = run(False, 0)
    assert not calls
    den = float(off.double().norm())
    d_on, d_modes = float((on.double() - off.double()).norm()) / den, float((off0.double() - off.double()).norm()) / den
    print(f"blocks 0-10 gradient, relative norm: on vs off {d_on:.3e}, GEMM mode 0 vs 1 (switch off) {d_modes:.3e}")
    assert d_on <= 2 * d_modes, (d_on, d_modes)
