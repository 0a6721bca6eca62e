"""GPU parity of the matrix-free IRN random walk: indexing.propagate_to_edge(method="stencil") (csrc/irn_walk.hip).

Yardsticks: the reference's fixture tests/golden/irn_rw.npz (limit 2e-4 of the output maximum, as tests/test_gpu_irn.py has for
the dense path) and the dense oracle in fp64 (limit 2 e32 + 2e-7, e32 = the fp32 oracle's own error against the fp64 oracle on
the same input, computed here: the form of tests/test_gpu_irn_net.py).  The numpy restatement tests/irn_walk_ref.py is printed
next to the kernel's figure; tests/test_cpu_irn_walk.py pins it.  Every figure is printed before it is asserted.
"""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import irn_net_ref as R  # noqa: E402
import irn_walk_ref as WR  # noqa: E402

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
GOLD = os.path.join(os.path.dirname(__file__), "golden")


def rel(a, ref):
    a = a.detach().cpu().numpy() if torch.is_tensor(a) else a
    ref = np.asarray(ref, np.float64)
    return float(np.abs(np.asarray(a, np.float64) - ref).max()) / max(float(np.abs(ref).max()), 1e-30)


def stencil(x, edge, **kw):
    from muscle_amd import indexing
    return indexing.propagate_to_edge(torch.as_tensor(x).to(DEV), torch.as_tensor(edge).to(DEV), method="stencil", **kw)


def check_vs_oracle(name, x, edge, radius, beta, times, dense_too=False):
    """x [1,C,h,w], edge [1,h,w] fp32 CPU tensors: the stencil walk against the fp64 dense oracle under 2 e32 + 2e-7."""
    from oracle import mcl_oracle as O
    from muscle_amd import indexing
    r64 = O.irn_propagate_to_edge(x.double(), edge.double(), radius, beta, times).numpy()
    e32 = rel(O.irn_propagate_to_edge(x, edge, radius, beta, times), r64)
    rw = stencil(x, edge, radius=radius, beta=beta, exp_times=times)
    assert tuple(rw.shape) == r64.shape and rw.dtype == torch.float32
    e_st = rel(rw, r64)
    e_np = rel(WR.walk(x.numpy(), edge.numpy(), radius, beta, times), r64)
    msg = f"[irn_walk] {name}: e_stencil {e_st:.3e}  restatement {e_np:.3e}  e32 {e32:.3e}  bound {2 * e32 + 2e-7:.3e}"
    if dense_too:
        e_dn = rel(indexing.propagate_to_edge(x.to(DEV), edge.to(DEV), radius=radius, beta=beta, exp_times=times), r64)
        msg += f"  dense HIP path {e_dn:.3e}"
    print(msg)
    assert e_st <= 2 * e32 + 2e-7, (name, e_st, e32)
    return rw


def synth_case(h, w, C, seed=7):
    from muscle_amd import synth
    x = torch.from_numpy(synth.uniform(seed, "irn_x", (1, C, h, w)).astype(np.float32))
    edge = torch.from_numpy(synth.uniform(seed, "irn_e", (1, h, w)).astype(np.float32)) ** 3
    return x, edge


# ---- 1. the reference's fixture -----------------------------------------------------------------------------------------
@pytest.mark.parametrize("tag", ["a", "b", "c"])
def test_stencil_vs_reference_fixture(tag):
    z = np.load(os.path.join(GOLD, "irn_rw.npz"))
    radius, beta, times = (int(v) for v in z[f"{tag}_params"])
    rw = stencil(z[f"{tag}_x"], z[f"{tag}_edge"], radius=radius, beta=beta, exp_times=times)
    ref = z[f"{tag}_rw"]
    assert tuple(rw.shape) == ref.shape
    e, e_np = rel(rw, ref), rel(WR.walk(z[f"{tag}_x"], z[f"{tag}_edge"], radius, beta, times), ref)
    print(f"[irn_walk] fixture {tag}: stencil {e:.3e}  restatement {e_np:.3e}  (limit 2e-4)")
    assert e <= 2e-4, (tag, e)


# ---- 2. / 5. n = 1395 (no multiple of 4 or 256), 256 steps; the same bits every run ---------------------------------------
def test_stencil_vs_fp64_oracle_31x45_and_deterministic():
    x, edge = synth_case(31, 45, 20)
    rw = check_vs_oracle("31x45 C=20 r=5 beta=10 exp_times=8", x, edge, 5, 10, 8, dense_too=True)
    again = stencil(x, edge, radius=5, beta=10, exp_times=8)
    assert torch.equal(rw, again)


# ---- 3. small and awkward shapes ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("h,w,C,radius,times", [(3, 7, 1, 5, 8), (1, 9, 2, 5, 8), (16, 12, 3, 3, 0)],
                         ids=["3x7-most-taps-outside", "1x9-one-row", "16x12-radius3-single-step"])
def test_stencil_small_shapes(h, w, C, radius, times):
    x, edge = synth_case(h, w, C, seed=11)
    check_vs_oracle(f"{h}x{w} C={C} r={radius} exp_times={times}", x, edge, radius, 10, times)


def test_stencil_with_exact_zero_and_one_edges():
    """9x22, C = 3, an edge map with exact 0.0 and exact 1.0 pixels, a corner among them: a pixel whose edge is 1.0 has no
    neighbours (weights 0, column sum 1) and a state of 0."""
    x, edge = synth_case(9, 22, 3, seed=13)
    edge[0, 0, 0] = 1.0
    edge[0, 8, 21] = 0.0
    edge[0, 4, 5:9] = 1.0
    edge[0, 2:6, 15] = 0.0
    edge[0, 0, 10] = 1.0
    rw = check_vs_oracle("9x22 C=3 with 0.0 / 1.0 edges", x, edge, 5, 10, 6)
    assert torch.isfinite(rw).all()
    assert float(rw[:, 0, 0, 0].abs().max()) == 0.0                    # an isolated vertex that starts at x * (1 - 1) = 0


# ---- 4. conservation ----------------------------------------------------------------------------------------------------
def test_stencil_conserves_an_all_ones_map():
    """T is column-stochastic and the state is fp64: only the final fp32 rounding remains."""
    one = stencil(torch.ones(1, 1, 31, 45), torch.zeros(1, 31, 45), exp_times=3)
    d = float((one - 1).abs().max())
    print(f"[irn_walk] all-ones map, edge 0, 8 steps: max |rw - 1| = {d:.3e}")
    assert d <= 1e-6


# ---- 6. the weights -----------------------------------------------------------------------------------------------------
def test_weights_equal_the_dense_paths_entries_bit_for_bit():
    """W of mx_irn_walk_weights against the matrix mx_irn_affinity builds, raised on the host by the same repeated multiplication,
    before normalisation: identical bits in every entry, zeros included (so no tap is misplaced and none is missing); cs within
    1e-6 relative of that matrix's fp64 column sums."""
    from muscle_amd import indexing, ops, synth
    from muscle_amd._lib import call, ptr, stream
    h, w, radius = 13, 17, 5
    n, n4 = h * w, (h * w + 3) // 4 * 4
    edge = torch.from_numpy(synth.uniform(5, "walk_e", (h, w)).astype(np.float32)) ** 3
    edge[3, 4] = 1.0
    edge[12, 16] = 0.0
    e = edge.to(DEV)
    table = indexing._path_table(radius, e.device)
    pc, off, ln, nd = table
    A = torch.empty(n4, n4, dtype=torch.float32, device=DEV)
    call("mx_irn_affinity", ptr(e), h, w, radius, ptr(pc), ptr(off), ptr(ln), nd, ptr(A), n4, n4, stream())
    aff = A.cpu().numpy()[:n, :n]
    for beta in (10, 8, 2.5):
        W, cs = ops.irn_walk_weights(e, table, radius, beta)
        assert tuple(W.shape) == (nd, n) and W.dtype == torch.float32 and cs.dtype == torch.float64
        Wh = W.cpu().numpy().reshape(nd, h, w)
        if beta == int(beta):
            scaled = WR.power_f32(aff, beta)
            mine = WR.dense_from_weights(Wh, radius)
            assert np.array_equal(mine.view(np.uint32), scaled.view(np.uint32)), beta
            Wn, _ = WR.walk_weights(edge.numpy(), radius, beta)
            assert np.array_equal(Wh.view(np.uint32), Wn.view(np.uint32)), beta
        else:                                                          # powf on the device: the pattern, and the values to fp32 round-off
            mine = WR.dense_from_weights(Wh, radius)
            scaled = aff.astype(np.float64) ** beta
            assert ((mine != 0) == (aff != 0)).all()
            assert float(np.abs(mine - scaled).max()) <= 4e-7
        sums = mine.astype(np.float64).sum(0)
        d = float(np.abs(cs.cpu().numpy() - sums).max() / sums.max())
        print(f"[irn_walk] weights 13x17 beta {beta}: {int((mine != 0).sum())} non-zeros, cs vs fp64 column sums {d:.2e}")
        assert float((np.abs(cs.cpu().numpy() - sums) / sums).max()) <= 1e-6


# ---- 7. infer_irn end to end ----------------------------------------------------------------------------------------------
def test_infer_irn_stencil_end_to_end():
    """infer_irn(method="stencil", soft_output=True) on the e2e case of irn_net.npz against the fixture and the fp64 restatement,
    under the caps test_infer_irn_end_to_end applies to the dense path: share of differing label pixels <= 2e-3, soft max
    difference <= 1e-3.  Checked on the CPU first: the reference's fixture against the fp64 restatement on this input has a label
    share of 0.0 and a soft max difference of 4.88e-4 (one fp16 ulp in [0.5, 1)), both inside the caps; the numpy restatement
    of the walk on the fp64 network's edge map has 0.0 / 1.53e-5 against the fp64 restatement and 0.0 / 4.88e-4 against the
    fixture."""
    import muscle_amd
    from muscle_amd import synth
    from muscle_amd.irn import infer_irn
    z = np.load(os.path.join(GOLD, "irn_net.npz"))
    crop, H, W, seed = (int(v) for v in z["a_params"])
    beta, times = (int(v) for v in z["e2e_params"])
    bg = float(z["e2e_bg_thres"])
    sd, x, cam = synth.irn_state_dict(seed), synth.irn_image_pair(H, W, seed), synth.irn_cam_dict(H, W, seed)
    m = muscle_amd.EdgeDisplacement(crop_size=crop)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(DEV).eval()
    label, soft = infer_irn(m, torch.from_numpy(x).to(DEV), cam, beta=beta, exp_times=times, bg_thres=bg, soft_output=True,
                            method="stencil")
    label, soft = label.cpu().numpy(), soft.cpu().numpy()
    assert label.dtype == np.uint8 and label.shape == (H, W) and soft.dtype == np.float16 and soft.shape == (H, W, 21)
    with torch.no_grad():
        lab64, soft64, _ = R.infer_irn(R.to_dtype(sd, torch.float64), torch.from_numpy(x).double(), cam, beta, times, bg, crop)
    for nm, lab_ref, soft_ref in (("fp64 restatement", lab64, soft64), ("fixture", z["e2e_label"], z["e2e_soft"])):
        diff = float((label != lab_ref).mean())
        sdiff = float(np.abs(soft.astype(np.float32) - soft_ref.astype(np.float32)).max())
        print(f"[irn_walk] infer_irn(stencil) vs {nm}: label share differing {diff:.3e}  soft max diff {sdiff:.3e}")
        assert diff <= 2e-3, (nm, diff)
        assert sdiff <= 1e-3, (nm, sdiff)


# ---- 8. the interface ---------------------------------------------------------------------------------------------------
def test_interface():
    from muscle_amd import indexing
    from muscle_amd.infer_irn import parse_args
    x, edge = (t.to(DEV) for t in synth_case(9, 14, 2))
    a = indexing.propagate_to_edge(x, edge, exp_times=3)
    b = indexing.propagate_to_edge(x, edge, exp_times=3, method="dense")
    assert torch.equal(a, b)
    with pytest.raises(ValueError, match="method"):
        indexing.propagate_to_edge(x, edge, method="sparse")
    with pytest.raises(ValueError, match="exp_times"):
        indexing.propagate_to_edge(x, edge, exp_times=13, method="stencil")
    assert tuple(indexing.propagate_to_edge(x, edge, exp_times=12, radius=2, method="stencil").shape) == (2, 1, 9, 14)
    assert parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "cams", "--walk", "stencil"]).walk == "stencil"
    assert parse_args(["--irn_weights_name", "w.pth", "--cam_dir", "cams"]).walk == "dense"
