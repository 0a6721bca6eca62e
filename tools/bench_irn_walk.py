"""Measure the IRN random walk both ways (one GPU, one process): indexing.propagate_to_edge(method="dense"), exp_times squarings
of the n x n transition matrix on the fp32 matrix pipe, against method="stencil", 2^exp_times matrix-free steps on an fp64 state.

  * geometry of a 375 x 500 VOC image at the IRN's 1/4 resolution: 94 x 125 (n = 11 750), radius 5, beta 8;
  * exp_times 6 (the script's default) and 8, C = 3 and C = 20 class maps;
  * outputs compared first; then dense and stencil alternate round by round, hipEvent timing, median [min..max];
  * peak device memory of both;
  * the stencil walk's time per step at n = 11 750 next to the same at 8 x 8 (one workgroup: what a launch costs), and the weights;
  * infer_irn per image with both methods.

    python tools/bench_irn_walk.py [--rounds 9] [--out profiles/irn_walk_bench.txt]

Without a GPU the file holds the work and byte counts only and names the commands still to be run.  Synthetic inputs.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

H, W, RADIUS, BETA = 94, 125, 5, 8
CONFIGS = [(6, 3), (6, 20), (8, 3), (8, 20)]                  # exp_times, C


def counts(n, nd, times, C):
    n4, C4 = (n + 3) // 4 * 4, (C + 3) // 4 * 4
    return {
        "dense_flop": 2.0 * n4 ** 3 * times + 2.0 * C4 * n4 * n4,
        "dense_bytes": 2 * 4 * n4 * n4 + 4 * n4 + 2 * 4 * C4 * n4,
        "stencil_flop": 2.0 * n * (2 * nd + 1) * C * 2 ** times,
        "stencil_bytes": 4 * nd * n + 8 * n + 2 * 8 * C * n + 4 * C * n,
    }


def count_lines(nd):
    n = H * W
    out = [f"work and memory, {H} x {W} (n = {n}), radius {RADIUS} ({nd} one-sided directions, {2 * nd + 1} non-zeros per column at most):",
           "  exp_times  C |   dense: GFLOP   buffers MB | stencil: steps   GFLOP   buffers MB | FLOP ratio"]
    for times, C in CONFIGS:
        c = counts(n, nd, times, C)
        out.append(f"  {times:9d} {C:2d} | {c['dense_flop'] / 1e9:14.0f} {c['dense_bytes'] / 1e6:12.1f} | {2 ** times:14d} {c['stencil_flop'] / 1e9:7.3f}"
                   f" {c['stencil_bytes'] / 1e6:12.2f} | {c['dense_flop'] / c['stencil_flop']:10.0f}")
    out.append("  dense buffers: the two n4 x n4 fp32 matrices, the column sums, the padded class maps in and out;")
    out.append("  stencil buffers: W fp32 [nd][n], cs fp64 [n], two fp64 [C][n] states, rw fp32 [C][n].")
    return out


def fmt(ts):
    ts = np.asarray(ts)
    return f"{np.median(ts):9.3f} [{ts.min():.3f}..{ts.max():.3f}] ms"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=9)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "irn_walk_bench.txt"))
    args = ap.parse_args()
    if args.rounds < 9:
        ap.error("--rounds must be at least 9")
    import torch
    from muscle_amd.indexing import search_paths
    nd = len(search_paths(RADIUS))
    lines = ["tools/bench_irn_walk.py - the IRN random walk, dense (matrix squarings) against stencil (matrix-free, csrc/irn_walk.hip)", ""]
    ok = True
    if not torch.cuda.is_available():
        lines += ["STATUS: NOT MEASURED.  No GPU was available where this file was written: no figure below is a measurement.  Run",
                  "", "    python tools/bench_irn_walk.py", "    python -m pytest tests/test_gpu_irn_walk.py -m gpu -s",
                  "", "on an MI355X; the first rewrites this file.", ""] + count_lines(nd)
    else:
        measured, ok = measure(torch, args.rounds, nd)
        lines += measured + [""] + count_lines(nd)
    text = "\n".join(lines) + "\n"
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(text)
    print(text, end="")
    return 0 if ok else 1


def measure(torch, rounds, nd):
    import muscle_amd
    from muscle_amd import indexing, ops, synth
    from muscle_amd.irn import infer_irn
    dev = torch.device("cuda:0")
    n = H * W

    def ev(fn):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        r = fn()
        b.record()
        b.synchronize()
        return a.elapsed_time(b), r

    def peak(fn):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        base = torch.cuda.memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        fn()
        torch.cuda.synchronize()
        return (torch.cuda.max_memory_allocated() - base) / 1e6

    edge = torch.from_numpy(synth.uniform(1, "walk_edge", (1, H, W)).astype(np.float32)).to(dev) ** 3
    out = [f"MEASURED on {torch.cuda.get_device_name(0)}, one process, {rounds} rounds, dense and stencil alternated round by round, hipEvent times,",
           f"median [min..max]; {H} x {W} (n = {n}), radius {RADIUS}, beta {BETA}; GEMM mode {muscle_amd.get_gemm_mode()}.", "",
           "propagate_to_edge (whole call: affinity / weights, walk, class maps):",
           "  exp_times  C | max |dense - stencil| / max | dense                          | stencil                        | dense min / stencil median | peak MB dense / stencil"]
    verdict = None
    for times, C in CONFIGS:
        x = torch.from_numpy(synth.uniform(2, f"walk_x{C}", (1, C, H, W)).astype(np.float32)).to(dev)
        run = {m: (lambda m=m: indexing.propagate_to_edge(x, edge, radius=RADIUS, beta=BETA, exp_times=times, method=m)) for m in ("dense", "stencil")}
        rd, rs = run["dense"](), run["stencil"]()                                     # warm-up and the comparison
        diff = float((rd - rs).abs().max()) / float(rd.abs().max())
        assert diff <= 2e-4, f"dense and stencil disagree: {diff}"
        ts = {"dense": [], "stencil": []}
        for _ in range(rounds):
            for m in ("dense", "stencil"):
                ts[m].append(ev(run[m])[0])
        pk = {m: peak(run[m]) for m in ("dense", "stencil")}
        ratio = min(ts["dense"]) / float(np.median(ts["stencil"]))
        out.append(f"  {times:9d} {C:2d} | {diff:29.2e} | {fmt(ts['dense'])} | {fmt(ts['stencil'])} | {ratio:26.1f} | {pk['dense']:.1f} / {pk['stencil']:.2f}")
        if (times, C) == (6, 20):
            verdict = float(np.median(ts["stencil"])) < min(ts["dense"])
    out += ["", f"acceptance (script defaults, exp_times 6, C = 20: stencil median below dense minimum): {'PASS' if verdict else 'FAIL'}", ""]

    table = indexing._path_table(RADIUS, dev)
    e2 = edge.reshape(H, W).contiguous()
    tw = [ev(lambda: ops.irn_walk_weights(e2, table, RADIUS, BETA))[0] for _ in range(rounds + 1)][1:]
    Wt, cs = ops.irn_walk_weights(e2, table, RADIUS, BETA)
    out.append(f"mx_irn_walk_weights (2 launches): {fmt(tw)}")
    out.append("mx_irn_walk, time per step = (call at 256 steps - call at 64 steps) / 192, one ctypes call each:")
    small_e = torch.zeros(8, 8, device=dev)
    Ws, css = ops.irn_walk_weights(small_e, table, RADIUS, BETA)
    for C in (3, 20):
        x = torch.rand(C, H, W, device=dev)
        xs = torch.rand(C, 8, 8, device=dev)
        per, per_s = [], []
        for r in range(rounds + 1):
            a = ev(lambda: ops.irn_walk(x, e2, Wt, cs, table, RADIUS, 64))[0]
            b = ev(lambda: ops.irn_walk(x, e2, Wt, cs, table, RADIUS, 256))[0]
            c = ev(lambda: ops.irn_walk(xs, small_e, Ws, css, table, RADIUS, 64))[0]
            d = ev(lambda: ops.irn_walk(xs, small_e, Ws, css, table, RADIUS, 256))[0]
            if r:
                per.append((b - a) / 192 * 1e3)
                per_s.append((d - c) / 192 * 1e3)
        c = counts(n, nd, 0, C)
        out.append(f"  C = {C:2d}: {np.median(per):7.2f} [{min(per):.2f}..{max(per):.2f}] us per step at n = {n} ({c['stencil_flop'] / np.median(per) / 1e3:.1f} GFLOP/s);"
                   f"  {np.median(per_s):6.2f} [{min(per_s):.2f}..{max(per_s):.2f}] us per step at 8 x 8, one workgroup per channel (the launch)")
    out.append("")

    Hi, Wi = 375, 500
    sd = synth.irn_state_dict(1)
    m = muscle_amd.EdgeDisplacement()
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=True)
    m = m.to(dev).eval()
    img = torch.from_numpy(synth.irn_image_pair(Hi, Wi, 1)).to(dev)
    cam = synth.irn_cam_dict(Hi, Wi, 1)
    run = {k: (lambda k=k: infer_irn(m, img, cam, method=k)) for k in ("dense", "stencil")}
    la, lb = run["dense"](), run["stencil"]()
    share = float((la != lb).float().mean())
    ts = {"dense": [], "stencil": []}
    for _ in range(rounds):
        for k in ("dense", "stencil"):
            ts[k].append(ev(run[k])[0])
    pk = {k: peak(run[k]) for k in ("dense", "stencil")}
    out.append(f"infer_irn per {Hi} x {Wi} image at the script's defaults (beta 8, exp_times 6), network + CAM stack upload + walk + label step, no file I/O:")
    out.append(f"  dense   {fmt(ts['dense'])}   peak {pk['dense']:.1f} MB")
    out.append(f"  stencil {fmt(ts['stencil'])}   peak {pk['stencil']:.1f} MB   label pixels differing from dense: {share:.2e}")
    out += host_work(rounds, Hi, Wi, cam, lb, float(np.median(ts["stencil"])))
    return out, bool(verdict)


def host_work(rounds, Hi, Wi, cam, label, device_ms):
    """What python -m muscle_amd.infer_irn does per image on the host around infer_irn(): wall clock, one thread, files in a
    temporary directory (page cache)."""
    import tempfile
    import time
    import PIL.Image
    from muscle_amd import synth
    from muscle_amd.infer import load_cam_dict, save_cam_dict
    from muscle_amd.irn import save_palette_png
    yy, xx = np.mgrid[0:Hi, 0:Wi]
    img = np.stack([(yy * 3 + xx) % 256, (yy + xx * 2) % 256, (yy * xx // 64) % 256], -1).astype(np.float64)
    img = np.clip(img * 0.5 + 128 * synth.uniform(3, "walk_jpeg", (Hi, Wi, 3)), 0, 255).astype(np.uint8)
    ts = {"JPEG decode": [], "np.load of the CAM dict": [], "label to host + PNG write": []}
    with tempfile.TemporaryDirectory() as d:
        PIL.Image.fromarray(img).save(os.path.join(d, "a.jpg"), quality=90)
        save_cam_dict(os.path.join(d, "a.npy"), cam)
        for _ in range(rounds + 1):
            t0 = time.perf_counter()
            PIL.Image.open(os.path.join(d, "a.jpg")).convert("RGB")
            t1 = time.perf_counter()
            load_cam_dict(os.path.join(d, "a.npy"))
            t2 = time.perf_counter()
            save_palette_png(os.path.join(d, "a.png"), label)
            t3 = time.perf_counter()
            for k, v in zip(ts, (t1 - t0, t2 - t1, t3 - t2)):
                ts[k].append(v * 1e3)
    out = ["", f"host work of the script per {Hi} x {Wi} image around infer_irn (wall clock, synthetic files, first round dropped):"]
    total = 0.0
    for k, v in ts.items():
        out.append(f"  {k:28s} {fmt(v[1:])}")
        total += float(np.median(v[1:]))
    out.append(f"  sum of medians {total:.2f} ms against {device_ms:.2f} ms for infer_irn(method=\"stencil\"): the host work is serial with it in the script")
    return out


if __name__ == "__main__":
    sys.exit(main())
