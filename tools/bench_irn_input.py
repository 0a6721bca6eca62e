"""Input path of IRN training, host loader against device loader, at the script's defaults (batch 32, crop 512, rescale 0.5 .. 1.5)
on a synthetic tree of 375 x 500 JPEGs with label PNGs.  One process, the two loaders ALTERNATED:
  (a) what `train_irn --loader host` runs: DataLoader(VOC12AffinityDataset, num_workers, pin_memory) + .to(device), img/s;
  (b) what `train_irn --loader device` runs: IrnLoader(VOC12AffinityPlans, num_workers) (decode + plan in the workers, one
      pinned copy, mx_resample + mx_irn_input_stage), img/s;
  (c) the device half alone between HIP events: the whole stager call (packing excluded from device time, copy included), then
      mx_resample and mx_irn_input_stage each on their own, with the stage kernel's achieved GB/s against the bytes it stores;
  (d) bytes of the one copy per batch against the float32 batch the host loader ships;
  (e) with --step: irn_step on the staged batch, alone and interleaved with the stager.
Both loaders re-create their workers per epoch (as the script does), so an epoch's rate includes the start of the workers; the
rate after the first batch is printed beside it.  Not the contract bench.
  python tools/bench_irn_input.py [--images 512] [--workers 8] [--rounds 3] [--reps 20] [--step]"""
import argparse
import os
import random
import sys
import tempfile
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np
import torch

N, S, H, W = 32, 512, 375, 500


def make_tree(root, count):
    import PIL.Image
    import irn_input_ref as R
    os.makedirs(os.path.join(root, "JPEGImages"))
    os.makedirs(os.path.join(root, "ir_label"))
    names = [f"2007_{i:06d}" for i in range(count)]
    for i, nm in enumerate(names):
        PIL.Image.fromarray(R.synth_image(H, W, i % 64), "RGB").save(os.path.join(root, "JPEGImages", nm + ".jpg"), quality=90)
        PIL.Image.fromarray(R.synth_label(H, W, i % 64), "L").save(os.path.join(root, "ir_label", nm + ".png"))
    return names


def epoch(loader, dev):
    """(images, seconds for the whole epoch, seconds after the first batch arrived) - every batch ends on the device."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    t1, n = None, 0
    for pack in loader:
        img, lab = pack["img"].to(dev, non_blocking=True), pack["label"].to(dev, non_blocking=True)
        n += img.shape[0]
        if t1 is None:
            torch.cuda.synchronize()
            t1, first = time.perf_counter(), img.shape[0]
    torch.cuda.synchronize()
    t2 = time.perf_counter()
    return n, t2 - t0, (n - first) / max(t2 - t1, 1e-9)


def events(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return float(np.median(ts)), float(min(ts)), float(max(ts))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--images", type=int, default=512)
    ap.add_argument("--workers", type=int, default=8)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--step", action="store_true")
    args = ap.parse_args()
    if args.workers > 8:
        ap.error("--workers: at most 8")
    from torch.utils.data import DataLoader
    import muscle_amd
    from muscle_amd._lib import call, stream
    from muscle_amd.irndata import IrnLoader, IrnStager, VOC12AffinityPlans, plan_irn_item
    from muscle_amd.train_irn import VOC12AffinityDataset
    import irn_input_ref as R
    dev = torch.device("cuda:0")
    torch.zeros(1, device=dev)
    print(f"# batch {N}, crop {S}, {args.images} JPEGs of {H}x{W} + label PNGs, {args.workers} workers, rescale 0.5 .. 1.5; "
          f"{os.cpu_count()} CPUs visible, torch {torch.__version__}")
    with tempfile.TemporaryDirectory() as root:
        names = make_tree(root, args.images)
        lab_dir = os.path.join(root, "ir_label")
        host = DataLoader(VOC12AffinityDataset(names, root, lab_dir, S), batch_size=N, shuffle=True, num_workers=args.workers,
                          pin_memory=True, drop_last=True)
        devl = IrnLoader(VOC12AffinityPlans(names, root, lab_dir, S), N, dev, num_workers=args.workers, shuffle=True,
                         drop_last=True, persistent_workers=False)
        rates = {"host": [], "device": []}
        for r in range(args.rounds):
            for kind, loader in (("host", host), ("device", devl)):
                random.seed(r)
                torch.manual_seed(r)
                n, dt, tail = epoch(loader, dev)
                rates[kind].append((n / dt, tail))
                print(f"round {r} ({kind:6s}): {n} images in {dt:.3f} s = {n / dt:7.1f} img/s with the workers' start, "
                      f"{tail:7.1f} img/s after the first batch")
        for kind, label in (("host", "(a) host loader  "), ("device", "(b) device loader")):
            v = np.array(rates[kind])
            print(f"{label}: median {np.median(v[:, 0]):7.1f} img/s per epoch ({v[:, 0].min():.1f}-{v[:, 0].max():.1f}), "
                  f"{np.median(v[:, 1]):7.1f} img/s after the first batch ({v[:, 1].min():.1f}-{v[:, 1].max():.1f})")
        a, b = np.median(np.array(rates["host"]), 0), np.median(np.array(rates["device"]), 0)
        print(f"    device / host: {b[0] / a[0]:.2f}x per epoch, {b[1] / a[1]:.2f}x after the first batch")

    # ---- (c), (d): one batch of 32 with the scales spread over the range
    ims = [R.synth_image(H, W, i) for i in range(N)]
    labs = [R.synth_label(H, W, i) for i in range(N)]
    rng = random.Random(0)
    t0 = time.perf_counter()
    plans = [plan_irn_item(ims[i], labs[i], S, rng, rescale=(0.5 + i / (N - 1),) * 2) for i in range(N)]
    t_plan = (time.perf_counter() - t0) / N
    stager = IrnStager(dev, N, S)
    out = stager(plans)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(10):
        stager(plans, out=out)
    torch.cuda.synchronize()
    t_wall = (time.perf_counter() - t0) / 10
    whole = events(lambda: stager(plans, out=out), args.reps)
    o_jobs, o_rs, m, rs_px = stager.last_launch
    base, st = stager.buf.base, stream()
    rs = events(lambda: call("mx_resample", base, base + o_rs, base, base, base, m, rs_px, st), args.reps)
    stg = events(lambda: call("mx_irn_input_stage", base, base + o_jobs, base, out["img"].data_ptr(), out["label"].data_ptr(), N, S, st),
                 args.reps)
    stored = out["img"].numel() * 4 + out["label"].numel()
    fmt = lambda v: f"{v[0]:7.3f} ms ({v[1]:.3f}-{v[2]:.3f})"
    print(f"(c) plan_irn_item {t_plan * 1e3:.2f} ms/item on one core (decode excluded); stager call, batch {N}: "
          f"{t_wall * 1e3:.2f} ms wall back to back (packing + copy + kernels)")
    print(f"    copy + mx_resample + mx_irn_input_stage between HIP events  {fmt(whole)}")
    print(f"    mx_resample alone ({m} of {N} items rescaled)                  {fmt(rs)}")
    print(f"    mx_irn_input_stage alone                                     {fmt(stg)}   {stored / 1e6:.1f} MB stored = "
          f"{stored / stg[0] / 1e6:.0f} GB/s")
    f32 = N * 3 * S * S * 4 + N * (S // 4) ** 2
    print(f"(d) one copy of {stager.last_bytes / 1e6:.1f} MB per batch (uint8 images, labels, tables, jobs) against {f32 / 1e6:.1f} MB "
          f"of float32 samples the host loader ships = {f32 / stager.last_bytes:.1f}x fewer bytes")

    if args.step:
        from muscle_amd import indexing, synth
        pi = indexing.PathIndex(10, (S // 4, S // 4))
        model = muscle_amd.AffinityDisplacementLoss(pi, crop_size=S)
        model.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in synth.irn_state_dict(1).items()}, strict=False)
        model = model.to(dev).train()
        edge_p, dp_p = model.trainable_parameters()
        opt = muscle_amd.PolyOptimizer([{"params": edge_p, "lr": 0.01}, {"params": dp_p, "lr": 0.1}], lr=0.01, weight_decay=1e-4,
                                       max_step=10 ** 6)
        step = events(lambda: muscle_amd.irn_step(model, opt, out), 5)
        both = events(lambda: muscle_amd.irn_step(model, opt, stager(plans)), 5)
        print(f"(e) irn_step on the staged batch (GEMM mode {muscle_amd.get_gemm_mode()})  {fmt(step)}  {N / step[0] * 1e3:.0f} img/s; "
              f"stager + irn_step interleaved  {fmt(both)}  {N / both[0] * 1e3:.0f} img/s")
    else:
        print("(e) irn_step was not timed in this run (--step)")


if __name__ == "__main__":
    main()
