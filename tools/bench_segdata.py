"""Input path of decoder training (muscle_amd.segdata) next to the step it feeds: per batch of 16 at 448x448 from 375x500
sources over the scale range 0.5 .. 1.75 - device time of the stage (one pinned copy + mx_color_jitter + mx_resample +
mx_input_stage + mx_mask_stage, HIP events), bytes copied, host time of plan_seg_item and of the stager's packing on one
core, the muscle_step time of tools/bench_dec.py's configuration on the staged batch, and the per-item time of the scipy
restatement of the reference's label resize (tests/segdata_ref.py) on one core.  Not the contract bench.
  python tools/bench_segdata.py [--reps 30] [--no-step]
  python tools/bench_segdata.py --compact [--reps 30]
  python tools/bench_segdata.py --mask_type label [--reps 30] [--no-step]
--compact: the same 16 items (labels of three present classes from mx_irn_finish) staged from the dense float16 arrays and
from their compact form (muscle_amd/softlabel.py), alternating in one run: per form the bytes of the one copy and the
HIP-event time of the stage; the result is appended to profiles/segdata_bench.txt.  Nothing else is measured then.
--mask_type label: the same 16 items staged with their soft labels and with hard label maps (mask_type="label": uint8 rows,
mx_label_stage), alternating in one run: bytes of the one copy, size of the staged mask, HIP-event time of the stage and the B7
muscle_step on each staged batch; appended to the same file."""
import os, sys, time, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
import numpy as np, torch
torch.set_num_threads(1)
import muscle_amd
from muscle_amd import segdata as D, synth
import segdata_ref as R

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
dev = torch.device("cuda:0")
N, S, H, W = 16, 448, 375, 500
random.seed(0); torch.manual_seed(0)
ims = [R.synth_image(H, W, i) for i in range(N)]
masks = [R.synth_label(H, W, 100 + i) for i in range(N)]
scales = [0.5 + 1.25 * i / (N - 1) for i in range(N)]

def plan_all(masks=masks):
    return [D.plan_seg_item(ims[i], masks[i], scales[i], scales[i], S) for i in range(N)]


def compact_run():
    from muscle_amd import indexing
    h, w = (H + 3) // 4, (W + 3) // 4
    dense, compact = [], []
    for i in range(N):
        rw = torch.from_numpy(synth.uniform(200 + i, "rw", (20, 1, h, w)).astype(np.float32)) ** 2
        for c in range(20):
            if c not in ((i + 1) % 20, (i + 8) % 20, (i + 15) % 20):
                rw[c] *= 0.0
        dense.append(indexing.finish_semseg(rw.to(dev), H, W, 0.35, soft_output=True)[1].cpu().numpy())
        compact.append(indexing.finish_semseg(rw.to(dev), H, W, 0.35, soft_output="compact")[1])
    forms = {}
    for name, src in (("dense", dense), ("compact", compact)):
        random.seed(0); torch.manual_seed(0)
        forms[name] = (plan_all(src), D.SegStager(dev, N, S))
    out = {}
    for name, (plans, stager) in forms.items():
        for _ in range(3): out[name] = stager(plans)
    torch.cuda.synchronize()
    same = all(torch.equal(out["dense"][k], out["compact"][k]) for k in ("img", "mask"))
    ms = {name: 0.0 for name in forms}
    rounds, per = 6, max(1, reps // 6)
    for _ in range(rounds):                                   # alternating: both forms see the same clocks and the same neighbours
        for name, (plans, stager) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per): stager(plans)
            e1.record(); torch.cuda.synchronize()
            ms[name] += e0.elapsed_time(e1) / (rounds * per)
    lines = [f"tools/bench_segdata.py --compact: batch {N} at {S}x{S} from {H}x{W} labels of 3 present classes, scales {scales[0]:.2f} .. "
             f"{scales[-1]:.2f}, {rounds} x {per} reps per form, alternating; staged batches of the two forms bit-equal: {same}"]
    for name, (plans, stager) in forms.items():
        lines.append(f"  {name:7s}: {stager.last_bytes/1e6:8.2f} MB in the one copy, {ms[name]:.3f} ms/batch between HIP events "
                     f"(copy, mx_color_jitter, mx_resample, mx_input_stage" + (", mx_soft_expand" if name == "compact" else "") + ", mx_mask_stage)")
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "segdata_bench.txt"), "a") as f:
        f.write("\n" + "\n".join(lines) + "\n")


def label_run():
    """--mask_type label: the same 16 items with their soft labels (dense float16) and with hard label maps (the arg-max of the
    soft label as uint8), alternating in one run: bytes of the one copy, HIP-event time of the stage, and - unless --no-step -
    the B7 muscle_step on each staged batch."""
    maps = [m.astype(np.float32).argmax(2).astype(np.uint8) for m in masks]
    forms = {}
    for name in ("soft", "label"):
        random.seed(0); torch.manual_seed(0)
        plans = plan_all() if name == "soft" else [D.plan_label_item(ims[i], maps[i], scales[i], scales[i], S) for i in range(N)]
        forms[name] = (plans, D.SegStager(dev, N, S))
    label = torch.from_numpy(synth.synth_labels(N, 7))
    out = {}
    for name, (plans, stager) in forms.items():
        for _ in range(3): out[name] = stager(plans, labels=label)
    torch.cuda.synchronize()
    same = torch.equal(out["soft"]["img"], out["label"]["img"])
    ms = {name: 0.0 for name in forms}
    rounds, per = 6, max(1, reps // 6)
    for _ in range(rounds):                                   # alternating: both forms see the same clocks and the same neighbours
        for name, (plans, stager) in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(per): stager(plans, labels=label)
            e1.record(); torch.cuda.synchronize()
            ms[name] += e0.elapsed_time(e1) / (rounds * per)
    lines = [f"tools/bench_segdata.py --mask_type label: batch {N} at {S}x{S} from {H}x{W} sources, scales {scales[0]:.2f} .. {scales[-1]:.2f}, "
             f"{rounds} x {per} reps per form, alternating; staged images of the two forms bit-equal: {same}"]
    kern = {"soft": "mx_mask_stage", "label": "mx_label_stage"}
    for name, (plans, stager) in forms.items():
        m = out[name]["mask"]
        lines.append(f"  {name:5s}: {stager.last_bytes/1e6:8.2f} MB in the one copy, mask {tuple(m.shape)} {str(m.dtype).replace('torch.', '')} = "
                     f"{m.numel() * m.element_size()/1e6:.2f} MB, {ms[name]:.3f} ms/batch between HIP events "
                     f"(copy, mx_color_jitter, mx_resample, mx_input_stage, {kern[name]})")
    if "--no-step" in sys.argv:
        lines.append("  muscle_step: not measured (--no-step)")
    else:
        torch.manual_seed(0)
        model = muscle_amd.MuSCLe(21, "efficientnet-b7", layers=3, last_pooling=True, mode="dec").to(dev)
        opt = muscle_amd.FusedAdam(model.live_parameters("seg"), lr=1e-5, weight_decay=5e-5)
        for name in forms:
            for _ in range(3): res = muscle_amd.muscle_step(model, opt, out[name], lamb=0.05, step=7, k=128)
        dt, rounds, per = {name: 0.0 for name in forms}, 3, 3
        for _ in range(rounds):
            for name in forms:
                torch.cuda.synchronize(); t0 = time.perf_counter()
                for _ in range(per): res = muscle_amd.muscle_step(model, opt, out[name], lamb=0.05, step=7, k=128)
                torch.cuda.synchronize(); dt[name] += (time.perf_counter() - t0) / (rounds * per)
        for name in forms:
            lines.append(f"  {name:5s}: muscle_step B7 dec {S}x{S} bs{N} lamb=0.05 on the staged batch: {dt[name]*1e3:.1f} ms/step  "
                         f"{N/dt[name]:.1f} img/s ({rounds} x {per} steps per form, alternating)")
    print("\n".join(lines))
    with open(os.path.join(ROOT, "profiles", "segdata_bench.txt"), "a") as f:
        f.write("\n" + "\n".join(lines) + "\n")


if "--compact" in sys.argv:
    compact_run()
    sys.exit(0)
if "--mask_type" in sys.argv:
    if sys.argv[sys.argv.index("--mask_type") + 1] != "label":
        sys.exit("--mask_type label is the only leg of that name (the soft path is the default run)")
    label_run()
    sys.exit(0)

plans = plan_all()
t0 = time.perf_counter()
for _ in range(3): plans = plan_all()
t_plan = (time.perf_counter() - t0) / (3 * N)
print(f"plan_seg_item: {t_plan*1e3:.2f} ms/item on one core (JPEG decode and np.load excluded), scales {scales[0]:.2f} .. {scales[-1]:.2f}")

label = synth.synth_labels(N, 7)
stager = D.SegStager(dev, N, S)
for _ in range(3): batch = stager(plans, labels=torch.from_numpy(label))
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter(); e0.record()
for _ in range(reps): batch = stager(plans, labels=torch.from_numpy(label))
e1.record(); torch.cuda.synchronize()
t_wall = (time.perf_counter() - t0) / reps
print(f"stage, batch {N} -> img [{N},3,{S},{S}] + mask [{N},21,{S},{S}]: {e0.elapsed_time(e1)/reps:.3f} ms/batch between HIP events "
      f"({reps} reps, back to back, copy included), {t_wall*1e3:.3f} ms/batch wall (host packing included), "
      f"{stager.last_bytes/1e6:.1f} MB copied per batch ({sum(p.mask_src.nbytes for p in plans)/1e6:.1f} MB label rows of "
      f"{sum(m.nbytes for m in masks)/1e6:.1f} MB, {sum(p.img_u8.size for p in plans)/1e6:.1f} MB images)")
for s in (0.5, 1.0, 1.75):
    m = masks[0].astype(np.float64)
    t0 = time.perf_counter(); R.skresize_ref(m, round(H * s), round(W * s)); dt = time.perf_counter() - t0
    print(f"scipy restatement of skimage.transform.resize, {H}x{W}x21 float64 at scale {s}: {dt*1e3:.0f} ms/item on one core")

if "--no-step" not in sys.argv:
    torch.manual_seed(0)
    model = muscle_amd.MuSCLe(21, "efficientnet-b7", layers=3, last_pooling=True, mode="dec").to(dev)
    opt = muscle_amd.FusedAdam(model.live_parameters("seg"), lr=1e-5, weight_decay=5e-5)
    for _ in range(5): out = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128)
    torch.cuda.synchronize(); t0 = time.perf_counter()
    steps = 8
    for _ in range(steps): out = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128)
    torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / steps
    print(f"muscle_step B7 dec {S}x{S} bs{N} lamb=0.05 on the staged batch: {dt*1e3:.1f} ms/step  {N/dt:.1f} img/s  "
          f"loss_seg {float(out['loss_seg']):.4f}")
    # steps and stage interleaved, as the training loop runs them
    torch.cuda.synchronize(); t0 = time.perf_counter()
    for _ in range(steps):
        batch = stager(plans, labels=torch.from_numpy(label))
        out = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128)
    torch.cuda.synchronize(); dt2 = (time.perf_counter() - t0) / steps
    print(f"stage + muscle_step interleaved: {dt2*1e3:.1f} ms/iteration  {N/dt2:.1f} img/s")
    print(f"plan time x step rate: {t_plan*1e3:.2f} ms/item x {N/dt:.0f} img/s = {t_plan*N/dt:.2f} cores")
