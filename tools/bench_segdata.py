"""Input path of decoder training (muscle_amd.segdata) next to the step it feeds: per batch of 16 at 448x448 from 375x500
sources over the scale range 0.5 .. 1.75 - device time of the stage (one pinned copy + mx_color_jitter + mx_resample +
mx_input_stage + mx_mask_stage, HIP events), bytes copied, host time of plan_seg_item and of the stager's packing on one
core, the muscle_step time of tools/bench_dec.py's configuration on the staged batch, and the per-item time of the scipy
restatement of the reference's label resize (tests/segdata_ref.py) on one core.  Not the contract bench.
  python tools/bench_segdata.py [--reps 30] [--no-step]"""
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

def plan_all():
    return [D.plan_seg_item(ims[i], masks[i], scales[i], scales[i], S) for i in range(N)]

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
