"""Input path of MCL training (muscle_amd.data.InputStager) on its own: a batch of 32 from the fixture JPEGs of
tests/golden/input_views.npz with everything on the device (plan_item(device_jitter=True, device_resize=True)) - device time
of the stage (the pinned copy + mx_resample + mx_color_jitter x 2 + mx_input_stage x 3, HIP events around back-to-back calls)
and wall time per batch (host packing included), host time of plan_item on one core.  Not the contract bench.
  python tools/bench_mcl_input.py [--reps 30]"""
import io, os, sys, time, random
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import numpy as np, torch
torch.set_num_threads(1)
import PIL.Image
from muscle_amd import data as D

reps = int(sys.argv[sys.argv.index("--reps") + 1]) if "--reps" in sys.argv else 30
dev = torch.device("cuda:0")
N = 32
G = np.load(os.path.join(ROOT, "tests", "golden", "input_views.npz"))
ims = [PIL.Image.open(io.BytesIO(G[f"jpg{i}"].tobytes())).convert("RGB") for i in range(6)]
random.seed(0); torch.manual_seed(0)
t0 = time.perf_counter()
plans = [D.plan_item(ims[i % len(ims)], device_jitter=True, device_resize=True) for i in range(N)]
t_plan = (time.perf_counter() - t0) / N
print(f"plan_item: {t_plan*1e3:.2f} ms/item on one core (JPEG decode excluded), sources {sorted({im.size for im in ims})}")

stager = D.InputStager(dev, N)
for _ in range(3): batch = stager(plans)
torch.cuda.synchronize()
e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
t0 = time.perf_counter(); e0.record()
for _ in range(reps): batch = stager(plans)
e1.record(); torch.cuda.synchronize()
t_wall = (time.perf_counter() - t0) / reps
print(f"stage, batch {N} -> img [{N},3,448,448] + 2 views [{N},3,224,224]: {e0.elapsed_time(e1)/reps:.3f} ms/batch between HIP events "
      f"({reps} reps, back to back, copies included), {t_wall*1e3:.3f} ms/batch wall (host packing included), "
      f"{sum(p.img_u8.size + p.view1_u8.size + p.view2_u8.size for p in plans)/1e6:.1f} MB of uint8 images per batch")
