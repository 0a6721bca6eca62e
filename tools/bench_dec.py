"""BASELINE.json configs[3]: train_muscle.py loop body (decoder mode + BEACON FieldLoss), EfficientNet-B7 448x448 batch 16
per GPU, synthetic soft pseudo-labels.  Not the contract bench.

--sampler host|device: where BEACON's boundary points are drawn (edge.FieldLoss(sampler=...)); --graph 1: the step replayed as
a hipGraph (muscle_amd.GraphedMuscleStep, needs --sampler device).  --backbone / --batch / --steps / --rounds choose the
configuration; with --rounds R each lamb is timed R times in turn and every figure printed (profiles/beacon_sampler_bench.txt).
No option: the host sampler on B7 / batch 16, as before."""
import argparse, os, random, sys, time
sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np, torch
import muscle_amd
from muscle_amd import synth
ap = argparse.ArgumentParser()
ap.add_argument("--sampler", default="host", choices=("host", "device"))
ap.add_argument("--graph", default=0, type=int, choices=(0, 1))
ap.add_argument("--backbone", default="b7")
ap.add_argument("--batch", default=16, type=int)
ap.add_argument("--steps", default=4, type=int)
ap.add_argument("--rounds", default=1, type=int)
ap.add_argument("--lambs", default="0.05,0.0")
args = ap.parse_args()
if args.graph and args.sampler != "device":
    ap.error("--graph 1 needs --sampler device")
dev = torch.device("cuda:0")
N, S = args.batch, 448
torch.manual_seed(0)
random.seed(0)
model = muscle_amd.MuSCLe(21, "efficientnet-" + args.backbone, layers=3, last_pooling=True, mode="dec").to(dev)
opt = muscle_amd.FusedAdam(model.live_parameters("seg") if hasattr(model, "live_parameters") else model.parameters(), lr=1e-5, weight_decay=5e-5)
label = synth.synth_labels(N, 7)
batch = {"img": torch.from_numpy(synth.normal(7, "img", (N, 3, S, S)).astype(np.float32)).to(dev),
         "label": torch.from_numpy(label).to(dev),
         "mask": torch.from_numpy(synth.synth_soft_mask(label, S, 7)).to(dev)}
for lamb in (float(v) for v in args.lambs.split(",")):
    crit = muscle_amd.edge.FieldLoss(sobel_size=5, beta=1e2, k=128, sampler=args.sampler, seed=7)
    if args.graph:
        graphed = muscle_amd.GraphedMuscleStep(model, opt, crit, lamb=lamb, step=7, k=128)
        step = lambda: graphed(batch)                                   # noqa: E731
        warm = 4                                                        # two eager steps, the capture, one more replay
    else:
        step = lambda: muscle_amd.muscle_step(model, opt, batch, lamb=lamb, step=7, k=128, criterion2=crit)   # noqa: E731
        warm = 2
    for _ in range(warm): out = step()
    for _ in range(args.rounds):
        torch.cuda.synchronize(); t0 = time.perf_counter()
        for _ in range(args.steps): out = step()
        torch.cuda.synchronize(); dt = (time.perf_counter() - t0) / args.steps
        print(f"muscle_step {args.backbone.upper()} dec 448x448 bs{N} lamb={lamb} sampler={args.sampler} graph={args.graph}: {dt*1e3:7.1f} ms/step  {N/dt:6.1f} img/s  "
              f"loss_seg {float(out['loss_seg'].detach()):.4f} beacon {float(out['loss_beacon'].detach()) if torch.is_tensor(out['loss_beacon']) else out['loss_beacon']}  peak mem {torch.cuda.max_memory_allocated()/1e9:.1f} GB", flush=True)
    if args.graph:
        graphed.close()
