"""Measure training the IRN heads on the HIP path (one GPU, one process), at the training geometry: N = 32, crop 512 (128 x 128
features), PathIndex(radius=10): 152 destinations, 13 090 sources per sample.

  * the frozen backbone forward (EdgeDisplacement.stages), the loss head forward + backward (mx_irn_loss_fwd / _bwd), the
    whole forward + loss + backward (AffinityDisplacementLoss.loss_backward) and the whole step (irn_step with PolyOptimizer);
    the head forward + backward is the difference of the last-but-one and the first two;
  * for comparison, the same loss head and the same heads as torch ops with autograd on the same device, fed with the same stage
    outputs (tests/irn_train_ref.py moved to the GPU: what a user of the reference's classes would run);
  * peak device memory of both above the resident model and inputs;
  * the loss head's byte and FLOP floor.

    python tools/bench_irn_train.py [--reps 10] [--batch 32] [--crop 512]

Warm-up first, hipEvent timing, HIP and torch runs ALTERNATED in one process on one box, median and min-max reported.
"""
from __future__ import annotations

import argparse
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

HBM_TBS = 8.0


def once(fn):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    fn()
    b.record()
    b.synchronize()
    return a.elapsed_time(b)


def alternated(fns, reps, warmup=2):
    """{name: (median, min, max) ms}, the candidates run in turn `reps` times."""
    for _ in range(warmup):
        for f in fns.values():
            f()
    torch.cuda.synchronize()
    ts = {k: [] for k in fns}
    for _ in range(reps):
        for k, f in fns.items():
            ts[k].append(once(f))
    return {k: (float(np.median(v)), float(min(v)), float(max(v))) for k, v in ts.items()}


def peak_above(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    fn()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=32)
    ap.add_argument("--crop", type=int, default=512)
    ap.add_argument("--radius", type=int, default=10)
    args = ap.parse_args()
    import muscle_amd
    from muscle_amd import indexing, ops, synth
    import irn_net_ref as R
    import irn_train_ref as T
    dev = torch.device("cuda:0")
    N, S, radius = args.batch, args.crop, args.radius
    f = S // 4
    pi = indexing.PathIndex(radius, (f, f))
    nd, nsrc = len(pi.search_dst), len(pi.src_indices)
    npts = sum(g.shape[0] * g.shape[1] for g in pi.search_paths)
    print(f"# N {N} crop {S} features {f}x{f} radius {radius}: {nd} destinations, {nsrc} sources, {npts} path points; GEMM mode "
          f"{muscle_amd.get_gemm_mode()}; reps {args.reps}")
    sd = synth.irn_state_dict(1)
    m = muscle_amd.AffinityDisplacementLoss(pi, crop_size=S)
    m.load_state_dict({k: torch.from_numpy(np.asarray(v)) for k, v in sd.items()}, strict=False)
    m = m.to(dev).train()
    img = torch.from_numpy(np.concatenate([synth.irn_image_pair(S, S, s) for s in range(1, N // 2 + 1)])[:N]).to(dev)
    lab = torch.zeros(N, f, f, dtype=torch.uint8)
    lab[:, f // 8:f // 2, f // 6:f // 2] = 5
    lab[:, f // 3:3 * f // 4, f // 2:7 * f // 8] = 12
    lab[:, 5 * f // 6:, :f // 4] = 255
    lab = lab.to(dev)
    edge_p, dp_p = m.trainable_parameters()
    opt = muscle_amd.PolyOptimizer([{"params": edge_p, "lr": 0.01}, {"params": dp_p, "lr": 0.1}], lr=0.01, weight_decay=1e-4, max_step=10 ** 6)
    table = m._path_table(dev)
    with torch.no_grad():
        c = m._run(img)
    eo, do = c["eo"], c["do"]

    def hip_head():
        res, amax = ops.irn_loss_fwd(eo, do, lab, table, radius)
        ops.irn_loss_bwd(eo, do, lab, table, radius, amax, res)

    # the torch partner: heads + loss head with autograd, from the same (frozen) stage outputs
    xs = [t.permute(0, 3, 1, 2).contiguous() for t in m.stages(img)]
    sdt = R.to_dtype(sd, torch.float32, dev)
    keys = [k for grp in T.trainable_keys() for k in grp]
    for k in keys:
        sdt[k] = sdt[k].clone().requires_grad_(True)
    bg, fg, ng = (t.to(dev).float() for t in T.affinity_labels(lab.cpu().numpy(), radius))      # as floats: loss_head's .to() is then free
    orig_labels = T.affinity_labels
    T.affinity_labels = lambda _l, _r: (bg, fg, ng)                     # the reference's loader ships them; not timed
    orig_stages = R.stages
    R.stages = lambda _sd, _x: xs

    def torch_all():
        for k in keys:
            sdt[k].grad = None
        e, d = T.train_forward(sdt, img)
        T.loss_head(e, d, None, radius)["terms"]["total"].backward()

    e_t = eo[..., :1].permute(0, 3, 1, 2).contiguous()
    d_t = do[..., :2].permute(0, 3, 1, 2).contiguous()

    def torch_head():
        e, d = e_t.clone().requires_grad_(True), d_t.clone().requires_grad_(True)
        T.loss_head(e, d, None, radius)["terms"]["total"].backward()

    t = alternated({"stages": lambda: m.stages(img), "hip_head": hip_head, "torch_head": torch_head,
                    "hip_fwd_bwd": lambda: m.loss_backward(img, lab), "torch_heads_loss": torch_all,
                    "hip_step": lambda: muscle_amd.irn_step(m, opt, {"img": img, "label": lab})}, args.reps)
    fmt = lambda v: f"{v[0]:8.2f} ms ({v[1]:.2f}-{v[2]:.2f})"
    print(f"frozen backbone forward (stages)                 {fmt(t['stages'])}")
    print(f"loss head forward + backward, HIP                {fmt(t['hip_head'])}")
    print(f"loss head forward + backward, torch autograd     {fmt(t['torch_head'])}   -> HIP {t['torch_head'][0] / t['hip_head'][0]:.1f}x")
    print(f"forward + loss + backward, HIP (with the stages) {fmt(t['hip_fwd_bwd'])}")
    hb = t["hip_fwd_bwd"][0] - t["stages"][0]
    print(f"  heads + loss head alone (minus the stages)     {hb:8.2f} ms;  heads forward + backward (minus the loss head) "
          f"{hb - t['hip_head'][0]:.2f} ms")
    print(f"heads + loss head, torch autograd (no stages)    {fmt(t['torch_heads_loss'])}   -> HIP {t['torch_heads_loss'][0] / hb:.1f}x")
    print(f"whole step, HIP (irn_step, PolyOptimizer)        {fmt(t['hip_step'])}   {N / t['hip_step'][0] * 1e3:.0f} img/s")
    print(f"peak memory above the resident state: HIP loss head {peak_above(hip_head):.0f} MiB, torch loss head {peak_above(torch_head):.0f} MiB; "
          f"HIP forward + loss + backward {peak_above(lambda: m.loss_backward(img, lab)):.0f} MiB, torch heads + loss head "
          f"{peak_above(torch_all):.0f} MiB (without a backbone)")
    R.stages, T.affinity_labels = orig_stages, orig_labels
    # floors of the loss head
    pix, pairs = N * f * f, N * nd * nsrc
    byts = pix * (16 + 16 + 1) * 2 + pix * 32 + 2 * pairs          # E, D (4-column rows) and labels read by both passes; dE, dD; the byte map
    flops = N * nsrc * npts + N * f * f * npts                      # one compare per path point, forward and backward
    print(f"loss head floor: {byts / 2 ** 20:.0f} MiB of HBM traffic = {byts / (HBM_TBS * 1e12) * 1e6:.0f} us at {HBM_TBS} TB/s "
          f"(the byte map {pairs / 2 ** 20:.0f} MiB written and read once; six fp32 [N,n_dst(,2),n_src] tensors would be "
          f"{8 * 4 * pairs / 2 ** 20:.0f} MiB); {flops / 1e9:.2f} G path-point visits, {pairs / 1e6:.1f} M pairs x (1 exp + 1 log in fp64)")
    head_peak = peak_above(hip_head) * 2 ** 20
    assert head_peak < 4 * pairs, f"the HIP loss head holds {head_peak} bytes: an [N, n_dst, n_src] fp32 tensor would be {4 * pairs}"

if __name__ == "__main__":
    main()
