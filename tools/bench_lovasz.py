"""Lovasz-softmax loss (muscle_amd.lovasz): cost at the decoder-training shape, N = 16, K = 21, 448 x 448, 15 % ignored pixels,
timed with device events.
  alone   forward + backward of the loss by itself, ms per call; beside it, alternating in the same process, the same loss
          written in torch ops on the GPU (softmax, sort, cumsum: what a user would write without the kernels).  The torch loss in
          float64 at this size is the full-size correctness check.  Also mx_lovasz_ws bytes and the bytes a digit pass moves.
  trace   a few forward + backward calls and nothing else: the program of a `rocprofv3 --kernel-trace --stats` run of its own
  parts   the cross entropy + BEACON part of today's step (forward and backward from the decoder's outputs), ms per call
  step    muscle_step on EfficientNet-B7 (train_muscle.py's loop body on label maps, lamb 0.05) with the loss off and on,
          alternated off / on / off / on in one process, ms per step.  The "off" rows are the step as it was before the loss.
Writes what it prints to --out as well.  Not the contract bench."""
import argparse
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
import numpy as np
import torch

import muscle_amd
from muscle_amd import edge, lovasz, synth
from muscle_amd._lib import lib

ap = argparse.ArgumentParser()
ap.add_argument("--part", default="all", choices=["all", "alone", "trace", "parts", "step"])
ap.add_argument("--reps", type=int, default=10)
ap.add_argument("--steps", type=int, default=20, help="timed muscle_steps per arm and round")
ap.add_argument("--rounds", type=int, default=3, help="alternation rounds")
ap.add_argument("--model", default="efficientnet-b7")
ap.add_argument("--batch", type=int, default=16)
ap.add_argument("--size", type=int, default=448)
ap.add_argument("--out", default=None, help="also write the lines to this file")
a = ap.parse_args()

assert torch.cuda.is_available(), "bench_lovasz needs the GPU"
dev = torch.device("cuda:0")
N, K, S = a.batch, 21, a.size
lines = []


def say(s):
    print(s, flush=True)
    lines.append(s)


def events(fn, reps):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    torch.cuda.synchronize()
    e0.record()
    for _ in range(reps):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) / reps


def torch_lovasz(seg, lab, dtype):
    """Berman's lovasz_softmax_flat (classes='present', one group) in torch ops; 255 ignored."""
    p = torch.softmax(seg.to(dtype), 1).permute(1, 0, 2, 3).reshape(K, -1)
    l = lab.reshape(-1)
    keep = l != 255
    p, l = p[:, keep], l[keep]
    losses = []
    for c in range(K):
        fg = (l == c).to(dtype)
        if fg.sum() == 0:
            continue
        es, perm = torch.sort((fg - p[c]).abs(), descending=True)
        fgs = fg[perm]
        G = fgs.sum()
        jac = 1.0 - (G - fgs.cumsum(0)) / (G + (1.0 - fgs).cumsum(0))
        losses.append(torch.dot(es, torch.cat([jac[:1], jac[1:] - jac[:-1]])))
    return torch.stack(losses).mean()


label = synth.synth_labels(N, 7)
hard = synth.synth_soft_mask(label, S, 7).argmax(1).astype(np.uint8)
hard[np.random.default_rng(7).random(hard.shape) < 0.15] = 255
mask = torch.from_numpy(hard).to(dev)
crit = muscle_amd.LovaszSoftmaxLoss()
say(f"Lovasz-softmax loss, N={N} K={K} {S}x{S}, classes present, one group, {float((mask == 255).float().mean()) * 100:.1f} % ignored")

if a.part in ("all", "alone", "trace"):
    gen = torch.Generator(dev).manual_seed(8)
    seg = (torch.randn(N, K, S, S, device=dev, generator=gen) * 2.5
           + 3.0 * torch.nn.functional.one_hot(mask.clamp(max=K - 1).long(), K).permute(0, 3, 1, 2)).requires_grad_(True)

    def ours():
        seg.grad = None
        loss = crit(seg, mask)
        loss.backward()
        return loss

    def theirs():
        seg.grad = None
        loss = torch_lovasz(seg, mask, torch.float32)
        loss.backward()
        return loss

    if a.part == "trace":
        for _ in range(3):
            ours()
        torch.cuda.synchronize()
        say("trace: 3 forward + backward calls")
    else:
        for _ in range(2):
            l_ours, l_theirs = ours().detach(), theirs().detach()
        ours()
        g_ours = seg.grad.clone()
        theirs()
        g_theirs = seg.grad.clone()
        with torch.no_grad():
            l64 = float(torch_lovasz(seg.detach(), mask, torch.float64))
        t = {"ours": [], "torch": []}
        for _ in range(a.rounds):
            t["ours"].append(events(ours, a.reps))
            t["torch"].append(events(theirs, max(1, a.reps // 3)))
        say("alone, forward + backward: kernels " + " / ".join(f"{x:.2f}" for x in t["ours"]) + " ms; torch ops (fp32) "
            + " / ".join(f"{x:.2f}" for x in t["torch"]) + " ms per call, alternating")
        say(f"loss at full size: kernels {float(l_ours):.9f}, torch float64 {l64:.9f} (difference {float(l_ours) - l64:+.2e}), "
            f"torch float32 {float(l_theirs):.9f} (difference {float(l_theirs) - l64:+.2e})")
        say(f"gradient against the torch fp32 gradient: max-abs difference {float((g_ours - g_theirs).abs().max()):.3e} of "
            f"max-abs {float(g_theirs.abs().max()):.3e}")
        P = N * S * S
        n = K * P
        nblk = -(-P // 4096)
        table = K * 256 * nblk * 4
        say(f"mx_lovasz_ws({K}, {P}) = {lib().mx_lovasz_ws(K, P) / 2 ** 20:.1f} MiB; err + flag + g beside it: {n * 9 / 2 ** 20:.1f} MiB")
        say(f"bytes per digit pass, {n / 1e6:.1f} M elements: first pass histogram {n * 5 / 1e6:.0f} MB read, scatter {n * 5 / 1e6:.0f} MB "
            f"read + {n * 8 / 1e6:.0f} MB written; later passes histogram {n * 4 / 1e6:.0f} MB read, scatter {n * 8 / 1e6:.0f} MB read + "
            f"{n * 8 / 1e6:.0f} MB written; the (digit, block) table is {table / 1e6:.1f} MB, written, scanned and read once per pass")

if a.part in ("all", "parts", "step"):
    torch.manual_seed(0)
    img = torch.from_numpy(synth.normal(7, "img", (N, 3, S, S)).astype(np.float32)).to(dev)
    model = muscle_amd.MuSCLe(21, a.model, layers=3, last_pooling=True, mode="dec").to(dev)
    opt = muscle_amd.FusedAdam(model.parameters(), lr=1e-5, weight_decay=5e-5)
    batch = {"img": img, "label": torch.from_numpy(label).to(dev), "mask": mask}

if a.part in ("all", "parts"):
    model.train()
    seg_map, ft = model(img, cam="seg_p3")
    seg_leaf, ft_leaf = seg_map.detach().requires_grad_(True), ft.detach().requires_grad_(True)
    lab_bg = torch.cat((torch.ones((N, 1), device=dev), batch["label"].float()), dim=1)
    field = edge.FieldLoss(sobel_size=5, beta=1e2, k=128)

    def ce_beacon():
        seg_leaf.grad = ft_leaf.grad = None
        l = edge.cross_entropy_label(seg_leaf, mask)
        l2, _ = field(seg_leaf, ft_leaf, mask, lab_bg, 7, dense_is_lowres_nhwc=True)
        if torch.is_tensor(l2):
            l = l + 0.05 * l2
        l.backward()

    def lov():
        seg_leaf.grad = None
        crit(seg_leaf, mask).backward()

    for _ in range(2):
        ce_beacon(), lov()
    t = {"ce": [], "lv": []}
    for _ in range(a.rounds):
        t["ce"].append(events(ce_beacon, a.reps))
        t["lv"].append(events(lov, a.reps))
    say(f"on the decoder's own seg_map, forward + backward: cross entropy + BEACON (host sampler) "
        + " / ".join(f"{x:.2f}" for x in t["ce"]) + " ms; Lovasz " + " / ".join(f"{x:.2f}" for x in t["lv"]) + " ms per call, alternating")
    del seg_map, ft, seg_leaf, ft_leaf

if a.part in ("all", "step"):
    arms = {"off": dict(), "on": dict(lovasz=crit, lovasz_weight=1.0)}
    out = {}
    for name, kw in arms.items():
        for _ in range(2):
            out[name] = muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128, **kw)
    ms = {"off": [], "on": []}
    for _ in range(a.rounds):
        for name, kw in arms.items():
            ms[name].append(events(lambda: out.__setitem__(name, muscle_amd.muscle_step(model, opt, batch, lamb=0.05, step=7, k=128, **kw)),
                                   a.steps))
    for name in arms:
        say(f"muscle_step {a.model} dec {S}x{S} bs{N} label maps lamb 0.05, lovasz {name}: " + " / ".join(f"{t:.2f}" for t in ms[name]) +
            f" ms per step ({a.steps} steps each), loss_seg {float(out[name]['loss_seg'].detach()):.4f}" +
            (f" loss_lovasz {float(out[name]['loss_lovasz'].detach()):.4f}" if "loss_lovasz" in out[name] else ""))
    off, on = min(ms["off"]), min(ms["on"])
    say(f"best of each arm: off {off:.2f} ms, on {on:.2f} ms: the loss costs {on - off:+.2f} ms per step ({(on / off - 1) * 100:+.2f} %)")

if a.out:
    with open(a.out, "a") as f:
        f.write("\n".join(lines) + "\n")
