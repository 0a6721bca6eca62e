"""BEACON boundary loss — drop-in for `src.edge.FieldLoss` (src/edge.py:175-384) on the HIP kernels of csrc/dec.hip, plus
the cross entropy against the arg-max pseudo-label and the gradient clipping of the train_muscle.py loop body.

The reference walks (sample, class) pairs in Python, thresholds a Sobel edge map of softmax(beta * seg), samples k boundary
points on each side with `random.sample` and compares k x k similarity matrices of channel-softmaxed dense features and of
the class-softmaxed soft mask.  Here stages 1-2 (edges, ordered point lists), 3 (feature gather), 4 (similarity GEMMs on
MFMA), 5 (the eight FP/FN/TP/TN terms and their gradient) and 6 (softmax backward + scatter) are kernels; the host only
reads the per-class point counts back (the reference synchronises at the same places) and replays Python's `random`
in the reference's draw order, so a seeded run picks the same points.

FieldLoss(sampler="device") (ours) draws on the GPU instead: mx_field_count and mx_field_sample take the counts of
all N*F (sample, class) slots, their active flags and a keyed k-subset per active slot and side; every slot then goes through
stages 3-6 with mx_field_terms_masked zeroing the inactive ones.  Nothing is read back, so the step can be captured
(muscle_amd.GraphedMuscleStep).
"""
from __future__ import annotations

import random
from typing import Optional

import torch
from torch import nn

from . import ops
from ._lib import call, ptr, stream

_ML = 24
IGNORE_LABEL = 255          # the ignore value of a hard label map (mask_type="label")


class _FieldLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, dense, plan):
        dev = dense.device
        S, k, CH = plan["S"], plan["k"], plan["CH"]
        N, K, H, W = plan["seg_shape"]
        mode, h, w = plan["mode"], plan["h"], plan["w"]
        npts = S * k
        feat = torch.empty(2, npts, CH, dtype=torch.float32, device=dev)          # [out | in]
        mfeat = torch.empty(2, npts, _ML, dtype=torch.float32, device=dev)
        lmap = plan.get("label")                                                  # a hard label map [N,H,W] uint8, or None
        for side in (0, 1):
            call("mx_field_gather", ptr(dense), mode, h, w, ptr(plan["mask"]), ptr(plan["pts"][side]), npts, ptr(feat[side]),
                 ptr(mfeat[side]) if lmap is None else None, CH, K, _ML, H, W, stream())
            if lmap is not None:
                call("mx_field_mask_label", ptr(lmap), ptr(plan["pts"][side]), npts, ptr(mfeat[side]), K, _ML, H, W, IGNORE_LABEL,
                     stream())
        sim = torch.empty(S, k, k, dtype=torch.float32, device=dev)
        simm = torch.empty(S, k, k, dtype=torch.float32, device=dev)
        ops.bgemm(0, feat[0].view(S, k, CH), feat[1].view(S, k, CH), sim, k, k, CH)
        ops.bgemm(0, mfeat[0].view(S, k, _ML), mfeat[1].view(S, k, _ML), simm, k, k, _ML)
        loss = torch.zeros(1, dtype=torch.float32, device=dev)
        gsim = torch.empty_like(sim)
        slot_loss = torch.empty(S, dtype=torch.float32, device=dev)
        active = plan.get("active")                                               # the device sampler's flags [S] (all N*F slots)
        if active is None:
            call("mx_field_terms", ptr(sim), ptr(simm), S, k, 1.0 / N, ptr(loss), ptr(gsim), ptr(slot_loss), stream())
        else:
            call("mx_field_terms_masked", ptr(sim), ptr(simm), ptr(active), S, k, 1.0 / N, ptr(loss), ptr(gsim), ptr(slot_loss), stream())
        ctx.save_for_backward(feat, gsim)
        ctx.plan = plan
        ctx.dshape = dense.shape
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        feat, gsim = ctx.saved_tensors
        plan = ctx.plan
        S, k, CH = plan["S"], plan["k"], plan["CH"]
        N, K, H, W = plan["seg_shape"]
        dev = feat.device
        gfo = torch.empty(S, k, CH, dtype=torch.float32, device=dev)
        ops.bgemm(1, gsim, feat[1].view(S, k, CH), gfo, k, CH, k)                   # d sim / d outs = gsim @ ins
        gd = torch.zeros(ctx.dshape, dtype=torch.float32, device=dev)
        gup = g.contiguous().float().reshape(1)
        gpt = torch.empty(S * k, CH, dtype=torch.float32, device=dev) if plan["mode"] == 1 else None
        call("mx_field_scatter", ptr(feat[0]), ptr(gfo), ptr(plan["pts"][0]), S * k, plan["mode"], plan["h"], plan["w"], ptr(gup),
             ptr(gd), ptr(gpt), N, CH, H, W, stream())
        return gd, None


class FieldLoss(nn.Module):
    def __init__(self, num_classes=21, gaussian_size=7, k=100, guassian_sigma=None, sobel_size=5, beta=1e3, sampler="host", seed=0):
        """sampler: "host" (the reference's draws: counts read back, Python's `random.sample`) or "device" (ours: counts, the
        active slots and a keyed k-subset per slot and side all stay on the GPU - DESIGN.md 7a; nothing is read back, the loss
        is always a 0-dim device tensor, exactly 0 with an all-zero gradient when no slot is active).  seed: the device sampler's
        seed; its draw counter lives in device memory and advances once per forward (`draws` mirrors it on the host)."""
        super().__init__()
        if sampler not in ("host", "device"):
            raise ValueError(f"sampler must be 'host' or 'device' (got {sampler!r})")
        self.sampler, self.seed, self.draws = sampler, int(seed), 0
        self._state = None               # uint64 {draw counter, stream key of the latest draw}, on the device (int64 storage)
        self.last_sample = None          # device sampler: the latest {"counts", "active", "n_active", "pts_out", "pts_in"}
        if sobel_size != 5:
            raise NotImplementedError("the HIP path implements the 5x5 Sobel the reference trains with (train_muscle.py:163)")
        if k % 4 or k > 256:
            raise NotImplementedError("k must be a multiple of 4 and <= 256")
        self.num_fg_cls, self.k, self.beta = num_classes - 1, k, beta
        # (sample index [S], out pixels [S,k], in pixels [S,k]) to use INSTEAD of thresholding + random.sample: which pixels
        # pass the 0.8*max edge threshold hinges on fp32 round-off of softmax(100*seg), so parity tests replay the point
        # sets the reference drew (tests/golden/muscle_step_b3_beacon.npz) and compare the loss on identical points
        self.replay_points = None

    def forward(self, seg_map, dense_ft, mask, label_with_bg, step=7, dense_is_lowres_nhwc: bool = False):
        """Returns (loss, edge magnitude [N,H,W]); loss is a tensor, the int 0 when no class has more than k points on
        both sides, or False when fewer than 10 boundary pixels exist (edge.py:376-383).  With sampler="device" the loss is
        always a 0-dim device tensor (exactly 0 in those two cases) and `last_sample` holds the draw.
        dense_ft: [N,CH,H,W] as MuSCLe.forward(cam='seg') returns it, or — dense_is_lowres_nhwc — the decoder's
        1/8-resolution NHWC map, upsampled on the fly at the sampled points only.
        mask: the soft label [N,K,H,W], or a hard label map [N,H,W] uint8 (mask_type="label"): then the mask row of a sampled
        point is softmax(onehot(label)) - uniform 1/K at an ignored (255) point, what the soft path's zero padding gives - written
        by mx_field_mask_label; no float tensor of the label is made."""
        seg = seg_map.detach().contiguous().float()
        N, K, H, W = seg.shape
        if mask.dtype == torch.uint8:
            if tuple(mask.shape) != (N, H, W):
                raise ValueError(f"a label map must be [N,H,W] = {(N, H, W)} uint8 (got {tuple(mask.shape)})")
            mask_kw = dict(mask=None, label=mask.detach().contiguous())
        else:
            mask_kw = dict(mask=mask.detach().contiguous().float())
        dev = seg.device
        F_ = K - 1
        lab = label_with_bg[:, 1:].contiguous().float()
        HW = H * W
        prob = torch.empty(N, F_, HW, dtype=torch.float32, device=dev)
        mag = torch.empty(N, F_, HW, dtype=torch.float32, device=dev)
        orient = torch.empty(N, F_, HW, dtype=torch.uint8, device=dev)
        mx = torch.empty(N * F_, dtype=torch.int32, device=dev)
        edge_fg = torch.empty(N, H, W, dtype=torch.float32, device=dev)
        call("mx_field_edges", ptr(seg), ptr(lab), float(self.beta), ptr(prob), ptr(mag), ptr(orient), ptr(mx), ptr(edge_fg), N, K,
             H, W, stream())
        del prob
        if self.replay_points is not None:
            rb, rout, rin = (torch.as_tensor(t) for t in self.replay_points)
            k = self.k
            S = int(rb.shape[0])
            if S == 0:
                return 0, edge_fg
            assert tuple(rout.shape) == (S, k) and tuple(rin.shape) == (S, k)
            nt = rb.to(dev, torch.int32).repeat_interleave(k)
            pts = [torch.stack((nt, t.reshape(-1).to(dev, torch.int32)), dim=1).contiguous() for t in (rout, rin)]
            dense = dense_ft.contiguous().float()
            if dense_is_lowres_nhwc:
                mode, h, w, CH = 1, dense.shape[1], dense.shape[2], dense.shape[3]
            else:
                mode, h, w, CH = 0, 0, 0, dense.shape[1]
            plan = dict(S=S, k=k, CH=CH, seg_shape=(N, K, H, W), mode=mode, h=h, w=w, pts=pts, **mask_kw)
            return _FieldLossFn.apply(dense, plan), edge_fg
        if self.sampler == "device":
            k, S = self.k, N * F_
            if HW > 2 ** 31 - 1 or S * k > 2 ** 30 - 1:
                raise ValueError(f"the device sampler needs H*W < 2^31 and N*F*k < 2^30 (got {HW}, {S * k})")
            if self._state is None or self._state.device != dev:
                self._state = torch.zeros(2, dtype=torch.int64, device=dev)       # (filled by kernels: no host copy, no sync)
                self._state[0] += self.draws
            counts = torch.empty(S, 3, dtype=torch.int32, device=dev)
            active = torch.empty(S, dtype=torch.int32, device=dev)
            n_active = torch.empty(1, dtype=torch.int32, device=dev)
            pts = [torch.empty(S * k, 2, dtype=torch.int32, device=dev) for _ in (0, 1)]
            call("mx_field_count", ptr(mag), ptr(orient), ptr(mx), ptr(lab), int(step), ptr(counts), N, F_, H, W, stream())
            seed = self.seed & (2 ** 64 - 1)
            call("mx_field_sample", ptr(mag), ptr(orient), ptr(mx), ptr(counts), int(step), k, seed - 2 ** 64 if seed >= 2 ** 63 else seed,
                 ptr(self._state), ptr(active), ptr(n_active), ptr(pts[0]), ptr(pts[1]), N, F_, H, W, stream())
            self.draws += 1
            self.last_sample = dict(counts=counts, active=active, n_active=n_active, pts_out=pts[0], pts_in=pts[1])
            dense = dense_ft.contiguous().float()
            if dense_is_lowres_nhwc:
                mode, h, w, CH = 1, dense.shape[1], dense.shape[2], dense.shape[3]
            else:
                mode, h, w, CH = 0, 0, 0, dense.shape[1]
            plan = dict(S=S, k=k, CH=CH, seg_shape=(N, K, H, W), mode=mode, h=h, w=w, pts=pts, active=active, **mask_kw)
            return _FieldLossFn.apply(dense, plan), edge_fg
        lab_h = lab.cpu()
        slots = [(b, c) for b in range(N) for c in range(F_) if lab_h[b, c] != 0]
        if not slots:
            return False, edge_fg
        S0 = len(slots)
        slots_t = torch.tensor(slots, dtype=torch.int32, device=dev)
        out_list = torch.empty(S0, HW, dtype=torch.int32, device=dev)
        in_list = torch.empty(S0, HW, dtype=torch.int32, device=dev)
        counts = torch.empty(S0, 3, dtype=torch.int32, device=dev)
        call("mx_field_select", ptr(mag), ptr(orient), ptr(mx), ptr(slots_t), S0, int(step), ptr(out_list), ptr(in_list), ptr(counts),
             F_, H, W, stream())
        cnt = counts.cpu().tolist()                       # the reference synchronises here too (boolean indexing)
        if sum(c[2] for c in cnt) < 10:
            return False, edge_fg
        k = self.k
        sel_out, sel_in, ns = [], [], []
        for s, (b, c) in enumerate(slots):
            n_out, n_in = cnt[s][0], cnt[s][1]
            if n_in > k and n_out > k:
                r_out = random.sample(range(n_out), k)    # edge.py:298-299: outs first, then ins
                r_in = random.sample(range(n_in), k)
                sel_out += [s * HW + r for r in r_out]
                sel_in += [s * HW + r for r in r_in]
                ns += [b] * k
        if not ns:
            return 0, edge_fg
        S = len(ns) // k
        nt = torch.tensor(ns, dtype=torch.int32, device=dev)
        pts = []
        for lst, sel in ((out_list, sel_out), (in_list, sel_in)):
            pix = lst.view(-1)[torch.tensor(sel, dtype=torch.int64, device=dev)]
            pts.append(torch.stack((nt, pix), dim=1).contiguous())
        dense = dense_ft.contiguous().float()
        if dense_is_lowres_nhwc:
            mode, h, w, CH = 1, dense.shape[1], dense.shape[2], dense.shape[3]
        else:
            mode, h, w, CH = 0, 0, 0, dense.shape[1]
        plan = dict(S=S, k=k, CH=CH, seg_shape=(N, K, H, W), mode=mode, h=h, w=w, pts=pts, **mask_kw)
        return _FieldLossFn.apply(dense, plan), edge_fg


class _CEArgmax(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, mask):
        seg, mask = seg.contiguous().float(), mask.contiguous().float()
        N, K, H, W = seg.shape
        loss = torch.zeros(1, dtype=torch.float32, device=seg.device)
        ws = torch.empty(1, dtype=torch.int64, device=seg.device)
        call("mx_ce_argmax", ptr(seg), ptr(mask), None, ptr(loss), None, N, K, H * W, 0, ws.data_ptr(), 8, stream())
        ctx.save_for_backward(seg, mask)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        seg, mask = ctx.saved_tensors
        N, K, H, W = seg.shape
        out = torch.empty_like(seg)
        call("mx_ce_argmax", ptr(seg), ptr(mask), ptr(g.contiguous().float().reshape(1)), None, ptr(out), N, K, H * W, 1, None, 0, stream())
        return out, None


def cross_entropy_argmax(seg_map, soft_mask):
    """nn.CrossEntropyLoss()(seg_map, torch.argmax(soft_mask, dim=1)) (train_muscle.py:189-191) in one kernel."""
    return _CEArgmax.apply(seg_map, soft_mask)


class _CELabel(torch.autograd.Function):
    @staticmethod
    def forward(ctx, seg, label):
        seg, label = seg.contiguous().float(), label.contiguous()
        N, K, H, W = seg.shape
        if label.dtype != torch.uint8 or tuple(label.shape) != (N, H, W):
            raise ValueError(f"a label map must be [N,H,W] = {(N, H, W)} uint8 (got {label.dtype} {tuple(label.shape)})")
        loss = torch.zeros(1, dtype=torch.float32, device=seg.device)
        ws = torch.empty(2, dtype=torch.int64, device=seg.device)
        call("mx_ce_label", ptr(seg), ptr(label), IGNORE_LABEL, None, ptr(loss), None, N, K, H * W, 0, ws.data_ptr(), 16, stream())
        ctx.save_for_backward(seg, label)
        return loss[0]

    @staticmethod
    def backward(ctx, g):
        seg, label = ctx.saved_tensors
        N, K, H, W = seg.shape
        out = torch.empty_like(seg)
        ws = torch.empty(2, dtype=torch.int64, device=seg.device)
        call("mx_ce_label", ptr(seg), ptr(label), IGNORE_LABEL, ptr(g.contiguous().float().reshape(1)), None, ptr(out), N, K, H * W, 1,
             ws.data_ptr(), 16, stream())
        return out, None


def cross_entropy_label(seg_map, label):
    """F.cross_entropy(seg_map, label.long(), ignore_index=255) for a hard label map [N,H,W] uint8, in one kernel: the mean
    of log sum exp - seg[label] over the pixels whose label is not 255.  Where torch returns NaN - no valid pixel at all -
    the loss is 0 and the gradient all zeros, so a batch of pure padding leaves the weights alone."""
    return _CELabel.apply(seg_map, label)


def clip_grad_norm_(model, max_norm: float):
    """torch.nn.utils.clip_grad_norm_(model.parameters(), max_norm) on the model's flat gradient arena
    (train_muscle.py:202).  Returns the total norm as a 0-dim device tensor (no host synchronisation)."""
    check = getattr(model.last_grad_sink, "check_aliases", None)
    if check is not None:
        check(model)                     # a gradient outside the arena would silently escape the clip
    arena = model.last_grad_sink.arena
    sq = torch.empty(2048, dtype=torch.float64, device=arena.device)      # per-workgroup partial square sums
    norm = torch.empty(1, dtype=torch.float32, device=arena.device)
    call("mx_clip_grad_norm", ptr(arena), arena.numel(), float(max_norm), ptr(sq), ptr(norm), stream())
    return norm[0]
