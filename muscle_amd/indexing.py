"""IRN random-walk propagation on the HIP path — src/indexing.py::propagate_to_edge as called by infer_irn.py:76.

The reference builds flat index tables for every search path (PathIndex), gathers the padded edge map with
index_select, max-pools along each path, assembles a sparse COO matrix on the CPU, densifies it, moves it to the GPU,
raises it to beta, normalises the columns and squares it exp_times times with torch.matmul.  Here one kernel writes the
dense symmetric affinity matrix directly from the edge map, one pass turns it into the column-stochastic matrix, and the
2^exp_times-step walk is exp_times fp32 MFMA GEMMs (`mx_bgemm`) ping-ponging between two buffers; the class maps are
propagated with one more GEMM.  For a VOC image at the IRN's 1/4 resolution (≈94x125 = 11.7k vertices) that is
8 x 2 x 11.7k^3 = 25.7 TFLOP per image, by far the dominant cost of infer_irn.py.

`method="stencil"` computes the same x . T^(2^exp_times) without the matrix: T has at most 2 nd + 1 non-zeros per column
(nd = 34 one-sided search directions at radius 5), so it is applied 2^exp_times times as a stencil on an fp64 state
(`mx_irn_walk_weights`, `mx_irn_walk`; DESIGN.md, "IRN random-walk propagation").  The dense path stays the default.

`propagate_to_edge_multi` is the stencil walk for several exp_times at the cost of the largest: the states at the smaller powers
of two are written on the way (`mx_irn_walk_snap`), each bit for bit what its own walk gives.  muscle_amd/irn_sweep.py builds on it.
"""
from __future__ import annotations

from typing import List, Tuple

import numpy as np
import torch

from . import ops
from ._lib import MuscleHipError, call, ptr, stream

_tables = {}


def search_paths(radius: int = 5) -> List[List[Tuple[int, int]]]:
    """PathIndex.get_search_paths_dst (indexing.py:13-47): the straight path (farthest pixel first) to every search
    destination, in the reference's order (grouped by path length, which fixes nothing observable in the dense matrix
    but is kept so the table can be compared with the reference's)."""
    dirs = [(0, x) for x in range(1, radius)]
    for y in range(1, radius):
        for x in range(-radius + 1, radius):
            if x * x + y * y < radius ** 2:
                dirs.append((y, x))
    by_len = {}
    for dy, dx in dirs:
        lsq = dy * dy + dx * dx
        coords = [(y, x) for y in range(min(0, dy), max(0, dy) + 1) for x in range(min(0, dx), max(0, dx) + 1)
                  if (dy * x - dx * y) ** 2 / lsq < 1]
        coords.sort(key=lambda c: -abs(c[0]) - abs(c[1]))
        by_len.setdefault(len(coords), []).append(coords)
    return [p for k in sorted(by_len) for p in by_len[k]]


def _path_table(radius: int, device):
    key = (radius, str(device))
    if key not in _tables:
        paths = search_paths(radius)
        pc = np.array([c for p in paths for c in p], np.int32).reshape(-1)
        ln = np.array([len(p) for p in paths], np.int32)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32)
        _tables[key] = tuple(torch.from_numpy(a).to(device) for a in (pc, off, ln)) + (len(paths),)
    return _tables[key]


WALK_METHODS = ("dense", "stencil")
_RW_KBLOCK = 128                                  # K block of the dense walk's final product (a multiple of 4)


def propagate_to_edge(x: torch.Tensor, edge: torch.Tensor, radius: int = 5, beta: float = 10, exp_times: int = 8,
                      method: str = "dense") -> torch.Tensor:
    """x: [..., C, h, w] class maps (any leading 1s), edge: [1,h,w] or [h,w] boundary probability, both CUDA.
    Returns rw [C,1,h,w] like the reference.  method="dense" squares the n x n transition matrix exp_times times as the
    reference does; method="stencil" applies it 2^exp_times times as a stencil (csrc/irn_walk.hip): O(nd * n) memory, fp64 state,
    0 <= exp_times <= 12."""
    if method not in WALK_METHODS:
        raise ValueError(f"propagate_to_edge: method must be one of {WALK_METHODS} (got {method!r})")
    if method == "stencil" and (int(exp_times) != exp_times or not 0 <= exp_times <= 12):
        raise ValueError(f"propagate_to_edge: the stencil walk takes exp_times 0..12, 2^exp_times steps (got {exp_times!r})")
    if not x.is_cuda or not edge.is_cuda:
        raise MuscleHipError("propagate_to_edge runs on the HIP kernels only")
    if method == "stencil":
        h, w = x.shape[-2:]
        e = edge.reshape(h, w).contiguous().float()
        table = _path_table(radius, x.device)
        W, cs = ops.irn_walk_weights(e, table, radius, beta)
        rw = ops.irn_walk(x.reshape(-1, h, w).contiguous().float(), e, W, cs, table, radius, 2 ** int(exp_times))
        return rw.reshape(-1, 1, h, w)
    h, w = x.shape[-2:]
    n = h * w
    n4 = (n + 3) // 4 * 4                         # GEMM operands need leading dimensions that are multiples of 4
    dev = x.device
    e = edge.reshape(h, w).contiguous().float()
    pc, off, ln, nd = _path_table(radius, dev)
    A = torch.empty(n4, n4, dtype=torch.float32, device=dev)
    B = torch.empty(n4, n4, dtype=torch.float32, device=dev)
    call("mx_irn_affinity", ptr(e), h, w, radius, ptr(pc), ptr(off), ptr(ln), nd, ptr(A), n4, n4, stream())
    colsum = torch.empty(n4, dtype=torch.float32, device=dev)
    call("mx_irn_transition", ptr(A), n4, n4, float(beta), ptr(colsum), stream())
    for _ in range(exp_times):                     # trans <- trans @ trans   (indexing.py:119-120)
        ops.bgemm(1, A.view(1, n4, n4), A.view(1, n4, n4), B.view(1, n4, n4), n4, n4, n4)
        A, B = B, A
    xm = (x.reshape(-1, h, w).float() * (1 - e)).reshape(-1, n)
    C = xm.shape[0]
    C4 = (C + 3) // 4 * 4
    xp = torch.zeros(C4, n4, dtype=torch.float32, device=dev)
    xp[:C, :n] = xm
    # The class maps are dense rows, so this product adds n non-zero terms per output where a squaring adds a few hundred: left
    # as one fp32 chain it is the least accurate step of the walk (tests/test_gpu_irn_dense.py: 1.7e-6 of the maximum after two
    # squarings, 4.6e-7 of it from the squarings).  K is therefore cut into blocks of _RW_KBLOCK vertices, one batch member each,
    # and the partial products are added: blocked summation, 0.1 % of the walk's work.
    kb, kt = n4 // _RW_KBLOCK, n4 % _RW_KBLOCK                # full blocks and the tail (a multiple of 4, as n4 is)
    part = torch.empty(kb + (1 if kt else 0), C4, n4, dtype=torch.float32, device=dev)
    if kb:
        call("mx_bgemm", 1, ptr(xp), ptr(A), ptr(part), C4, n4, _RW_KBLOCK, n4, n4, n4, _RW_KBLOCK, _RW_KBLOCK * n4, C4 * n4, kb, 0,
             stream())
    if kt:
        k0 = kb * _RW_KBLOCK
        call("mx_bgemm", 1, ptr(xp) + 4 * k0, ptr(A) + 4 * k0 * n4, ptr(part) + 4 * kb * C4 * n4, C4, n4, kt, n4, n4, n4, 0, 0, 0, 1, 0,
             stream())
    rw = part.sum(dim=0)
    return rw[:C, :n].reshape(C, 1, h, w)


def check_exp_times_list(exp_times_list) -> Tuple[int, ...]:
    """The exp_times of one multi-snapshot walk: integers in 0..12, strictly ascending (so no duplicates), at least one."""
    ets = tuple(exp_times_list)
    if not ets:
        raise ValueError("exp_times_list is empty")
    if any(isinstance(e, bool) or int(e) != e or not 0 <= e <= 12 for e in ets):
        raise ValueError(f"exp_times_list: the stencil walk takes integer exp_times 0..12, 2^exp_times steps (got {list(ets)})")
    if any(b <= a for a, b in zip(ets, ets[1:])):
        raise ValueError(f"exp_times_list must be strictly ascending, without duplicates (got {list(ets)})")
    return tuple(int(e) for e in ets)


def propagate_to_edge_multi(x: torch.Tensor, edge: torch.Tensor, radius: int = 5, beta: float = 10,
                            exp_times_list=(8,)) -> torch.Tensor:
    """propagate_to_edge(method="stencil") for several exp_times from ONE walk to the largest: the walk reaches 2^e steps
    through every smaller power of two, so the states of the smaller exp_times are snapshots on the way (mx_irn_walk_snap).
    Returns [E,C,1,h,w]; slice i equals propagate_to_edge(x, edge, radius, beta, exp_times_list[i], method="stencil") bit for
    bit.  Stencil only; exp_times_list: integers in 0..12, ascending, no duplicates (ValueError otherwise)."""
    ets = check_exp_times_list(exp_times_list)
    if not x.is_cuda or not edge.is_cuda:
        raise MuscleHipError("propagate_to_edge_multi runs on the HIP kernels only")
    h, w = x.shape[-2:]
    e = edge.reshape(h, w).contiguous().float()
    table = _path_table(radius, x.device)
    W, cs = ops.irn_walk_weights(e, table, radius, beta)
    rw = ops.irn_walk_snap(x.reshape(-1, h, w).contiguous().float(), e, W, cs, table, radius, [2 ** t for t in ets])
    return rw.reshape(len(ets), -1, 1, h, w)


def finish_semseg(rw: torch.Tensor, H: int, W: int, bg_thres: float, soft_output=False):
    """infer_irn.py:78-94: rw [C,1,h,w] -> uint8 label map [H,W] (argmax over [bg_thres, upsampled rw / max]); with
    soft_output also the fp16 [H,W,C+1] array the script saves.  soft_output="compact": (label, softlabel.CompactSoft) - the
    maps of the channels that hold a non-zero word, the maximum mx_irn_finish divided by (its max_scratch word) and the
    threshold, which `softlabel.expand` turns back into that array bit for bit.  An all-zero rw gives vmax = 0 (the dense
    array would be NaN): such a CompactSoft cannot be saved or expanded."""
    C, _, h, w = rw.shape
    r = rw.reshape(C, h, w).contiguous().float()
    compact = isinstance(soft_output, str)
    if compact and soft_output != "compact":
        raise ValueError(f"finish_semseg: soft_output must be False, True or 'compact' (got {soft_output!r})")
    label = torch.empty(H, W, dtype=torch.uint8, device=rw.device)
    soft = torch.empty(H, W, C + 1, dtype=torch.float16, device=rw.device) if soft_output and not compact else None
    scratch = torch.empty(1, dtype=torch.int32, device=rw.device)
    call("mx_irn_finish", ptr(r), C, h, w, H, W, float(bg_thres), ptr(scratch), ptr(label), ptr(soft), stream())
    if compact:
        from .softlabel import CompactSoft
        present = (r.view(torch.int32) != 0).reshape(C, -1).any(dim=1)          # by the bits: a map of -0 is not "absent"
        keys = torch.nonzero(present).reshape(-1)
        vmax = scratch.view(torch.float32).cpu().numpy()[0]
        return label, CompactSoft(keys.cpu().numpy(), r[keys].cpu().numpy(), (H, W), vmax, np.float32(bg_thres), C + 1)
    return (label, soft) if soft_output else label


class PathIndex:
    """src/indexing.py:5-74 for any integer radius and any (H, W): `search_paths` (arrays [n_paths, length, 2] grouped by path
    length), `search_dst` [n_dst, 2] as (dy, dx), and the flat index arrays `path_indices` / `src_indices` / `dst_indices` over the
    (H - rf) x (W - 2 rf) source window, rf = radius - 1.  The kernels use the offsets (`offsets_table`), the flat arrays exist for
    AffinityDisplacementLoss's `path_indices{i}` buffers, which a reference checkpoint carries."""

    def __init__(self, radius: int, default_size):
        self.radius = int(radius)
        self.radius_floor = int(np.ceil(radius) - 1)
        self.size = (int(default_size[0]), int(default_size[1]))
        paths = search_paths(self.radius)
        by_len = {}
        for p in paths:
            by_len.setdefault(len(p), []).append(p)
        self.search_paths = [np.asarray(by_len[k]) for k in sorted(by_len)]
        self.search_dst = np.concatenate([p[:, 0] for p in self.search_paths], axis=0)
        H, W = self.size
        rf = self.radius_floor
        ch, cw = H - rf, W - 2 * rf
        if ch <= 0 or cw <= 0:
            raise ValueError(f"PathIndex: a {H}x{W} map has no source window at radius {radius}")
        full = np.arange(H * W, dtype=np.int64).reshape(H, W)
        self.path_indices = [np.array([[full[dy:dy + ch, rf + dx:rf + dx + cw].reshape(-1) for dy, dx in p] for p in grp])
                             for grp in self.search_paths]
        self.src_indices = full[:ch, rf:rf + cw].reshape(-1)
        self.dst_indices = np.concatenate([p[:, 0] for p in self.path_indices], axis=0)

    def offsets_table(self, device):
        """(pts int32 [2 * points], poff int32 [n_dst], plen int32 [n_dst], n_dst) on the device, paths in search_dst's order."""
        flat = [p for grp in self.search_paths for p in grp]
        pc = np.array([c for p in flat for c in p], np.int32).reshape(-1, 2)
        rf = self.radius_floor
        if pc[:, 0].min() < 0 or pc[:, 0].max() > rf or np.abs(pc[:, 1]).max() > rf:
            raise MuscleHipError("PathIndex: a path point leaves the halo the loss kernels stage")
        ln = np.array([len(p) for p in flat], np.int32)
        off = np.concatenate([[0], np.cumsum(ln)[:-1]]).astype(np.int32)
        return tuple(torch.from_numpy(a).to(device) for a in (pc.reshape(-1).copy(), off, ln)) + (len(flat),)
