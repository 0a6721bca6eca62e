"""The device sampler of the BEACON boundary points, restated in numpy (include/muscle_hip.h): counts for every
(sample, class) slot, the active rule, the 64-bit keys, the k smallest keys per active slot and side, the point tables with their
filler rows.  The positives and their targets come from dec_ref.field_select's arithmetic, restated here per source pixel (an
entry is identified by its source pixel, which field_select's lists no longer carry)."""
import numpy as np

import dec_ref as R

M64 = (1 << 64) - 1
GOLDEN = 0x9E3779B97F4A7C15


def mix(z):
    z &= M64
    z ^= z >> 30
    z = (z * 0xBF58476D1CE4E5B9) & M64
    z ^= z >> 27
    z = (z * 0x94D049BB133111EB) & M64
    z ^= z >> 31
    return z


def stream_key(seed, draw):
    return mix((seed + GOLDEN * (draw + 1)) & M64)


def key(stream, s, side, p):
    return ((mix(stream ^ (((2 * s + side) << 32) | p)) >> 32) << 32) | p


def k_smallest(stream, s, side, sources, k):
    """The k source pixels with the smallest keys, in ascending source pixel."""
    order = sorted(sources, key=lambda p: key(stream, s, side, int(p)))
    return sorted(int(p) for p in order[:k])


def entries(mag, orient, mx, n, f, step, H, W):
    """(out sources, out targets, in sources, in targets, n_pos) of one plane: dec_ref.field_select's positives and index
    arithmetic with the source pixel kept; sources ascending."""
    HW = H * W
    ind = np.arange(HW, dtype=np.int64)
    m = np.float32(mx[n, f])
    pos = (mag[n, f].astype(np.float32) >= np.float32(0.8) * m) & bool(m > np.float32(1.0))
    o = orient[n, f].astype(np.int64) + 1
    o4, o26 = (o % 4 == 0).astype(np.int64), ((o == 2) | (o == 6)).astype(np.int64)
    lt4 = (o < 4).astype(np.int64)
    oi = ind + np.where(lt4 == 1, step * step, -step) * (o4 * W) + np.where((1 + o) % 2 == 1, -1, 1) * o26
    ii = ind + np.where(lt4 == 1, -step, 1) * (o4 * W) + np.where(o % 2 == 1, -1, 1) * o26

    def keep(x):
        r = np.mod(x, W - 1)
        return (r != 0) & (r != 1) & (x > 0) & (x < HW - 1)
    ko, ki = pos & keep(oi), pos & keep(ii)
    return ind[ko], oi[ko], ind[ki], ii[ki], int(pos.sum())


def counts(mag, orient, mx, lab_fg, step, H, W):
    """[N*F, 3] int32 {n_out, n_in, n_pos}; an unlabelled slot counts zeros."""
    N, F = lab_fg.shape
    out = np.zeros((N * F, 3), dtype=np.int32)
    for n in range(N):
        for f in range(F):
            if lab_fg[n, f] != 0:
                so, _, si, _, npos = entries(mag, orient, mx, n, f, step, H, W)
                out[n * F + f] = (len(so), len(si), npos)
    return out


def active_slots(cnt, k):
    enough = int(cnt[:, 2].astype(np.int64).sum()) >= 10
    return (enough & (cnt[:, 0] > k) & (cnt[:, 1] > k)).astype(np.int32)


def sample(mag, orient, mx, lab_fg, step, k, seed, draw, H, W):
    """dict(counts, active, n_active, pts_out, pts_in): the whole launch for draw number `draw` (the counter's value before it)."""
    N, F = lab_fg.shape
    HW = H * W
    cnt = counts(mag, orient, mx, lab_fg, step, H, W)
    act = active_slots(cnt, k)
    st = stream_key(seed, draw)
    tables = [np.zeros((N * F * k, 2), dtype=np.int32) for _ in (0, 1)]
    for s in range(N * F):
        n, f = divmod(s, F)
        rows = slice(s * k, (s + 1) * k)
        if not act[s]:
            for t in tables:
                t[rows, 0] = n
                t[rows, 1] = (np.arange(s * k, (s + 1) * k, dtype=np.int64) % HW).astype(np.int32)
            continue
        so, to, si, ti, _ = entries(mag, orient, mx, n, f, step, H, W)
        for side, (src, tgt) in enumerate(((so, to), (si, ti))):
            chosen = k_smallest(st, s, side, src, k)
            lookup = dict(zip(src.tolist(), tgt.tolist()))
            tables[side][rows, 0] = n
            tables[side][rows, 1] = [lookup[p] for p in chosen]
    return dict(counts=cnt, active=act, n_active=int(act.sum()), pts_out=tables[0], pts_in=tables[1])


def sample_inputs(H, W):
    """dec_ref.select_inputs as [N=2, F=3] planes (numpy copies) plus lab_fg with plane (1,0) unlabelled.  At (3,3) only the
    all-positive plane (1,2) is labelled: its 9 positives are then all there are, one short of the 10 the rule asks for (with
    every plane labelled the six 3x3 planes hold 32)."""
    mag, orient, mx, _ = R.select_inputs(H, W)
    lab = np.ones((2, 3), dtype=np.float32)
    lab[1, 0] = 0.0
    if (H, W) == (3, 3):
        lab[:] = 0.0
        lab[1, 2] = 1.0
    return mag.numpy().copy(), orient.numpy().copy(), mx.numpy().copy(), lab


def fit_plane(mag, orient, mx, n, f, step, H, W, n_out):
    """Zero magnitudes of plane (n,f) (never at its maximum's pixel), one pixel at a time, until its out count is n_out: pixels
    that give an out entry only go first (last source first), so that the in count stays as large as it can.  Returns the
    plane's (n_out, n_in) reached."""
    top = int(np.argmax(mag[n, f]))
    while True:
        so, _, si, _, _ = entries(mag, orient, mx, n, f, step, H, W)
        if len(so) <= n_out:
            return len(so), len(si)
        both = set(si.tolist())
        cand = [int(p) for p in so if int(p) != top]
        only = [p for p in cand if p not in both]
        assert cand, "cannot shrink the plane further"
        mag[n, f, (only or cand)[-1]] = 0.0


# (H, W, k) of the GPU sampling cases; EDGE_CASE: plane (1,2) of (16,16) shrunk to n_out = k (inactive) and k + 1 (active)
SAMPLE_CASES = [(16, 16, 4), (16, 16, 8), (17, 19, 4), (17, 19, 8), (40, 33, 128), (3, 3, 4)]
EDGE_CASE = (16, 16, 8, 1)          # H, W, k, step
