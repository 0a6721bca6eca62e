"""The sampling rule of the device BEACON sampler (include/muscle_hip.h) as tests/field_sample_ref.py restates it:
distinct keys, the k-subset, its uniformity over draws, the edges of the active rule, and the input conditions the GPU tests
(tests/test_gpu_field_sample.py) rely on."""
import math

import numpy as np
import pytest

import dec_ref as R
import field_sample_ref as FS

SEED = 20261021


def test_keys_of_a_slot_side_are_distinct():
    st = FS.stream_key(SEED, 0)
    for s, side in ((0, 0), (0, 1), (319, 1)):
        keys = [FS.key(st, s, side, p) for p in range(5000)]
        assert len(set(keys)) == len(keys)
        assert all(k & 0xFFFFFFFF == p for p, k in enumerate(keys))          # the lower half is the source pixel
    # equal upper halves are told apart by p: the rule's order is the order of (upper half, p)
    assert FS.key(st, 3, 0, 7) != FS.key(st, 3, 0, 8)


def test_subset_is_the_k_smallest_keys_and_follows_every_argument():
    src = np.arange(3, 3 + 3 * 60, 3)
    k = 8
    st = FS.stream_key(SEED, 5)
    got = FS.k_smallest(st, 4, 1, src, k)
    keys = sorted(FS.key(st, 4, 1, int(p)) for p in src)
    assert sorted(FS.key(st, 4, 1, p) for p in got) == keys[:k]
    assert got == sorted(got) and len(set(got)) == k
    others = [FS.k_smallest(FS.stream_key(SEED + 1, 5), 4, 1, src, k), FS.k_smallest(FS.stream_key(SEED, 6), 4, 1, src, k),
              FS.k_smallest(st, 5, 1, src, k), FS.k_smallest(st, 4, 0, src, k)]
    for o in others:
        assert o != got


def test_mix_wraps_as_uint64():
    assert FS.mix(0) == 0
    assert 0 <= FS.mix((1 << 64) - 1) < (1 << 64)
    assert FS.mix(1 << 64) == FS.mix(0)                                       # arithmetic modulo 2^64
    assert FS.stream_key((1 << 64) - 1, 0) == FS.mix((FS.GOLDEN - 1) & FS.M64)


def test_inclusion_is_uniform_over_draws():
    """n = 40 entries, k = 8, D = 4000 draws: every entry's inclusion count within 5 sigma of D*k/n = 800, sigma =
    sqrt(D * 0.2 * 0.8) = 25.3.  A property of the rule, deterministic for the seed."""
    n, k, D = 40, 8, 4000
    src = np.arange(100, 100 + 7 * n, 7)
    hits = dict.fromkeys(src.tolist(), 0)
    for draw in range(D):
        for p in FS.k_smallest(FS.stream_key(SEED, draw), 11, 0, src, k):
            hits[p] += 1
    sigma = math.sqrt(D * 0.2 * 0.8)
    worst = max(abs(c - D * k / n) for c in hits.values())
    print("worst deviation", worst, "of", 5 * sigma)
    assert worst <= 5 * sigma
    assert sum(hits.values()) == D * k


def test_edges_of_the_active_rule():
    k = 8
    cnt = np.array([[k, 50, 60], [k + 1, k + 1, 20], [50, k, 60], [0, 0, 0]], dtype=np.int32)
    assert FS.active_slots(cnt, k).tolist() == [0, 1, 0, 0]
    few = np.array([[k + 1, k + 1, 5], [k + 1, k + 1, 4]], dtype=np.int32)   # 9 positives in total
    assert FS.active_slots(few, k).tolist() == [0, 0]
    few[1, 2] = 5                                                            # 10
    assert FS.active_slots(few, k).tolist() == [1, 1]


def test_unlabelled_slot_counts_zero_and_is_inactive():
    H, W = 16, 16
    mag, orient, mx, lab = FS.sample_inputs(H, W)
    lab[1, 2] = 0.0                                                          # the all-positive plane
    cnt = FS.counts(mag, orient, mx, lab, 1, H, W)
    assert cnt[5].tolist() == [0, 0, 0] and cnt[3].tolist() == [0, 0, 0]
    assert FS.active_slots(cnt, 4)[5] == 0
    lab[1, 2] = 1.0
    assert FS.counts(mag, orient, mx, lab, 1, H, W)[5, 2] == H * W


@pytest.mark.parametrize("step", R.SELECT_STEPS)
@pytest.mark.parametrize("hw", R.SELECT_HW)
def test_counts_and_targets_restate_field_select(hw, step):
    """entries() is dec_ref.field_select with the source pixel kept: same lists, same counts, on every select case."""
    H, W = hw
    mag, orient, mx, lab = FS.sample_inputs(H, W)
    slots = [(n, f) for n in range(2) for f in range(3)]
    outs, ins, counts = R.field_select(mag, orient, mx, slots, step, H, W)
    lab[:] = 1.0
    assert FS.counts(mag, orient, mx, lab, step, H, W).tolist() == counts.tolist()
    for s, (n, f) in enumerate(slots):
        so, to, si, ti, _ = FS.entries(mag, orient, mx, n, f, step, H, W)
        assert to.tolist() == outs[s].tolist() and ti.tolist() == ins[s].tolist()
        assert np.all(np.diff(so) > 0) and np.all(np.diff(si) > 0)


def test_gpu_case_conditions():
    """What tests/test_gpu_field_sample.py takes for granted about its inputs."""
    for H, W, k in FS.SAMPLE_CASES:
        mag, orient, mx, lab = FS.sample_inputs(H, W)
        ref = FS.sample(mag, orient, mx, lab, 1, k, SEED, 0, H, W)
        if (H, W) == (3, 3):
            assert int(ref["counts"][:, 2].sum()) == 9 and ref["n_active"] == 0
            continue
        assert ref["n_active"] >= 1 and ref["n_active"] < 6                  # active and inactive slots in one launch
        assert ref["active"][5] == 1                                         # the all-positive plane
        assert ref["counts"][5, 0] > k and ref["counts"][5, 1] > k
        again = FS.sample(mag, orient, mx, lab, 1, k, SEED, 1, H, W)
        assert not np.array_equal(ref["pts_out"], again["pts_out"])
        for t in (ref["pts_out"], ref["pts_in"]):
            assert t[:, 1].min() >= 0 and t[:, 1].max() < H * W
    H, W, k, step = FS.EDGE_CASE
    for want, act in ((k, 0), (k + 1, 1)):
        mag, orient, mx, lab = FS.sample_inputs(H, W)
        n_out, n_in = FS.fit_plane(mag, orient, mx, 1, 2, step, H, W, want)
        assert n_out == want and n_in > k
        assert FS.sample(mag, orient, mx, lab, step, k, SEED, 0, H, W)["active"][5] == act


def test_train_muscle_refuses_graph_without_device_sampler_or_with_energy(capsys):
    from muscle_amd import train_muscle
    base = ["--mask_root", "masks"]
    a = train_muscle.parse_args(base)
    assert a.beacon_sampler == "host" and a.graph == 0
    a = train_muscle.parse_args(base + ["--graph", "1", "--beacon_sampler", "device"])
    assert a.beacon_sampler == "device" and a.graph == 1
    for bad in (["--graph", "1"], ["--graph", "1", "--beacon_sampler", "host"],
                ["--graph", "1", "--beacon_sampler", "device", "--energy_weight", "0.5"], ["--beacon_sampler", "gpu"]):
        with pytest.raises(SystemExit):
            train_muscle.parse_args(base + bad)
    capsys.readouterr()


def test_field_loss_refuses_an_unknown_sampler():
    from muscle_amd import edge
    with pytest.raises(ValueError):
        edge.FieldLoss(sobel_size=5, k=8, sampler="gpu")
    c = edge.FieldLoss(sobel_size=5, k=8)
    assert c.sampler == "host" and c.draws == 0 and c.last_sample is None
