"""CPU tests of the batched evaluation sweeps: the size grouping, the two script arguments, the header's new entry points."""
import numpy as np
import pytest


def _pairs():
    g = np.random.default_rng(0)
    sizes = [(500, 375), (375, 500), (500, 333), (500, 375), (334, 500)]
    return [(f"n{i:03d}", sizes[int(g.integers(0, len(sizes)))]) for i in range(57)]


@pytest.mark.parametrize("batch", [1, 2, 3, 8, 100])
def test_size_buckets(batch):
    from muscle_amd.evaluation import size_buckets
    pairs = _pairs()
    size_of = dict(pairs)
    buckets = size_buckets(pairs, batch)
    flat = [n for b in buckets for n in b]
    assert sorted(flat) == sorted(size_of) and len(flat) == len(size_of)             # every name exactly once
    for b in buckets:
        assert 1 <= len(b) <= batch and len({size_of[n] for n in b}) == 1               # homogeneous, at most `batch`
    order = {n: i for i, (n, _) in enumerate(pairs)}
    for sz in set(size_of.values()):
        grp = [n for n in flat if size_of[n] == sz]
        assert grp == sorted(grp, key=order.get)                                        # list order inside a group
        full = [b for b in buckets if size_of[b[0]] == sz]
        assert all(len(b) == batch for b in full[:-1])                                  # only a group's last batch is short
    if batch == 1:
        assert flat == [n for n, _ in pairs]                                            # the list itself


def test_size_buckets_edges():
    from muscle_amd.evaluation import size_buckets
    assert size_buckets([], 4) == []
    assert size_buckets([("a", (3, 2)), ("b", [3, 2]), ("c", (2, 3))], 2) == [["a", "b"], ["c"]]
    with pytest.raises(ValueError):
        size_buckets([("a", (1, 1))], 0)


def test_script_arguments_default_to_one():
    from muscle_amd import train_mcl, train_muscle
    assert train_mcl.parse_args([]).eval_batch == 1
    assert train_mcl.parse_args(["--eval_batch", "8"]).eval_batch == 8
    assert train_muscle.parse_args(["--mask_root", "m"]).val_batch == 1
    assert train_muscle.parse_args(["--mask_root", "m", "--val_batch", "4"]).val_batch == 4
    for bad in ("0", "9"):
        with pytest.raises(SystemExit):
            train_mcl.parse_args(["--eval_batch", bad])
        with pytest.raises(SystemExit):
            train_muscle.parse_args(["--mask_root", "m", "--val_batch", bad])


def test_decode_pool_is_small_and_fixed():
    from muscle_amd import evaluation as E
    assert 1 <= E._DECODE_THREADS <= 8 and E.MAX_EVAL_BATCH == 8
    with pytest.raises(ValueError, match="batch"):
        E._check_batch(9)


def test_header_declares_the_batched_entry_points():
    from muscle_amd._lib import HEADER_PATH, LONG_RETURNS, parse_header
    sigs = parse_header()
    assert sigs["mx_rapid_eval_lr"] == "ppppiiiiiiiipplp"
    assert sigs["mx_rapid_eval_lr_ws"] == "ii" and "mx_rapid_eval_lr_ws" in LONG_RETURNS
    assert sigs["mx_seg_infer_batch"] == "piiiiiipppppp"
    text = open(HEADER_PATH).read()
    assert "train_mcl.py:297-303" in text and "train_muscle.py:224-283" in text         # declared with their reference lines
