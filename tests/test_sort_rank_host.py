"""The fast sort's rank rule (tests/sort_rank_model.py) against a brute-force stable sort.  CPU only."""
from __future__ import annotations

import numpy as np
import pytest

import sort_rank_model as m


def _sorted_keys(counts):
    return np.repeat(np.arange(len(counts)), counts)


def _check(key_old, key_new, G, seed=0, block=256):
    key_old = np.asarray(key_old)
    key_new = np.asarray(key_new)
    want = m.brute_force(key_new)
    for rng in (None, np.random.default_rng(seed)):        # chain order = the order the movers' atomics land in
        got = m.fast_rank(key_old, key_new, G, rng, block=block)
        assert np.array_equal(got, want)
    assert np.array_equal(np.sort(want), np.arange(len(key_new)))   # a permutation


def test_no_movers():
    k = _sorted_keys([3, 0, 5, 1, 0, 4])
    _check(k, k.copy(), 6)


def test_all_movers():
    k = _sorted_keys([4, 4, 4, 4])
    _check(k, (k + 1) % 4, 4)
    _check(k, 3 - k, 4)


def test_only_leavers_and_only_arrivals():
    k = _sorted_keys([5, 5, 5])
    new = k.copy()
    new[[5, 7, 9]] = 2          # cell 1 only loses, cell 2 only gains (from lower old indices)
    _check(k, new, 3)
    new = k.copy()
    new[[6, 8]] = 0             # cell 0 only gains, from higher old indices
    _check(k, new, 3)


def test_arrivals_from_both_sides():
    k = _sorted_keys([4, 4, 4])
    new = k.copy()
    new[[1, 3]] = 1             # low arrivals
    new[[8, 11]] = 1            # high arrivals
    new[5] = 0                  # and a leaver between stayers
    _check(k, new, 3)


def test_arrival_into_empty_cell_and_cell_emptied():
    k = _sorted_keys([3, 0, 3, 2])
    new = k.copy()
    new[[0, 4, 7]] = 1          # the empty cell 1 is entered from both sides
    _check(k, new, 4)
    new = k.copy()
    new[[6, 7]] = 2             # cell 3 is emptied completely
    _check(k, new, 4)
    new = k.copy()
    new[[0, 1, 2]] = [3, 2, 3]  # cell 0 is emptied completely
    _check(k, new, 4)


def test_flat_cell_zero_and_last_cell():
    k = _sorted_keys([2, 3, 0, 4])
    new = k.copy()
    new[[3, 8]] = 0             # into flat cell 0
    new[[0, 2]] = 3             # into the last cell
    _check(k, new, 4)
    new = k.copy()
    new[5:] = 0                 # the last cell empties into cell 0
    _check(k, new, 4)


def test_chain_a_to_b_to_c():
    k = _sorted_keys([3, 3, 3, 3])
    new = k.copy()
    new[1] = 1                  # a -> b
    new[4] = 2                  # b -> c
    new[7] = 3                  # c -> d in the same step
    _check(k, new, 4)
    new = k.copy()
    new[[0, 1, 2]] = 1          # all of a -> b while all of b -> c
    new[[3, 4, 5]] = 2
    _check(k, new, 4)


def test_segment_straddles_blocks_and_crowded_cell():
    # small blocks: cell segments start before the block of most of their members; one cell is far longer than a block
    k = _sorted_keys([5, 70, 3, 9, 1])
    rng = np.random.default_rng(5)
    for _ in range(20):
        new = k.copy()
        mv = rng.random(len(k)) < 0.2
        new[mv] = rng.integers(0, 5, int(mv.sum()))
        _check(k, new, 5, block=8)


@pytest.mark.parametrize("frac", [0.003, 0.02, 0.3, 1.0])
def test_random_mover_patterns(frac):
    rng = np.random.default_rng(int(frac * 1000))
    for trial in range(25):
        G = int(rng.integers(1, 40))
        counts = rng.integers(0, 12, G)
        if counts.sum() == 0:
            counts[0] = 1
        k = _sorted_keys(counts)
        new = k.copy()
        mv = rng.random(len(k)) < frac
        # mostly neighbouring cells, as particles move; some anywhere
        step = rng.integers(-2, 3, len(k))
        far = rng.integers(0, G, len(k))
        tgt = np.where(rng.random(len(k)) < 0.8, np.clip(k + step, 0, G - 1), far)
        new[mv] = tgt[mv]
        _check(k, new, G, seed=trial, block=int(rng.choice([4, 16, 256])))


def test_scan_of_deltas_is_the_new_histogram():
    rng = np.random.default_rng(11)
    G = 17
    k = _sorted_keys(rng.integers(0, 9, G))
    new = rng.integers(0, G, len(k))
    delta, _, _ = m.hash_pass(k, new, G)
    assert np.array_equal(m.scan_pass(delta, m.old_cell_end(k, G)), np.cumsum(np.bincount(new, minlength=G)))
