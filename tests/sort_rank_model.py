"""Host model of the fast sort's rank rule (sph_taichi_amd/csrc/sph_sort.hip, SPH_OPT_SORT_FAST), in numpy.

The input order is sorted by `key_old` (the previous sort's output); `key_new` holds the cell every old index hashes to
now.  The stable counting sort by `key_new` -- ascending old index inside a cell -- sends old index i to `dst[i]`.

For cell c with old segment [ob, oe) the new members are, in order: the arrivals with old index < ob, the stayers in
their old order, the arrivals with old index >= oe.  The model works through the same per-cell state the kernels keep:

  delta[c]      arrivals - leavers             (hash pass, two atomics per mover)
  head / nxt    per cell the chain of arrivals (hash pass, one returning exchange per mover), 1 + old index, 0 = end
  new_end       inclusive scan of delta[c] + old count, the old count being the adjacent difference of old_end

  stayer i : dst = new_start(c) + A_lo(c) + (i - ob) - #movers in [ob, i)
  arrival i: dst = new_start(c) + #arrivals of c with a smaller old index + (i >= ob ? #stayers of c : 0)
             with #stayers = new count - #arrivals
"""
from __future__ import annotations

import numpy as np


def brute_force(key_new: np.ndarray) -> np.ndarray:
    """dst[i] of the stable sort by key_new (the reference's serial order)."""
    order = np.argsort(np.asarray(key_new), kind="stable")
    dst = np.empty(len(order), dtype=np.int64)
    dst[order] = np.arange(len(order))
    return dst


def old_cell_end(key_old: np.ndarray, G: int) -> np.ndarray:
    return np.cumsum(np.bincount(np.asarray(key_old), minlength=G)[:G]).astype(np.int64)


def hash_pass(key_old, key_new, G, rng=None):
    """delta, head, nxt as the fast hash pass leaves them; the movers push themselves in any order (atomics)."""
    key_old = np.asarray(key_old)
    key_new = np.asarray(key_new)
    delta = np.zeros(G, dtype=np.int64)
    head = np.zeros(G, dtype=np.int64)
    nxt = np.zeros(len(key_old), dtype=np.int64)
    movers = np.nonzero(key_old != key_new)[0]
    if rng is not None:
        movers = rng.permutation(movers)
    for i in movers:
        delta[key_old[i]] -= 1
        delta[key_new[i]] += 1
        nxt[i] = head[key_new[i]]
        head[key_new[i]] = i + 1
    return delta, head, nxt


def scan_pass(delta, old_end):
    old_count = np.diff(np.concatenate(([0], old_end)))
    return np.cumsum(delta + old_count)


def fast_rank(key_old, key_new, G, rng=None, block=256) -> np.ndarray:
    """dst[i] by the fast rule, computed the way the scatter does: thread i is old index i, the movers before it are
    counted per `block` from the block's mover flags plus a direct comparison of the keys over [ob, block start)."""
    key_old = np.asarray(key_old, dtype=np.int64)
    key_new = np.asarray(key_new, dtype=np.int64)
    n = len(key_old)
    assert np.all(np.diff(key_old) >= 0), "the input order must be sorted by the old key"
    old_end = old_cell_end(key_old, G)
    delta, head, nxt = hash_pass(key_old, key_new, G, rng)
    new_end = scan_pass(delta, old_end)
    mover = key_old != key_new
    dst = np.empty(n, dtype=np.int64)
    for i in range(n):
        c = key_new[i]
        ob = old_end[c - 1] if c > 0 else 0
        nb = new_end[c - 1] if c > 0 else 0
        arrivals = smaller = 0
        a = head[c]
        while a != 0:
            arrivals += 1
            smaller += 1 if a - 1 < i else 0
            a = nxt[a - 1]
        if mover[i]:
            stayers = new_end[c] - nb - arrivals
            dst[i] = nb + smaller + (stayers if i >= ob else 0)
        else:
            bs = (i // block) * block
            lo = max(ob, bs)
            gone = int(np.count_nonzero(mover[lo:i]))                          # the block's ballots
            if ob < bs:
                gone += int(np.count_nonzero(key_old[ob:bs] != key_new[ob:bs]))  # the stretch before the block
            dst[i] = nb + smaller + (i - ob) - gone
    return dst
