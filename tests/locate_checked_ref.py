"""numpy reference of single-shard location in a degraded block
(shmr_ec_locate_checked_batch_dev), written from the definition and not from
the kernel's shortcut.

A set of shards of one block is CONSISTENT when rebuilding the block from any
k of them reproduces the rest (the code is MDS, so "any k" is "the first k":
if the first k reproduce every other member, every k-subset decodes to the
same data).  For a block with absent shards:

  * the survivors are consistent                      -> CLEAN (-1); also with
    exactly k survivors, where nothing can be compared;
  * exactly one survivor e exists such that the survivors without e are
    consistent                                        -> e;
  * otherwise (no such survivor, or several: with k + 1 survivors every e
    leaves k shards, which are always consistent)     -> NONE (-2).

`ratio_rule` is the rule the kernels run (locate_plan.hpp), restated in numpy:
the word of the surplus rows, then the ratio test over the first min(s, 4)
rows.  The two agree wherever at most one survivor is damaged; where they part
(damage in two survivors), include/shmr_ec.h says how.
"""
import numpy as np

from oracle import rs_oracle as O

CLEAN, NONE = -1, -2


def _apply(row, shards, cols):
    """XOR_t row[t] (x) shards[t][cols]."""
    acc = np.zeros(len(cols), dtype=np.uint8)
    for c, sh in zip(row, shards):
        acc ^= O.MUL_TABLE[int(c)][sh[cols]]
    return acc


def _inconsistent_columns(M, k, shards, members, cols):
    """The columns among `cols` in which `members` (shard indices, > k of them
    compared) are not consistent."""
    members = list(members)
    head, rest = members[:k], members[k:]
    if not rest or len(cols) == 0:
        return cols[:0]
    dec = O.mat_invert(M[head])                                      # data = dec * shards[head]
    bad = np.zeros(len(cols), dtype=bool)
    for i in rest:
        row = O.mat_mul(M[i:i + 1], dec)[0]                          # shard i from the head
        bad |= _apply(row, [shards[h] for h in head], cols) != shards[i][cols]
    return cols[bad]


def locate_checked_ref(k, p, shards, present) -> int:
    """shards: [k + p, L] uint8 (absent rows are never read); present: k + p flags."""
    M = O.ReedSolomon(k, p).matrix
    shards = np.asarray(shards, dtype=np.uint8)
    alive = [i for i in range(k + p) if present[i]]
    assert len(alive) >= k
    cols = np.arange(shards.shape[1])
    # (a subset of a consistent set is consistent: only the columns in which the
    # survivors disagree can tell candidates apart)
    bad = _inconsistent_columns(M, k, shards, alive, cols)
    if len(bad) == 0:
        return CLEAN
    found = [e for e in alive if len(_inconsistent_columns(M, k, shards, [i for i in alive if i != e], bad)) == 0]
    return found[0] if len(found) == 1 else NONE


def pattern(k, p, present):
    """(in_idx, out_idx, D) of the pattern: the first k present shards, the
    surplus shards behind them, and D = M[surplus] * inv(M[inputs])."""
    M = O.ReedSolomon(k, p).matrix
    alive = [i for i in range(k + p) if present[i]]
    in_idx, out_idx = alive[:k], alive[k:]
    D = O.mat_mul(M[out_idx], O.mat_invert(M[in_idx])) if out_idx else np.zeros((0, k), dtype=np.uint8)
    return in_idx, out_idx, D


def check_word(k, p, shards, present) -> int:
    """The word of shmr_ec_reconstruct_checked_batch_dev: bit min(r, 31) for
    every surplus parity shard k + r that differs from what the inputs say."""
    in_idx, out_idx, D = pattern(k, p, present)
    shards = np.asarray(shards, dtype=np.uint8)
    cols = np.arange(shards.shape[1])
    word = 0
    for r, o in enumerate(out_idx):
        if (_apply(D[r], [shards[i] for i in in_idx], cols) != shards[o]).any():
            word |= 1 << min(o - k, 31)
    return word


def ratio_rule(k, p, shards, present) -> int:
    """The kernels' rule (locate_plan.hpp resolve_checked over the ratio test)."""
    in_idx, out_idx, D = pattern(k, p, present)
    shards = np.asarray(shards, dtype=np.uint8)
    s = len(out_idx)
    word = check_word(k, p, shards, present)
    if word == 0:
        return CLEAN
    if s < 2:
        return NONE
    if word & (word - 1) == 0:
        return next(o for o in out_idx if word == 1 << min(o - k, 31))
    if word != sum(1 << min(o - k, 31) for o in out_idx):
        return NONE
    R = min(s, 4)
    cols = np.arange(shards.shape[1])
    syn = [_apply(D[r], [shards[i] for i in in_idx], cols) ^ shards[out_idx[r]] for r in range(R)]
    cand = [t for t in range(k)
            if all(np.array_equal(O.MUL_TABLE[O.gal_div(int(D[r][t]), int(D[0][t]))][syn[0]], syn[r])
                   for r in range(1, R))]
    return in_idx[cand[0]] if len(cand) == 1 else NONE
