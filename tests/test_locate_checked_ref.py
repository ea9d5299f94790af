"""The numpy reference of degraded single-shard location (tests/locate_checked_ref.py)
against the facts it must reproduce, and against the rule the kernels run
(`ratio_rule`, the numpy restatement of locate_plan.hpp) on random single-shard
damage, where the two must agree.  CPU only.
"""
import random

import numpy as np
import pytest

from locate_checked_ref import CLEAN, NONE, check_word, locate_checked_ref, pattern, ratio_rule
from oracle import rs_oracle as O

L = 48


def _codeword(k, p, seed):
    rng = np.random.default_rng(seed)
    shards = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(p)]
    O.ReedSolomon(k, p).encode(shards)
    return np.stack(shards)


def _lose(k, p, lost, rng):
    gone = set(rng.sample(range(k + p), lost))
    return [0 if i in gone else 1 for i in range(k + p)]


def _damage(block, shard, rng, ncols=1):
    for col in rng.sample(range(L), ncols):
        block[shard, col] ^= rng.randrange(1, 256)


@pytest.mark.parametrize("k,p", [(4, 3), (4, 4), (8, 3), (10, 4), (6, 6), (3, 5)])
def test_single_damage_is_named_by_both_rules(k, p):
    rng = random.Random(k * 31 + p)
    for trial in range(24):
        lost = rng.randint(0, p)
        present = _lose(k, p, lost, rng)
        block = _codeword(k, p, trial)
        for i in range(k + p):
            if not present[i]:
                block[i] = 0xA5                                   # an absent slot: never read
        assert locate_checked_ref(k, p, block, present) == CLEAN
        assert ratio_rule(k, p, block, present) == CLEAN and check_word(k, p, block, present) == 0
        e = rng.choice([i for i in range(k + p) if present[i]])
        _damage(block, e, rng, ncols=rng.choice([1, 3]))
        s = p - lost
        in_idx, out_idx, _ = pattern(k, p, present)
        want = e if s >= 2 else (CLEAN if s == 0 else NONE)
        assert locate_checked_ref(k, p, block, present) == want, (present, e)
        assert ratio_rule(k, p, block, present) == want, (present, e)
        word = check_word(k, p, block, present)
        if e in in_idx:
            assert word == sum(1 << (o - k) for o in out_idx)     # every surplus row differs
        else:
            assert word == 1 << (e - k)


def test_two_damaged_survivors():
    """s >= 3: never taken for one.  s == 2: different columns cannot be; the
    same column can (distance 3), and then both rules name the same third shard
    or both say NONE."""
    rng = random.Random(7)
    for k, p, lost in [(4, 4, 1), (10, 4, 1), (6, 6, 1), (8, 3, 0)]:           # s = 3, 3, 5, 3
        for trial in range(12):
            present = _lose(k, p, lost, rng)
            block = _codeword(k, p, trial)
            a, b = rng.sample([i for i in range(k + p) if present[i]], 2)
            col = rng.randrange(L)
            block[a, col] ^= rng.randrange(1, 256)
            block[b, col] ^= rng.randrange(1, 256)
            assert locate_checked_ref(k, p, block, present) == NONE
            assert ratio_rule(k, p, block, present) == NONE
    for k, p, lost in [(8, 3, 1), (4, 3, 1), (10, 4, 2)]:                     # s = 2
        for trial in range(12):
            present = _lose(k, p, lost, rng)
            block = _codeword(k, p, trial)
            a, b = rng.sample([i for i in range(k + p) if present[i]], 2)
            ca, cb = rng.sample(range(L), 2)
            block[a, ca] ^= rng.randrange(1, 256)
            block[b, cb] ^= rng.randrange(1, 256)
            assert locate_checked_ref(k, p, block, present) == NONE
            assert ratio_rule(k, p, block, present) == NONE
            block[b, ca] ^= rng.randrange(1, 256)                 # now a and b share column ca
            got = locate_checked_ref(k, p, block, present)
            assert got == NONE                                    # (b is damaged in cb as well: no alias survives)
            assert ratio_rule(k, p, block, present) == got


def test_same_column_alias_at_distance_three():
    """RS(8,3), one absent: an error in two survivors in ONE column that equals
    what a third survivor's damage would leave is reported as that third shard
    by both rules -- the header's s == 2 caveat, constructed."""
    k, p = 8, 3
    present = [1] * 11
    present[2] = 0
    in_idx, out_idx, D = pattern(k, p, present)
    block = _codeword(k, p, 99)
    col, err = 5, 0x3c
    # damage input position 0 by err: syndromes D[r][0] * err.  The same
    # syndromes from input position 1 (e1) plus surplus row 0 (e2):
    #   D[1][1] * e1 = D[1][0] * err,  D[0][1] * e1 ^ e2 = D[0][0] * err
    e1 = O.gal_div(O.gal_mul(int(D[1][0]), err), int(D[1][1]))
    e2 = O.gal_mul(int(D[0][1]), e1) ^ O.gal_mul(int(D[0][0]), err)
    assert e2 != 0
    block[in_idx[1], col] ^= e1
    block[out_idx[0], col] ^= e2
    assert locate_checked_ref(k, p, block, present) == in_idx[0]
    assert ratio_rule(k, p, block, present) == in_idx[0]


def test_rows_beyond_the_first_group_are_where_the_rules_part():
    """RS(6,6), one absent (s = 5): an input plus the fifth surplus row.  The
    definition says NONE (two survivors are damaged); the ratio rule looks at
    four rows and names the input -- the repair call's closing verify demotes it."""
    k, p = 6, 6
    present = [0] + [1] * 11
    in_idx, out_idx, _ = pattern(k, p, present)
    block = _codeword(k, p, 5)
    block[in_idx[2], 3] ^= 0x11
    block[out_idx[4], 40] ^= 0x22
    assert locate_checked_ref(k, p, block, present) == NONE
    assert ratio_rule(k, p, block, present) == in_idx[2]
