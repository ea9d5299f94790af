"""The numpy references of two-shard location (tests/locate_pair_ref.py) on the
CPU: the definition (every pair of the k + p shards against all p rows) and the
first-group rule the library documents, on oracle-encoded blocks.

Every pair of shards is damaged with random non-zero bytes in three layouts:
a shared column (both shards hit in the same three columns), disjoint columns
only, and one byte each.  The definition must return exactly that pair.  The
rule must equal the definition, except at its stated limit (p > 4): a data
shard together with a parity shard beyond the first group of four rows is
reported as the data shard alone -- the group's rows are consistent with it and
every row differs -- which a scrub's closing verify then catches.
"""
import itertools

import numpy as np
import pytest

from locate_pair_ref import CLEAN, NONE, locate_pair_ref, locate_pair_rule, locate_ref, syndromes
from oracle import c_oracle

CODES = [(10, 4), (4, 4), (5, 5), (8, 6)]
L = 24
LAYOUTS = ["shared", "disjoint", "one_byte"]


def codeword(k, p, rng):
    shards = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(p)]
    c_oracle.encode(k, p, shards)
    return np.stack(shards)


def hit(block, shard, cols, rng):
    for c in cols:
        block[shard, c] ^= rng.integers(1, 256, dtype=np.uint8)


def damage_pair(block, e, f, layout, rng):
    if layout == "shared":
        cols = rng.choice(L, 3, replace=False)
        hit(block, e, cols, rng)
        hit(block, f, cols, rng)
    elif layout == "disjoint":
        cols = rng.choice(L, 4, replace=False)
        hit(block, e, cols[:2], rng)
        hit(block, f, cols[2:], rng)
    else:
        cols = rng.choice(L, 2, replace=False)
        hit(block, e, cols[:1], rng)
        hit(block, f, cols[1:], rng)


@pytest.mark.parametrize("layout", LAYOUTS)
@pytest.mark.parametrize("k,p", CODES)
def test_every_pair_of_shards(k, p, layout):
    rng = np.random.default_rng((k * 64 + p) * 8 + LAYOUTS.index(layout))
    clean = codeword(k, p, rng)
    limit = 0
    for e, f in itertools.combinations(range(k + p), 2):
        block = clean.copy()
        damage_pair(block, e, f, layout, rng)
        data, parity = block[:k], block[k:]
        assert locate_pair_ref(k, p, data, parity) == (e, f), (e, f)
        rule = locate_pair_rule(k, p, data, parity)
        if e < k and f >= k + 4:
            # the documented limit: the data shard alone, for the closing verify to catch
            assert rule == (e, CLEAN), (e, f, rule)
            limit += 1
        else:
            assert rule == (e, f), (e, f, rule)
    assert limit == k * max(p - 4, 0)


@pytest.mark.parametrize("k,p", CODES)
def test_single_damage_and_clean_blocks_are_locates(k, p):
    rng = np.random.default_rng(k * 64 + p)
    clean = codeword(k, p, rng)
    assert locate_ref(k, p, clean[:k], clean[k:]) == CLEAN
    assert locate_pair_ref(k, p, clean[:k], clean[k:]) == (CLEAN, CLEAN)
    assert locate_pair_rule(k, p, clean[:k], clean[k:]) == (CLEAN, CLEAN)
    for e in range(k + p):
        for ncols in (1, 3):
            block = clean.copy()
            hit(block, e, rng.choice(L, ncols, replace=False), rng)
            want = locate_ref(k, p, block[:k], block[k:])
            assert want == e
            assert locate_pair_ref(k, p, block[:k], block[k:]) == (want, CLEAN)
            assert locate_pair_rule(k, p, block[:k], block[k:]) == (want, CLEAN)


def _rebuilt_is_codeword(k, p, block, pair):
    """Rebuilds the shards of `pair` from the others, as a scrub does, and
    verifies the block again."""
    shards = [None if i in pair else block[i].copy() for i in range(k + p)]
    full = c_oracle.reconstruct(k, p, shards, L)
    return not syndromes(k, p, np.stack(full[:k]), np.stack(full[k:])).any()


@pytest.mark.parametrize("k,p", CODES)
def test_triple_damage(k, p):
    """p = 4 (distance 5): three damaged shards can pass for two; the rule and
    the definition agree with each other whatever the answer.  p >= 5: NONE, or
    a pair that the verify after the rebuild rejects."""
    rng = np.random.default_rng(k * 64 + p + 1000)
    clean = codeword(k, p, rng)
    triples = list(itertools.combinations(range(k + p), 3))
    for i in rng.choice(len(triples), min(len(triples), 60), replace=False):
        t = triples[i]
        block = clean.copy()
        cols = rng.choice(L, 5, replace=False)
        hit(block, t[0], cols[[0, 1]], rng)          # one shared column, one alone, for each
        hit(block, t[1], cols[[0, 2]], rng)
        hit(block, t[2], cols[[0, 3, 4]], rng)
        data, parity = block[:k], block[k:]
        rule = locate_pair_rule(k, p, data, parity)
        if p == 4:
            assert rule == locate_pair_ref(k, p, data, parity), t
        elif rule != (NONE, NONE):
            assert rule[0] >= 0, (t, rule)
            pair = [x for x in rule if x >= 0]
            assert not _rebuilt_is_codeword(k, p, block, pair), (t, rule)
