"""Host logic of single-shard location in degraded blocks (the degraded half of
shmr_amd/csrc/locate_plan.hpp) and the per-pattern ratio plan a codec caches
(gf256.cpp Codec::locate_checked_plan), on the CPU: tools/locate_checked_plan_check.cpp
is compiled with g++ under ASan + UBSan together with the host GF code.

For a presence pattern with s surplus shards the degraded locate kernel tells
damaged inputs apart by s_r == q[r][t] (x) s_0, q[r][t] = D[r][t] / D[0][t],
D = M[surplus] * inv(M[inputs]): the plan must hold exactly those ratios of the
matrix the oracle builds, no D[0][t] may be zero, and the ratio tuples of two
inputs must differ or they could not be told apart.  resolve_checked turns a
block's word, candidate bitmap and pattern into its answer; the degraded
resolve kernel runs the same function.
"""
import itertools
import os
import random
import subprocess

import numpy as np
import pytest

from oracle import rs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")

CLEAN, NONE = -1, -2
FULL = 0xffffffff


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locate_checked") / "locate_checked_plan_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "locate_checked_plan_check.cpp"), os.path.join(CSRC, "gf256.cpp"),
                    "-o", exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return run


def _patterns(k, p):
    """Every presence pattern of RS(k, p) with at least k present."""
    t = k + p
    for lost in range(p + 1):
        for gone in itertools.combinations(range(t), lost):
            yield [0 if i in gone else 1 for i in range(t)]


def _sample(k, p, n, seed):
    """n patterns of a wide code: the complete one, single losses at the edges
    of the data and the parity, and random losses of 1 .. p shards."""
    t, rng = k + p, random.Random(seed)
    out = [[1] * t]
    for i in (0, k - 1, k, t - 1):
        out.append([0 if j == i else 1 for j in range(t)])
    while len(out) < n:
        gone = set(rng.sample(range(t), rng.randint(1, p)))
        out.append([0 if j in gone else 1 for j in range(t)])
    return out


def _check_patterns(check, k, p, patterns):
    patterns = list(patterns)
    out = check("".join(f"plan {k} {p} " + " ".join(map(str, pr)) + "\n" for pr in patterns))
    M = O.ReedSolomon(k, p).matrix
    pos = 0
    for pr in patterns:
        alive = [i for i in range(k + p) if pr[i]]
        inputs, surplus = alive[:k], alive[k:]
        s, R = len(surplus), min(len(surplus), 4)
        mask = sum(1 << min(o - k, 31) for o in surplus)
        assert out[pos] == f"plan {s} {max(R - 1, 0)} {mask}", (pr, out[pos])
        assert [int(x) for x in out[pos + 1].split()] == inputs
        assert (out[pos + 2] == "-") if s == 0 else ([int(x) for x in out[pos + 2].split()] == surplus)
        rows = [[int(x) for x in line.split()] for line in out[pos + 3:pos + 3 + s + max(R - 1, 0)]]
        pos += 3 + s + max(R - 1, 0)
        if s == 0:
            continue
        D = O.mat_mul(M[surplus], O.mat_invert(M[inputs]))
        assert rows[:s] == D.tolist(), pr
        assert D.all(), f"a zero in D of {pr}"                     # the MDS property, entry by entry
        if s < 2:
            continue                                               # no ratio plan: nothing can be located
        q = [[O.gal_div(int(D[r][t]), int(D[0][t])) for t in range(k)] for r in range(1, R)]
        assert rows[s:] == q, pr
        tuples = list(zip(*q))
        assert len(set(tuples)) == k, f"two inputs of {pr} share their ratios"
    assert out[pos] == ""


@pytest.mark.parametrize("k,p", [(4, 3), (4, 4), (8, 3), (10, 4), (3, 5), (6, 6)])
def test_every_pattern_holds_the_ratios_of_the_oracles_matrix(check, k, p):
    _check_patterns(check, k, p, _patterns(k, p))


@pytest.mark.parametrize("k,p,n", [(40, 3, 24), (100, 30, 8)])
def test_sampled_patterns_of_wide_codes(check, k, p, n):
    _check_patterns(check, k, p, _sample(k, p, n, seed=k * 1000 + p))


def _resolve(check, cases):
    text = ""
    for k, s, mask, bm, word, in_idx, out_idx in cases:
        text += (f"resolve {k} {s} {mask} {len(bm)} " + " ".join(map(str, bm)) + f" {word} "
                 + " ".join(map(str, list(in_idx) + list(out_idx))) + "\n")
    return [int(x) for x in check(text)[:len(cases)]]


def test_resolve_rule_of_a_degraded_block(check):
    # RS(8,3) with shard 2 absent: inputs 0 1 3 4 5 6 7 8, surplus 9 10 (s = 2, rows 1 and 2: mask 6)
    i83, o83 = [0, 1, 3, 4, 5, 6, 7, 8], [9, 10]
    # RS(6,6) with shard 0 absent: inputs 1 .. 6, surplus 7 .. 11 (s = 5, rows 1 .. 5: mask 62)
    i66, o66 = [1, 2, 3, 4, 5, 6], [7, 8, 9, 10, 11]
    # RS(40,3) with data shard 5 absent: inputs 0 .. 4, 6 .. 40, surplus 41 42 (mask 6)
    i403, o403 = [i for i in range(41) if i != 5], [41, 42]
    cases = [
        # (k, s, mask, bitmap, word, in_idx, out_idx)                    -> answer
        ((8, 0, 0, [FULL], 0, list(range(8)), []), CLEAN),                # s = 0: nothing compared
        ((8, 0, 0, [0], 0, [0, 1, 2, 3, 4, 5, 6, 9], []), CLEAN),
        ((8, 1, 4, [FULL], 0, [0, 1, 3, 4, 5, 6, 7, 8], [10]), CLEAN),    # s = 1, the row agrees
        ((8, 1, 4, [1], 4, [0, 1, 3, 4, 5, 6, 7, 8], [10]), NONE),        # s = 1, a word: never located,
        ((8, 1, 4, [FULL], 4, [0, 1, 3, 4, 5, 6, 7, 8], [10]), NONE),     # ... not the one-bit rule
        ((8, 2, 6, [FULL], 0, i83, o83), CLEAN),
        ((8, 2, 6, [FULL], 2, i83, o83), 9),                              # one bit: that surplus shard
        ((8, 2, 6, [0], 4, i83, o83), 10),
        ((8, 2, 6, [FULL], 1, i83, o83), NONE),                           # a bit outside the pattern's rows
        ((8, 2, 6, [FULL], 8, i83, o83), NONE),
        ((8, 2, 6, [1 << 2], 6, i83, o83), 3),                            # the mask, one candidate: through in_idx
        ((8, 2, 6, [1 << 7], 6, i83, o83), 8),
        ((8, 2, 6, [1], 6, i83, o83), 0),
        ((8, 2, 6, [(1 << 2) | (1 << 8) | (1 << 31)], 6, i83, o83), 3),   # bits at and above k are ignored
        ((8, 2, 6, [FULL & ~0xff], 6, i83, o83), NONE),                   # ... and never count as candidates
        ((8, 2, 6, [0], 6, i83, o83), NONE),                              # no candidate
        ((8, 2, 6, [5], 6, i83, o83), NONE),                              # two candidates
        ((8, 2, 6, [1 << 2], 7, i83, o83), NONE),                         # more than the mask
        ((6, 5, 62, [1 << 5], 62, i66, o66), 6),                          # s = 5: an input that is a parity shard
        ((6, 5, 62, [1], 62, i66, o66), 1),
        ((6, 5, 62, [FULL], 32, i66, o66), 11),                           # a row of the second group
        ((6, 5, 62, [FULL], 2, i66, o66), 7),
        ((6, 5, 62, [1], 30, i66, o66), NONE),                            # four rows of five
        ((6, 5, 62, [1], 63, i66, o66), NONE),
        ((6, 5, 62, [3], 62, i66, o66), NONE),
        ((40, 2, 6, [1, 0], 6, i403, o403), 0),                           # two bitmap words
        ((40, 2, 6, [1 << 31, 0], 6, i403, o403), 32),
        ((40, 2, 6, [0, 1], 6, i403, o403), 33),
        ((40, 2, 6, [0, 1 << 7], 6, i403, o403), 40),
        ((40, 2, 6, [0, 1 << 8], 6, i403, o403), NONE),                   # bit 40 is not an input
        ((40, 2, 6, [1, 1], 6, i403, o403), NONE),                        # one candidate in each word
        ((4, 2, 3 << 30, [1 << 1], 3 << 30, [0, 1, 2, 3], [34, 35]), 1),  # p = 32: rows 30 and 31
        ((4, 2, 3 << 30, [0], 1 << 31, [0, 1, 2, 3], [34, 35]), 35),
    ]
    got = _resolve(check, [c for c, _ in cases])
    assert got == [want for _, want in cases], [(c, g, w) for (c, w), g in zip(cases, got) if g != w]


@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (10, 4), (6, 6), (40, 4), (4, 32)])
def test_resolve_of_the_complete_pattern_is_the_complete_rule(check, k, p):
    """Every shard present: resolve_checked is locate::resolve, answer for answer."""
    rng = random.Random(k * 100 + p)
    n = (k + 31) // 32
    full = FULL if p >= 32 else (1 << p) - 1
    words = [0, full, full >> 1, full + 1 & FULL, 1 << 31, 3] + [1 << r for r in range(min(p + 2, 32))]
    words += [rng.getrandbits(32) & (full | 1 << min(p, 31)) for _ in range(20)]
    bitmaps = [[0] * n, [FULL] * n] + [[1 << (t % 32) if w == t // 32 else 0 for w in range(n)] for t in range(k)]
    bitmaps += [[1 << (k % 32) if w == k // 32 else 0 for w in range(n)]] if k % 32 else []
    bitmaps += [[rng.getrandbits(32) & rng.getrandbits(32) & rng.getrandbits(32) for _ in range(n)] for _ in range(20)]
    text = "".join(f"both {k} {p} {w} {n} " + " ".join(map(str, bm)) + "\n" for w in words for bm in bitmaps)
    out = check(text)[:len(words) * len(bitmaps)]
    assert len(out) == len(words) * len(bitmaps)
    diff = [line for line in out if line.split()[0] != line.split()[1]]
    assert not diff, diff[:5]
    assert {int(line.split()[0]) for line in out} >= {CLEAN, NONE, 0, k - 1, k, k + p - 1}
