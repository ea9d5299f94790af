"""Host logic of two-shard location (shmr_amd/csrc/locate_plan.hpp) and the pair
plan a codec caches, on the CPU: tools/locate_pair_plan_check.cpp is compiled
with g++ under ASan + UBSan together with the host GF code (gf256.cpp) and run
as a program of its own.

The pair kernel tells candidate pairs apart by the coefficients of
locate_pair_ref.pair_coeffs_ref: the plan must hold exactly those of the matrix
the oracle builds, in the fixed pair-index order.  The resolve rule turns a
block's verify word, single answer and pair bitmap into its two answers; the
pair resolve kernel runs the same function.
"""
import os
import subprocess

import pytest

from locate_pair_ref import pair_coeffs_ref, pair_index

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")

CODES = [(10, 4), (4, 4), (5, 5), (8, 6)]
CLEAN, NONE = -1, -2
FULL = 0xffffffff


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locate_pair") / "locate_pair_plan_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tools", "locate_pair_plan_check.cpp"),
                    os.path.join(CSRC, "gf256.cpp"), "-o", exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def limits(check):
    min_parity, max_data, lds, lds_next = (int(x) for x in check("limits\n")[0].split())
    return min_parity, max_data, lds, lds_next


def test_limits(limits):
    """pair_max_data is the largest k whose staged 4-row plan (k * 4 tables of
    32 bytes, k + 4 offsets of 8) and pair tables (32 bytes per coefficient)
    fit 64 KiB."""
    min_parity, max_data, lds, lds_next = limits
    assert min_parity == 4

    def lds_of(k):
        plan = (k * 4 * 32 + k * 8 + 4 * 8 + 15) // 16 * 16
        return plan + 32 * (2 * k * (k - 1) + 8 * k)
    assert lds == lds_of(max_data) <= 64 * 1024 < lds_of(max_data + 1) == lds_next
    assert max_data in (28, 29)


def _plan(check, k, p):
    out = check(f"plan {k} {p}\n")
    tag, n, npairs, words = out[0].split()
    assert tag == "coeffs"
    return int(n), int(npairs), int(words), [int(x) for x in out[1].split()] if int(n) else []


def _codes(limits):
    return CODES + [(limits[1], 4)]


@pytest.mark.parametrize("which", range(len(CODES) + 1))
def test_plan_holds_the_coefficients_of_the_oracles_matrix(check, limits, which):
    k, p = _codes(limits)[which]
    n, npairs, words, coeffs = _plan(check, k, p)
    ndd = k * (k - 1) // 2
    assert npairs == ndd + 4 * k and words == (npairs + 31) // 32
    assert n == 4 * ndd + 8 * k == len(coeffs)
    dd, dp = pair_coeffs_ref(k, p)
    assert coeffs[:4 * ndd] == dd.reshape(-1).tolist()
    assert coeffs[4 * ndd:] == dp.reshape(-1).tolist()
    # two candidates with the same coefficients could not be told apart
    assert len({tuple(row) for row in dd.tolist()}) == ndd
    for r in range(4):
        assert len({tuple(x) for x in dp[:, r].tolist()}) == k


@pytest.mark.parametrize("k", [1, 2, 4, 10, 29])
def test_pair_index_is_a_bijection(check, k):
    out = check(f"index {k}\n")
    npairs = k * (k - 1) // 2 + 4 * k
    rows = [tuple(int(x) for x in line.split()) for line in out[:npairs]]
    assert out[npairs] == "ok"
    assert [i for i, _, _ in rows] == list(range(npairs))
    want = [(a, b) for a in range(k) for b in range(a + 1, k)] + [(a, k + r) for a in range(k) for r in range(4)]
    assert [(e, f) for _, e, f in rows] == want                  # data-data first, lexicographic; then a * 4 + r
    assert all(pair_index(k, e, f) == i for i, e, f in rows)


def test_refused_codecs_have_no_plan(check, limits):
    max_data = limits[1]
    assert _plan(check, 4, 3)[0] == 0
    assert _plan(check, 4, 33)[0] == 0
    assert _plan(check, max_data + 1, 4)[0] == 0
    assert _plan(check, 4, 32)[0] == 2 * 4 * 3 + 8 * 4
    assert _plan(check, max_data, 4)[0] > 0


def _resolve(check, cases):
    text = "".join(f"resolve {k} {p} {word} {single} {len(bm)} " + " ".join(str(w) for w in bm) + "\n"
                   for k, p, word, single, bm in cases)
    return [tuple(int(x) for x in line.split()) for line in check(text)[:len(cases)]]


def _bits(*idx, words=3):
    bm = [0] * words
    for i in idx:
        bm[i // 32] |= 1 << (i % 32)
    return bm


def test_resolve_pair_rule(check):
    k = 10                                    # RS(10, p): 45 + 40 = 85 candidates, 3 words
    dd = lambda a, b: pair_index(k, a, b)
    dp = lambda a, r: pair_index(k, a, k + r)
    full = [FULL] * 3
    cases = [
        # (k, p, verify word, single answer, pair bitmap)               -> answers
        # 1. a single answer stands, whatever the bitmap
        ((k, 4, 0, CLEAN, full), (CLEAN, CLEAN)),
        ((k, 4, 0, CLEAN, _bits(dd(0, 1))), (CLEAN, CLEAN)),
        ((k, 4, 15, 7, _bits(dd(0, 1))), (7, CLEAN)),
        ((k, 4, 4, k + 2, full), (k + 2, CLEAN)),
        ((k, 5, 31, 3, _bits()), (3, CLEAN)),
        # 2. two rows: those two parity shards, ascending
        ((k, 4, 0b0011, NONE, full), (k, k + 1)),
        ((k, 4, 0b1010, NONE, _bits()), (k + 1, k + 3)),
        ((k, 6, 0b100100, NONE, full), (k + 2, k + 5)),               # beyond the group as well
        ((k, 4, 0b110000, NONE, full), (NONE, NONE)),                 # bits past the parity rows
        # 3. a row at or above 4 that does not differ: no data shard is in the pair
        ((k, 5, 0b01111, NONE, _bits(dd(0, 1))), (NONE, NONE)),
        ((k, 6, 0b101111, NONE, _bits(dp(2, 1))), (NONE, NONE)),
        ((k, 6, 0b110111, NONE, _bits(dp(2, 3))), (2, k + 3)),        # a row of the group may be zero
        # 4. exactly one candidate
        ((k, 4, 15, NONE, _bits(dd(0, 1))), (0, 1)),
        ((k, 4, 15, NONE, _bits(dd(3, 9))), (3, 9)),
        ((k, 4, 15, NONE, _bits(dd(8, 9))), (8, 9)),
        ((k, 4, 15, NONE, _bits(dp(0, 0))), (0, k)),
        ((k, 4, 15, NONE, _bits(dp(9, 3))), (9, k + 3)),
        ((k, 4, 0b0111, NONE, _bits(dp(4, 3))), (4, k + 3)),          # three rows are enough
        ((k, 5, 31, NONE, _bits(dp(4, 2))), (4, k + 2)),
        ((k, 4, 15, NONE, _bits(dd(2, 5), 85)), (2, 5)),              # bits at and above pair_count are ignored
        ((k, 4, 15, NONE, _bits(85, 86, 95)), (NONE, NONE)),          # ... and never count as candidates
        ((k, 4, 15, NONE, _bits()), (NONE, NONE)),                    # nobody survives
        ((k, 4, 15, NONE, _bits(dd(0, 1), dd(0, 2))), (NONE, NONE)),  # two survive
        ((k, 4, 15, NONE, _bits(dd(0, 1), dp(9, 3))), (NONE, NONE)),  # ... in different words
        ((k, 4, 15, NONE, full), (NONE, NONE)),
        ((k, 4, 0b0001, NONE, full), (NONE, NONE)),                   # (not locate's: one row always has an answer)
        # one word of candidates; k = 29: 17 words
        ((4, 4, 15, NONE, _bits(pair_index(4, 2, 3), words=1)), (2, 3)),
        ((4, 4, 15, NONE, _bits(pair_index(4, 3, 7), words=1)), (3, 7)),
        ((29, 4, 15, NONE, _bits(pair_index(29, 27, 28), words=17)), (27, 28)),
        ((29, 4, 15, NONE, _bits(pair_index(29, 28, 32), words=17)), (28, 32)),
        ((29, 4, 15, NONE, _bits(0, 521, words=17)), (NONE, NONE)),
        ((29, 4, 15, NONE, _bits(522, 543, words=17)), (NONE, NONE)),
    ]
    got = _resolve(check, [c for c, _ in cases])
    assert got == [want for _, want in cases], [(c, g, w) for (c, w), g in zip(cases, got) if g != w]
