"""Host logic of single-shard location (shmr_amd/csrc/locate_plan.hpp) and the
locate plan a codec caches, on the CPU: tools/locate_plan_check.cpp is compiled
with g++ under ASan + UBSan together with the host GF code (gf256.cpp).

The locate kernel tells damaged data shards apart by s_r == q[r][j] (x) s_0
with q[r][j] = C[r][j] / C[0][j]: the plan must hold exactly those ratios of
the matrix the oracle builds, every C[0][j] must be non-zero for them to exist,
and the ratios of one row must differ between shards or two shards could not be
told apart.  The resolve rule turns a block's verify word and candidate bitmap
into its answer; the resolve kernel runs the same function.
"""
import os
import subprocess

import pytest

from oracle import rs_oracle as O

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")

CODES = [(2, 2), (4, 2), (8, 3), (10, 4), (5, 5), (3, 9), (16, 4), (100, 30), (200, 56), (4, 32)]
CLEAN, NONE = -1, -2


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("locate") / "locate_plan_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, os.path.join(ROOT, "tools", "locate_plan_check.cpp"),
                    os.path.join(CSRC, "gf256.cpp"), "-o", exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return run


def _rows(lines, n):
    return [[int(x) for x in line.split()] for line in lines[:n]]


@pytest.mark.parametrize("k,p", CODES)
def test_plan_holds_the_ratios_of_the_oracles_matrix(check, k, p):
    out = check(f"plan {k} {p}\n")
    tag, m, kk = out[0].split()
    R = min(p, 4) if p <= 32 else 1            # (p > 32: the matrix is still checked, the API refuses the codec)
    assert (tag, int(m), int(kk)) == ("rows", R - 1, k)
    C = _rows(out[1:], p)
    q = _rows(out[1 + p:], R - 1)
    assert C == O.ReedSolomon(k, p).parity_rows().tolist()          # the golden matrix
    assert all(C[r][j] != 0 for r in range(p) for j in range(k))
    for r in range(1, R):
        for j in range(k):
            assert O.gal_mul(q[r - 1][j], C[0][j]) == C[r][j], (r, j)
        assert len(set(q[r - 1])) == k, f"two data shards share the ratio of row {r}"


def test_codecs_that_cannot_locate_have_no_plan(check):
    """p = 1: nothing to compare; p > 32: rows share bit 31 of the verify word."""
    assert check("plan 4 1\n")[0] == "rows 0 4"
    assert check("plan 4 33\n")[0] == "rows 0 4"
    assert check("plan 4 32\n")[0] == "rows 3 4"


def test_ratio_rows_of_a_given_matrix(check):
    C = [[1, 2, 3], [4, 5, 6], [7, 8, 9]]
    out = check("ratios 3 3\n" + " ".join(str(x) for row in C for x in row) + "\n")
    assert out[0] == "ok"
    assert _rows(out[1:], 2) == [[O.gal_div(C[r][j], C[0][j]) for j in range(3)] for r in (1, 2)]
    # a zero in row 0: no ratio exists
    assert check("ratios 3 2\n1 0 3 4 5 6\n")[0] == "zero"
    # one row: nothing to compute
    assert check("ratios 2 1\n7 9\n")[0] == "ok"


def _resolve(check, cases):
    text = "".join(f"resolve {k} {p} {word} {len(bm)} " + " ".join(str(w) for w in bm) + "\n"
                   for k, p, word, bm in cases)
    return [int(x) for x in check(text)[:len(cases)]]


def test_resolve_rule(check):
    full = 0xffffffff
    cases = [
        # (k, p, verify word, bitmap)                          -> answer
        ((8, 3, 0, [full]), CLEAN),                            # a codeword, whatever the bitmap
        ((8, 3, 0, [0]), CLEAN),
        ((8, 3, 1, [full]), 8),                                # one parity row: that parity shard
        ((8, 3, 2, [full]), 9),
        ((8, 3, 4, [0]), 10),
        ((8, 3, 3, [full]), NONE),                             # two rows of three
        ((8, 3, 6, [1]), NONE),
        ((8, 3, 8, [full]), NONE),                             # a bit past the parity rows
        ((8, 3, 7, [1 << 5]), 5),                              # every row, one candidate
        ((8, 3, 7, [1]), 0),
        ((8, 3, 7, [1 << 7]), 7),
        ((8, 3, 7, [(1 << 5) | (1 << 8)]), 5),                 # bits at and above k are ignored
        ((8, 3, 7, [full & ~0xff]), NONE),                     # ... and never count as candidates
        ((8, 3, 7, [0]), NONE),                                # nobody survives
        ((8, 3, 7, [3]), NONE),                                # two survive
        ((8, 3, 7, [full]), NONE),
        ((4, 2, 3, [1 << 3]), 3),                              # p = 2: both rows
        ((4, 2, 1, [0]), 4),
        ((4, 2, 2, [0]), 5),
        ((40, 4, 15, [0, 1 << 7]), 39),                        # a second bitmap word
        ((40, 4, 15, [1 << 31, 0]), 31),
        ((40, 4, 15, [1, 1]), NONE),                           # one candidate in each word
        ((40, 4, 15, [0, 1 << 8]), NONE),                      # bit 40 is not a shard
        ((33, 4, 15, [0, 1]), 32),
        ((4, 32, full, [1 << 2]), 2),                          # p = 32: the word is all ones
        ((4, 32, 1 << 31, [0]), 4 + 31),
        ((4, 32, full >> 1, [1 << 2]), NONE),                  # 31 rows of 32
    ]
    got = _resolve(check, [c for c, _ in cases])
    assert got == [want for _, want in cases], [(c, g, w) for (c, w), g in zip(cases, got) if g != w]
