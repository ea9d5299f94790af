"""Host logic of the launch planner's run split (shmr_amd/csrc/run_split.hpp),
on the CPU: tools/run_split_check.cpp is compiled with g++ under ASan + UBSan
and fed block lists.

Every launch form that carries its blocks in the kernel arguments (slot
lattices, segment launches of a reconstruct, the lattice / table choice of a
pointer table) takes its runs from split_runs, and the forms only agree on what
fits while they share it.  Checked against a restatement of the rule: a run
ends where the stride changes, where the plan index changes or where the list
stops ascending; a single block is a run of stride 1.
"""
import os
import re
import subprocess

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")

with open(os.path.join(CSRC, "gf_apply.hpp")) as _f:
    MAX_SEGS = int(re.search(r"#define SHMR_MAX_SEGS (\d+)", _f.read()).group(1))   # kern::kMaxSegs


@pytest.fixture(scope="module")
def split(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("runs") / "run_split_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC,
                    os.path.join(ROOT, "tools", "run_split_check.cpp"), "-o", exe], check=True)

    def run(cases, limit=MAX_SEGS):
        """cases: (blocks, plans or None) -> [(count, [(start, first, stride, plan)])]"""
        inp = []
        for blocks, plans in cases:
            inp.append(f"{len(blocks)} {int(plans is not None)} {limit}")
            inp += [f"{b} {plans[i]}" if plans is not None else f"{b}" for i, b in enumerate(blocks)]
        out = subprocess.run([exe], input="\n".join(inp) + "\n", capture_output=True, text=True,
                             check=True).stdout.split("\n")
        res, at = [], 0
        for _ in cases:
            count, given = (int(x) for x in out[at].split())
            res.append((count, [tuple(int(x) for x in line.split()) for line in out[at + 1:at + 1 + given]]))
            at += 1 + given
        return res
    return run


def reference(blocks, plans=None):
    runs = []   # [start, first, stride, plan, length]
    for i, b in enumerate(blocks):
        p, r = (plans[i] if plans is not None else 0), (runs[-1] if runs else None)
        if r and p == r[3] and b > blocks[i - 1] and (r[4] == 1 or b - blocks[i - 1] == r[2]):
            r[2], r[4] = b - blocks[i - 1], r[4] + 1
        else:
            runs.append([i, b, 1, p, 1])
    return [tuple(r[:4]) for r in runs]


def _is_run(blocks, plans):
    d = [b - a for a, b in zip(blocks, blocks[1:])]
    return all(x > 0 and x == d[0] for x in d) and len(set(plans)) <= 1


def _check(case, got, limit=MAX_SEGS):
    blocks, plans = case
    count, runs = got
    want = reference(blocks, plans)
    if len(want) > limit:   # does not fit: limit + 1, the runs so far
        assert count == limit + 1
        assert runs == want[:limit]
        return
    assert count == len(want)
    assert runs == want
    # expanding the runs reproduces the list (and its plan indices) ...
    ends = [r[0] for r in runs[1:]] + [len(blocks)]
    exp = [(first + j * stride, plan) for (start, first, stride, plan), end in zip(runs, ends)
           for j in range(end - start)]
    assert [b for b, _ in exp] == list(blocks)
    assert [p for _, p in exp] == (list(plans) if plans is not None else [0] * len(blocks))
    # ... and no two adjacent runs could be one
    pl = plans if plans is not None else [0] * len(blocks)
    for (s0, _, _, _), s1, e1 in zip(runs, [r[0] for r in runs[1:]], ends[1:]):
        assert not _is_run(blocks[s0:e1], pl[s0:e1]), (blocks[s0:e1], pl[s0:e1], s1)


def _ascending(rng, n):
    """Strides from a few values, held for 1, 2 or many blocks."""
    blocks, b = [], int(rng.integers(0, 1000))
    while len(blocks) < n:
        st = int(rng.choice([1, 1, 2, 3, 7, 64]))
        for _ in range(int(rng.choice([1, 1, 2, 3, 17]))):
            blocks.append(b)
            b += st
    return blocks[:n]


def _plans(rng, n):
    plans, p = [], 0
    while len(plans) < n:
        plans += [p] * int(rng.choice([1, 2, 5, 40]))
        p = int(rng.integers(0, 4))   # (may repeat: no break from the plan then)
    return plans[:n]


def test_random_ascending_lists(split):
    rng = np.random.default_rng(7)
    cases = []
    for i in range(600):
        n = (0, 0, 1, 1, 300, 300)[i] if i < 6 else int(rng.integers(0, 301))
        cases.append((_ascending(rng, n), _plans(rng, n) if i % 2 else None))
    limit = 400   # every run comes back
    for c, g in zip(cases, split(cases, limit)):
        _check(c, g, limit)
    for c, g in zip(cases, split(cases)):   # and against the kernels' limit
        _check(c, g)
    lens = [len(reference(*c)) for c in cases]
    assert min(lens) == 0 and max(lens) > MAX_SEGS


def test_descending_at_a_pattern_boundary(split):
    """A reconstruct groups its blocks by erasure pattern: each group ascends, the
    next starts below the last one's end."""
    cases = []
    for npat, n in ((3, 64), (2, 7), (5, 33), (4, 4)):
        groups = [list(range(p, n, npat)) for p in range(npat)]
        blocks = [b for g in groups for b in g]
        plans = [p for p, g in enumerate(groups) for _ in g]
        cases += [(blocks, plans), (blocks, None), (blocks, [0] * len(blocks))]
    # a step down that equals the stride in wrapping arithmetic, and equal neighbours
    cases += [([5, 3, 1], None), ([5, 3, 1], [0, 0, 0]), ([4, 4, 4], None), ([0, 2, 4, 2, 4, 6], None),
              ([0, 2 ** 32 - 1, 0], [1, 1, 1]), ([0, 2 ** 40, 2 ** 41, 3], None)]
    res = split(cases)
    for c, g in zip(cases, res):
        _check(c, g)
    assert res[0][0] == 3 and res[1][0] == 3   # one run per pattern, with or without the plan indices
    assert res[12][0] == 3                     # [5], [3], [1]


@pytest.mark.parametrize("with_plans", [False, True])
def test_limit(split, with_plans):
    def runs_of(n):   # n runs of two blocks each: strides alternate
        blocks = []
        for r in range(n):
            blocks += [100 * r, 100 * r + 1 + r % 2]
        return blocks, ([r % 3 for r in range(n) for _ in range(2)] if with_plans else None)
    cases = [runs_of(MAX_SEGS), runs_of(MAX_SEGS + 1), runs_of(3 * MAX_SEGS)]
    res = split(cases)
    for c, g in zip(cases, res):
        _check(c, g)
    assert res[0][0] == MAX_SEGS and len(res[0][1]) == MAX_SEGS      # fits
    assert res[1][0] == MAX_SEGS + 1 and len(res[1][1]) == MAX_SEGS  # does not
    assert res[2][0] == MAX_SEGS + 1                                  # (stopped early)


def test_empty_and_single(split):
    cases = [([], None), ([], []), ([9], None), ([9], [3]), ([0], None), ([2 ** 32 - 1], [65535])]
    res = split(cases)
    for c, g in zip(cases, res):
        _check(c, g)
    assert res[0] == (0, []) and res[1] == (0, [])
    assert res[2] == (1, [(0, 9, 1, 0)]) and res[3] == (1, [(0, 9, 1, 3)])
    assert res[5] == (1, [(0, 2 ** 32 - 1, 1, 65535)])
    assert split([([1, 2], None)], limit=0) == [(1, [])]
