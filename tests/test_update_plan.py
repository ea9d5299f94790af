"""Host logic of the parity delta update (shmr_amd/csrc/update_plan.hpp) on the
CPU: tools/update_plan_check.cpp is compiled with g++ under ASan + UBSan.

The planner validates an update list, splits every update into pieces that tile
its byte range exactly (a byte-granular head up to the next multiple of 16,
whole 16-byte chunks, a byte-granular tail) and assigns every update a round.
The kernel rewrites parity bytes in place, so no round may hold two pieces of a
block whose store footprints intersect.  This build's footprint rule is
byte-exact (the checker prints it): a piece stores exactly the parity columns
of its byte range, so ranges that merely share a 16-byte chunk share a round.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")
CHUNK, TILE = 16, 4096


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("update") / "update_plan_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "update_plan_check.cpp"), "-o", exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return run


@pytest.fixture(scope="module")
def byte_exact(check):
    out = check("rule\n")
    assert out[0] in ("edges byte-exact", "edges widened")
    assert out[1].split()[:4] == ["chunk", str(CHUNK), "tile", str(TILE)]
    return out[0] == "edges byte-exact"


def plan(check, updates, nblocks=1, k=4, shard_len=1 << 20, src_bytes=1 << 40):
    """-> None (refused) or (nrounds, round_of, pieces); the checker has verified
    the tiling and the footprint property itself ("bad ..." otherwise)."""
    text = f"plan {nblocks} {k} {shard_len} {src_bytes} {len(updates)}\n" + "".join(
        "%d %d %d %d %d\n" % u for u in updates)
    out = check(text)
    if out[0] == "invalid":
        return None
    tag, nrounds, npieces = out[0].split()
    assert tag == "ok", out[0]
    rounds = [int(x) for x in out[1].split()]
    pieces = [dict(zip(("update", "block", "shard", "col", "len", "src", "round", "vec", "tiles"),
                       (int(x) for x in line.split()))) for line in out[2:2 + int(npieces)]]
    assert len(rounds) == len(updates) and len(pieces) == int(npieces)
    return int(nrounds), rounds, pieces


M64 = (1 << 64) - 1


@pytest.mark.parametrize("update,kw", [
    ((3, 0, 0, 1, 0), {}),                               # block >= nblocks
    ((0, 4, 0, 1, 0), {}),                               # shard >= data
    ((0, 0, 0, 0, 0), {}),                               # len == 0
    ((0, 0, 100, 1, 0), {"shard_len": 100}),             # offset + len > shard_len
    ((0, 0, 99, 2, 0), {"shard_len": 100}),
    ((0, 0, 0, 101, 0), {"shard_len": 100}),
    ((0, 0, M64, 2, 0), {"shard_len": 100}),             # offset + len wraps to 1
    ((0, 0, 2, M64, 0), {"shard_len": 100}),
    ((0, 0, M64, M64, 0), {"shard_len": M64}),
    ((0, 0, 0, 8, 93), {"src_bytes": 100}),              # src_offset + len > src_bytes
    ((0, 0, 0, 8, M64), {"src_bytes": 100}),             # ... wraps to 7
    ((0, 0, 0, 8, M64 - 7), {"src_bytes": M64}),
    ((0, 0, 0, 8, 0), {"src_bytes": 7}),
    ((0xffffffff, 0, 0, 8, 0), {}),
    ((0, 0xffffffff, 0, 8, 0), {}),
])
def test_each_validation_error(check, update, kw):
    args = dict(nblocks=3, shard_len=1000, src_bytes=1000)
    args.update(kw)
    assert plan(check, [update], **args) is None
    # the same list is refused wherever the bad update stands
    good = (1, 1, 0, 1, 0)
    assert plan(check, [good, update], **args) is None
    assert plan(check, [good], **args) is not None


def test_limits_are_accepted(check):
    """The last byte of a shard, of the source and of the 64-bit range."""
    assert plan(check, [(2, 3, 999, 1, 999)], nblocks=3, shard_len=1000, src_bytes=1000) is not None
    assert plan(check, [(0, 0, 0, 1000, 0)], shard_len=1000, src_bytes=1000) is not None
    nr, rounds, pieces = plan(check, [(0, 0, M64 - 40, 40, M64 - 40)], shard_len=M64, src_bytes=M64)
    assert nr == 1 and sum(p["len"] for p in pieces) == 40
    assert plan(check, [], nblocks=0) == (0, [], [])


def test_intersecting_writes_to_one_shard_are_refused(check):
    assert plan(check, [(0, 0, 0, 8, 0), (0, 0, 7, 8, 8)]) is None
    assert plan(check, [(0, 0, 0, 100, 0), (0, 1, 0, 100, 0), (0, 0, 99, 1, 0)]) is None
    assert plan(check, [(0, 0, 50, 1, 0), (0, 0, 0, 100, 0)]) is None
    assert plan(check, [(0, 0, 5, 1, 0), (0, 0, 5, 1, 1)]) is None
    # the same bytes of another shard or another block are another matter
    assert plan(check, [(0, 0, 0, 8, 0), (0, 1, 7, 8, 8)]) is not None
    assert plan(check, [(0, 0, 0, 8, 0), (1, 0, 7, 8, 8)], nblocks=2) is not None
    assert plan(check, [(0, 0, 0, 8, 0), (0, 0, 8, 8, 8)]) is not None


@pytest.mark.parametrize("off,n", [(0, 1), (15, 1), (16, 1), (5, 4), (0, 16), (1, 16), (13, 4096 + 6), (0, 4096),
                                   (16, 12288 - 16), (7, 9), (7, 10), (3, 60000), (4090, 12)])
def test_pieces_tile_the_update(check, off, n):
    nr, rounds, pieces = plan(check, [(0, 2, off, n, 77)])
    assert nr == 1 and rounds == [0]
    col, src = off, 77
    for p in pieces:
        assert (p["col"], p["src"], p["shard"], p["block"], p["update"]) == (col, src, 2, 0, 0)
        if p["vec"]:
            assert p["col"] % CHUNK == 0 and p["len"] % CHUNK == 0
        else:
            assert p["len"] < CHUNK and p["col"] // CHUNK == (p["col"] + p["len"] - 1) // CHUNK
        assert p["tiles"] == -(-p["len"] // TILE)
        col += p["len"]
        src += p["len"]
    assert col == off + n
    head, tail = -off % CHUNK, (off + n) % CHUNK
    if n >= head + CHUNK:
        assert [p["vec"] for p in pieces] == [0] * bool(head) + [1] + [0] * bool(tail)


def test_large_updates_split_below_the_piece_limit(check):
    nr, rounds, pieces = plan(check, [(0, 0, 5, (3 << 30) + 100, 0)], shard_len=1 << 40)
    assert nr == 1 and all(p["len"] <= 1 << 30 for p in pieces) and len(pieces) == 6
    assert sum(p["len"] for p in pieces) == (3 << 30) + 100


def test_rounds_on_one_block(check, byte_exact):
    L = 5000
    # disjoint inputs: one round
    nr, rounds, _ = plan(check, [(0, 0, 0, 100, 0), (0, 1, 100, 100, 0), (0, 2, 4096, 904, 0), (0, 0, 200, 3, 0)])
    assert nr == 1 and rounds == [0, 0, 0, 0]
    # neighbours inside one 16-byte chunk: disjoint bytes, one round iff the edge stores are byte-exact
    want = 1 if byte_exact else 2
    nr, rounds, _ = plan(check, [(0, 0, 0, 8, 0), (0, 0, 8, 8, 8)])
    assert nr == want and len(set(rounds)) == want
    nr, rounds, _ = plan(check, [(0, 0, 5, 4, 0), (0, 1, 9, 14, 4)])
    assert nr == want and len(set(rounds)) == want
    # two shards over the same columns: two rounds
    nr, rounds, _ = plan(check, [(0, 0, 0, L, 0), (0, 1, 0, L, L)], shard_len=L)
    assert nr == 2 and sorted(rounds) == [0, 1]
    # all k shards over [0, L): k rounds
    for k in (2, 4, 8, 10):
        nr, rounds, _ = plan(check, [(0, s, 0, L, s * L) for s in range(k)], k=k, shard_len=L)
        assert nr == k and sorted(rounds) == list(range(k))
    # one byte of overlap is enough; the same ranges in other blocks are free
    nr, rounds, _ = plan(check, [(0, 0, 0, 101, 0), (0, 1, 100, 100, 0)])
    assert nr == 2
    nr, rounds, _ = plan(check, [(b, s, 0, L, 0) for b in range(3) for s in range(2)], nblocks=3, shard_len=L)
    assert nr == 2 and rounds == [0, 1, 0, 1, 0, 1]


def test_round_count_is_the_deepest_overlap(check):
    """A staircase: ranges [i*10, i*10 + 25) of shards i % 4 overlap three deep."""
    ups = [(0, i % 4, i * 10, 25, 0) for i in range(40)]
    nr, rounds, _ = plan(check, ups)
    assert nr == 3
    for i in range(40):
        for j in range(i + 1, 40):
            if j * 10 < i * 10 + 25:
                assert rounds[i] != rounds[j], (i, j)
    # the input order does not matter
    nr2, rounds2, _ = plan(check, ups[::-1])
    assert nr2 == 3


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_20000_updates(check, seed):
    """A seeded list of 20,000 updates (distinct 64-column slots of 64 blocks x
    8 shards, a random sub-range each): the checker verifies that the pieces
    tile every update and that no round holds two pieces of a block with
    intersecting footprints; up to 8 shards overlap in a slot."""
    out = check(f"fuzz {seed} 20000 64 8 4096\n")
    tag, nrounds, npieces = out[0].split()
    assert tag == "ok", out[0]
    assert 2 <= int(nrounds) <= 8 and int(npieces) >= 20000


def chunks(check, updates, **kw):
    """-> the sizes of the table chunks the planned pieces travel in."""
    args = dict(nblocks=1, k=4, shard_len=1 << 20, src_bytes=1 << 40)
    args.update(kw)
    text = "chunks {nblocks} {k} {shard_len} {src_bytes} ".format(**args) + f"{len(updates)}\n" + "".join(
        "%d %d %d %d %d\n" % u for u in updates)
    out = check(text)[0].split()
    assert out[0] == "ok", out
    return [int(x) for x in out[1:]]


def test_table_chunks(check):
    """A chunk holds one ring slot of 32-byte entries (8192) and fewer than 2^31
    tiles: 8192 pieces of the largest size are exactly 2^31 tiles, one too many
    for a launch's grid, so the last piece takes a chunk of its own."""
    table, maxpiece = 256 * 1024 // 32, 1 << 30
    assert table * (maxpiece // TILE) == 1 << 31
    big = dict(nblocks=table + 1, shard_len=maxpiece, src_bytes=maxpiece)
    assert chunks(check, [(b, 0, 0, maxpiece, 0) for b in range(table)], **big) == [table - 1, 1]
    assert chunks(check, [(b, 0, 0, 4096, 0) for b in range(table)], **big) == [table]
    assert chunks(check, [(b, 0, 0, 4096, 0) for b in range(table + 1)], **big) == [table, 1]
    assert chunks(check, [], nblocks=0) == []


def test_tile_search(check):
    t0 = [0, 1, 2, 10, 11, 300]
    for tile, want in [(0, 0), (1, 1), (2, 2), (9, 2), (10, 3), (11, 4), (299, 4), (300, 5), (301, 5)]:
        assert int(check("find %d %s %d\n" % (len(t0), " ".join(map(str, t0)), tile))[0]) == want
    assert int(check("find 1 7 9\n")[0]) == 0
