"""Host logic of the ranged read (shmr_amd/csrc/read_plan.hpp) on the CPU:
tools/read_plan_check.cpp is compiled with g++ under ASan + UBSan.

The planner validates a read list, refuses two requests that write the same
destination byte, and splits every request into pieces that tile its byte
range exactly (a byte-granular head up to the next multiple of 16 in the shard,
whole 16-byte chunks, a byte-granular tail).  The kernel finds a tile's piece
by the search over tile prefixes it shares with the update kernel.
"""
import os
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "shmr_amd", "csrc")
CHUNK, TILE, ENTRY = 16, 4096, 40
TABLE = 256 * 1024 // ENTRY
M64 = (1 << 64) - 1
EDGES = [0, 1, 15, 16, 17, 4095, 4096, 4097]


@pytest.fixture(scope="module")
def check(tmp_path_factory):
    exe = str(tmp_path_factory.mktemp("read") / "read_plan_check")
    # (any sanitizer report aborts the checker and fails the test)
    subprocess.run(["g++", "-O1", "-std=c++17", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", CSRC, "-I", os.path.join(ROOT, "include"),
                    os.path.join(ROOT, "tools", "read_plan_check.cpp"), "-o", exe], check=True)

    def run(text):
        return subprocess.run([exe], input=text, capture_output=True, text=True, check=True).stdout.split("\n")
    return run


def plan(check, reads, nblocks=1, k=4, shard_len=1 << 20, dst_bytes=1 << 40):
    """-> None (refused) or (nchunks, pieces); the checker has verified the
    tiling and the tile search itself ("bad ..." otherwise)."""
    text = f"plan {nblocks} {k} {shard_len} {dst_bytes} {len(reads)}\n" + "".join("%d %d %d %d %d\n" % r for r in reads)
    out = check(text)
    if out[0] == "invalid":
        return None
    tag, npieces, nchunks = out[0].split()
    assert tag == "ok", out[0]
    pieces = [dict(zip(("read", "block", "shard", "col", "len", "dst", "vec", "tiles", "tile0"),
                       (int(x) for x in line.split()))) for line in out[1:1 + int(npieces)]]
    assert len(pieces) == int(npieces)
    return int(nchunks), pieces


def test_constants(check):
    assert check("rule\n")[0].split() == ["chunk", str(CHUNK), "tile", str(TILE), "maxpiece", str(1 << 30),
                                          "entry", str(ENTRY), "table", str(TABLE)]


@pytest.mark.parametrize("read,kw", [
    ((3, 0, 0, 1, 0), {}),                               # block >= nblocks
    ((0, 4, 0, 1, 0), {}),                               # shard >= data
    ((0, 0, 0, 0, 0), {}),                               # len == 0
    ((0, 0, 100, 1, 0), {"shard_len": 100}),             # offset + len > shard_len
    ((0, 0, 99, 2, 0), {"shard_len": 100}),
    ((0, 0, 0, 101, 0), {"shard_len": 100}),
    ((0, 0, M64, 2, 0), {"shard_len": 100}),             # offset + len wraps to 1
    ((0, 0, 2, M64, 0), {"shard_len": 100}),
    ((0, 0, M64, M64, 0), {"shard_len": M64}),
    ((0, 0, 0, 8, 93), {"dst_bytes": 100}),              # dst_offset + len > dst_bytes
    ((0, 0, 0, 8, M64), {"dst_bytes": 100}),             # ... wraps to 7
    ((0, 0, 0, 8, M64 - 7), {"dst_bytes": M64}),
    ((0, 0, 0, 8, 0), {"dst_bytes": 7}),
    ((0xffffffff, 0, 0, 8, 0), {}),
    ((0, 0xffffffff, 0, 8, 0), {}),
])
def test_each_validation_error(check, read, kw):
    args = dict(nblocks=3, shard_len=1000, dst_bytes=1000)
    args.update(kw)
    assert plan(check, [read], **args) is None
    # the same list is refused wherever the bad request stands
    good = (1, 1, 0, 1, 6)                               # (inside the smallest destination used above)
    assert plan(check, [good, read], **args) is None
    assert plan(check, [read, good], **args) is None
    assert plan(check, [good], **args) is not None


def test_limits_are_accepted(check):
    """The last byte of a shard, of the destination and of the 64-bit range."""
    assert plan(check, [(2, 3, 999, 1, 999)], nblocks=3, shard_len=1000, dst_bytes=1000) is not None
    assert plan(check, [(0, 0, 0, 1000, 0)], shard_len=1000, dst_bytes=1000) is not None
    nchunks, pieces = plan(check, [(0, 0, M64 - 40, 40, M64 - 40)], shard_len=M64, dst_bytes=M64)
    assert nchunks == 1 and sum(p["len"] for p in pieces) == 40
    assert plan(check, [], nblocks=0) == (0, [])


def test_destination_overlap(check):
    a = (0, 0, 0, 8, 100)
    # touching ranges are fine, on either side
    assert plan(check, [a, (0, 1, 0, 8, 108)]) is not None
    assert plan(check, [a, (0, 1, 0, 8, 92)]) is not None
    # one byte of overlap is refused, on either side and in either list order
    for b in [(0, 1, 0, 8, 107), (0, 1, 0, 8, 93), (0, 1, 50, 1, 100), (0, 1, 50, 1, 107), (0, 3, 0, 1000, 0),
              (0, 0, 0, 8, 100)]:
        assert plan(check, [a, b]) is None, b
        assert plan(check, [b, a]) is None, b
    # ... wherever the pair stands among disjoint requests, whatever the order of the list
    others = [(0, 2, i, 5, 1000 + 5 * i) for i in range(20)]
    bad = (0, 1, 7, 3, 106)
    for cut in (0, 7, 20):
        assert plan(check, others[:cut] + [a] + others[cut:] + [bad]) is None
        assert plan(check, [bad] + others[cut:] + [a] + others[:cut]) is None
        assert plan(check, others[:cut] + [a] + others[cut:]) is not None
    # a long range over a short one that does not follow it in the list
    assert plan(check, [(0, 0, 0, 1000, 0), (0, 1, 0, 8, 2000), (0, 2, 0, 1, 999)]) is None
    # the same SOURCE bytes twice are fine
    assert plan(check, [(0, 0, 0, 64, 0), (0, 0, 0, 64, 64), (0, 0, 32, 64, 128)]) is not None


@pytest.mark.parametrize("off", EDGES)
@pytest.mark.parametrize("n", [1, 15, 16, 17, 4095, 4096, 4097])
def test_pieces_tile_the_request(check, off, n):
    nchunks, pieces = plan(check, [(0, 2, off, n, 77)])
    assert nchunks == 1
    col, dst, tile0 = off, 77, 0
    for p in pieces:
        assert (p["col"], p["dst"], p["shard"], p["block"], p["read"], p["tile0"]) == (col, dst, 2, 0, 0, tile0)
        if p["vec"]:
            assert p["col"] % CHUNK == 0 and p["len"] % CHUNK == 0
        else:
            assert p["len"] < CHUNK and p["col"] // CHUNK == (p["col"] + p["len"] - 1) // CHUNK
        assert p["tiles"] == -(-p["len"] // TILE)
        col += p["len"]
        dst += p["len"]
        tile0 += p["tiles"]
    assert col == off + n
    head, tail = -off % CHUNK, (off + n) % CHUNK
    if n >= head + CHUNK:
        assert [p["vec"] for p in pieces] == [0] * bool(head) + [1] + [0] * bool(tail)
    else:
        assert not any(p["vec"] for p in pieces) and len(pieces) <= 2


def test_large_requests_split_below_the_piece_limit(check):
    nchunks, pieces = plan(check, [(0, 0, 5, (3 << 30) + 100, 0)], shard_len=1 << 40)
    assert all(p["len"] <= 1 << 30 for p in pieces) and len(pieces) == 6
    assert sum(p["len"] for p in pieces) == (3 << 30) + 100 and nchunks == 1


def test_table_chunks(check):
    """A chunk holds one ring slot of entries; tile prefixes restart in every chunk."""
    reads = [(0, 0, 16 * (i % 1000), 16, 16 * i) for i in range(2 * TABLE + 1)]
    nchunks, pieces = plan(check, reads)
    assert nchunks == 3 and len(pieces) == 2 * TABLE + 1
    assert [p["tile0"] for p in pieces] == [i % TABLE for i in range(len(pieces))]
    assert plan(check, reads[:TABLE])[0] == 1 and plan(check, reads[:TABLE + 1])[0] == 2
    # the tiles of a full chunk of the largest pieces are still one grid
    assert TABLE * ((1 << 30) // TILE) < 1 << 31


def test_tile_search(check):
    t0 = [0, 1, 2, 10, 11, 300]
    for tile, want in [(0, 0), (1, 1), (2, 2), (9, 2), (10, 3), (11, 4), (299, 4), (300, 5), (301, 5)]:
        assert int(check("find %d %s %d\n" % (len(t0), " ".join(map(str, t0)), tile))[0]) == want
    assert int(check("find 1 0 9\n")[0]) == 0
    # over the prefixes of a planned list: every tile of every piece
    _, pieces = plan(check, [(0, 0, 3, 9000, 0), (0, 1, 16, 4096, 9000), (0, 2, 0, 1, 13096), (0, 3, 4090, 12300, 13097)])
    t0 = [p["tile0"] for p in pieces]
    for i, p in enumerate(pieces):
        for tile in range(p["tile0"], p["tile0"] + p["tiles"]):
            assert int(check("find %d %s %d\n" % (len(t0), " ".join(map(str, t0)), tile))[0]) == i


@pytest.mark.parametrize("seed", [1, 2])
def test_fuzz_20000_requests(check, seed):
    """A seeded list of 20,000 requests, destinations packed back to back in a
    shuffled order (every neighbour touches): the checker verifies that the
    pieces tile every request, source and destination, and that every chunk's
    tile search finds each piece's first and last tile."""
    out = check(f"fuzz {seed} 20000 64 8 40000\n")
    tag, npieces, nchunks = out[0].split()
    assert tag == "ok", out[0]
    assert int(npieces) >= 20000 and int(nchunks) >= 4
