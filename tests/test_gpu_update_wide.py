"""Parity delta update past tests/test_gpu_update.py's small batches: whole
pieces through the byte-granular path, a table-chunk boundary between
multi-tile pieces, and more table chunks in one call than the upload ring has
slots.  Bit-exact against oracle/c_oracle.py through test_gpu_update.Case: the
whole device buffer with guards and non-codeword padding, and src unwritten.

B1  update_on_device keeps kVecFlag on a whole-chunk piece where the device
    serves unaligned vector access, else only where every address of the piece
    is 16-byte aligned.  On an MI355X the probe passes, so update_chunk<false>
    otherwise runs on heads and tails alone: lane 0 of one tile, n < 16.  Under
    the knob uvec = 0 (what a device that fails the probe runs) whole multi-tile
    pieces take it: every lane, every tile, n = 16.
B2  The piece table travels in chunks of 8,192 pieces, each followed by one
    launch per round present in it; the kernel finds a tile's piece through
    tile_base and the pieces' tile prefixes, which restart in every chunk.
B3  33 * 8,192 + 1 pieces are 34 chunks, two more than the ring's 32 slots: a
    slot is taken again while the launch that reads it may still be in flight.
"""
import numpy as np
import pytest

import shmr_amd
from test_gpu_update import Case, _case, shapes

pytestmark = pytest.mark.gpu

# ---- the product constants under test, mirrored once ----------------------------
TABLE_CHUNK = 256 * 1024 // 32   # update_plan.hpp   update::kTablePieces: one ring slot of 32-byte pieces
RING_SLOTS = 32                  # ec_core.hpp        UploadRing::kSlots
CHUNK = 16                       # piece_plan.hpp     piece::kChunk
TILE = 256 * CHUNK               # piece_plan.hpp     piece::kTileBytes


def _piece_lens(offset, n):
    """piece_plan.hpp split(): a byte-granular head up to the next multiple
    of 16, the whole chunks (one piece: every length here is far below
    kMaxPieceBytes), a byte-granular tail."""
    out = []
    head = min(n, -offset % CHUNK)
    if head:
        out.append(head)
    whole = (n - head) // CHUNK * CHUNK
    if whole:
        out.append(whole)
    if n - head - whole:
        out.append(n - head - whole)
    return out


def _launches(ups, round_of):
    """One launch per round per table chunk: the pieces in ascending round,
    stable in update order, cut every TABLE_CHUNK pieces.  -> (launches, the
    (update index, length) of every piece in table order)."""
    pieces = [(int(round_of[i]), i, n) for i, u in enumerate(ups) for n in _piece_lens(u[2], u[3])]
    pieces.sort(key=lambda x: x[0])                                # stable
    launches = sum(len({r for r, _, _ in pieces[c0:c0 + TABLE_CHUNK]}) for c0 in range(0, len(pieces), TABLE_CHUNK))
    return launches, [(i, n) for _, i, n in pieces]


# ---- B1 --------------------------------------------------------------------------
@pytest.fixture
def byte_path():
    """As a device that failed the unaligned-access probe (knob uvec = 0)."""
    shmr_amd.set_tuning(uvec=0)
    try:
        yield
    finally:
        shmr_amd.set_tuning(uvec=-2)


@pytest.mark.parametrize("shift", [0, 3], ids=["aligned_base", "base_off_by_3"])
@pytest.mark.parametrize("L", [1000, 4096 + 48, 12288 - 16])
@pytest.mark.parametrize("k,p", [(8, 3), (3, 9), (2, 1)])
def test_whole_pieces_on_the_byte_path(gpu, byte_path, k, p, L, shift):
    """Every write shape of tests/test_gpu_update.py under uvec = 0.  With the
    base off alignment every piece goes byte by byte.  With aligned bases both
    arms of the source-alignment test run: "src = offset (mod 16)" keeps the
    vector flag on its whole-chunk pieces, "src 3 vs offset 13" loses it.  On a
    device that serves unaligned vector access that decision cannot be seen in
    results -- either path gives the same bytes; only the byte path it selects
    can, and that is what is compared here."""
    c = _case((k, p, L, shift), gpu)
    assert c.data.data_ptr() % 16 == shift and c.parity.data_ptr() % 16 == shift
    multi_tile = 0
    for what, (writes, residue) in shapes(k, L).items():
        ups, src = c.place(writes, residue)
        # whole-chunk pieces above one tile whose addresses are off alignment (the piece starts behind the head)
        multi_tile += sum(1 for _, _, off, n, so in ups for m in _piece_lens(off, n)
                          if m > TILE and (shift or (so + -off % CHUNK) % CHUNK))
        c.apply(ups, src, what)
    assert multi_tile or L <= TILE, "no whole multi-tile piece took the byte path"


# ---- B2 --------------------------------------------------------------------------
def _boundary_updates(c, two_rounds):
    """TABLE_CHUNK - 1 one-byte updates at distinct columns of blocks 0, 2, 4;
    whole-shard updates (three tiles each) of blocks 1 and 3; a few more
    one-byte updates.  two_rounds: the same columns again in a second shard of
    blocks 1 and 3.  (A whole-shard update at column 0 is a single piece, so
    8,191 pieces in front of the first put the chunk boundary between the two;
    the pairs stand next to each other, so whichever of a pair takes round 0,
    table entries 8,191 and 8,192 are whole-shard pieces of blocks 1 and 3.)"""
    k, L = c.k, c.L
    rng = np.random.default_rng(8191)
    n1 = TABLE_CHUNK - 1 + 5
    per = -(-n1 // 3)
    assert per <= L
    ones = [(b, int(rng.integers(0, k)), int(col), 1) for b in (0, 2, 4) for col in rng.choice(L, per, replace=False)]
    ones = [ones[i] for i in rng.permutation(len(ones))][:n1]
    whole = [(1, 2, 0, L), (3, k - 1, 0, L)]
    if two_rounds:
        whole = [(1, 2, 0, L), (1, 5, 0, L), (3, k - 1, 0, L), (3, 0, 0, L)]
    return ones[:TABLE_CHUNK - 1] + whole + ones[TABLE_CHUNK - 1:]


@pytest.mark.parametrize("two_rounds", [False, True], ids=["one_round", "two_rounds"])
def test_chunk_boundary_between_multi_tile_pieces(gpu, two_rounds):
    """RS(8,3), len 12288 - 16.  In table order piece 8,191 (the last of chunk
    0) and piece 8,192 (the first of chunk 1) are whole-shard pieces of three
    tiles each.  One round: two launches.  Two rounds: chunk 1 also holds the
    two pieces of round 1, behind round 0's -- their launch starts at a
    non-zero tile_base."""
    k, p, L = 8, 3, 12288 - 16
    c = _case((k, p, L, 0), gpu)
    ups, src = c.place(_boundary_updates(c, two_rounds), 3)
    round_of, nrounds = c.rs.update_rounds(ups, c.B, L, len(src))
    assert nrounds == (2 if two_rounds else 1)
    if two_rounds:                                            # each pair of whole-shard updates: rounds 0 and 1
        at = TABLE_CHUNK - 1
        assert sorted(round_of[at:at + 2]) == [0, 1] and sorted(round_of[at + 2:at + 4]) == [0, 1]
        assert int(round_of.sum()) == 2
    launches, table = _launches(ups, round_of)
    assert len(table) == len(ups) and launches == (3 if two_rounds else 2)
    (i0, n0), (i1, n1) = table[TABLE_CHUNK - 1], table[TABLE_CHUNK]
    assert n0 == n1 == L and -(-L // TILE) == 3 and ups[i0][0] == 1 and ups[i1][0] == 3
    assert all(n == 1 for _, n in table[:TABLE_CHUNK - 1])
    shmr_amd.device_init(0)
    st = shmr_amd.device_stats(0)
    c.apply(ups, src, "chunk boundary")
    now = shmr_amd.device_stats(0)
    assert now["launches"] - st["launches"] == launches


# ---- B3 --------------------------------------------------------------------------
def test_more_chunks_than_ring_slots(gpu):
    """RS(8,3), len 1000, 40 blocks: 270,337 one-byte updates drawn without
    replacement, the new bytes in another order than the updates, the list an
    int64 array.  Two calls with no synchronisation in between, the second with
    fresh bytes over the first's result; then one image comparison, and verify
    finds every block a codeword.  (Nothing about blocking_calls: whether a
    slot is ready when it comes round again is timing.)"""
    import torch
    k, p, L, blocks = 8, 3, 1000, 40
    n = (RING_SLOTS + 1) * TABLE_CHUNK + 1
    assert -(-n // TABLE_CHUNK) == RING_SLOTS + 2 and n <= blocks * k * L
    c = Case(k, p, L, gpu, seed=33, blocks=blocks)
    rng = np.random.default_rng(33)
    flat = rng.choice(blocks * k * L, size=n, replace=False)
    ups = np.stack([flat // (k * L), flat // L % k, flat % L, np.ones(n, np.int64), rng.permutation(n)],
                   axis=1).astype(np.int64)
    src1 = rng.integers(0, 256, n, dtype=np.uint8)
    src2 = rng.integers(0, 256, n, dtype=np.uint8)
    s1, s2 = torch.from_numpy(src1).to(gpu), torch.from_numpy(src2).to(gpu)
    c.reset()
    torch.cuda.synchronize()
    c.rs.update_batch_dev(c.data, c.parity, ups, s1, shard_len=L)
    c.rs.update_batch_dev(c.data, c.parity, ups, s2, shard_len=L)
    words = c.rs.verify_batch_dev(c.data, c.parity, shard_len=L)
    torch.cuda.synchronize()
    rows = ups.tolist()
    want = c.expected(rows, src2, start=c.expected(rows, src1))
    got = c.buf.cpu().numpy()
    bad = np.flatnonzero(got != want)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0])} " \
                          f"(data region at {c.data_off}, parity region at {c.par_off}, pitch {c.pitch})"
    assert not words.cpu().numpy().any()
    assert np.array_equal(s1.cpu().numpy(), src1) and np.array_equal(s2.cpu().numpy(), src2), "src was written"
