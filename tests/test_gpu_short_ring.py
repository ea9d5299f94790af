"""The compare tile's peeled depth-2 ring (gf_syndrome.hpp syndrome_tile, the
ring of gf_tile.hpp ring2_peeled) at the two shapes no other code reaches: no loop
with a one-shard tail (k = 1) and no loop with a two-shard tail (k = 2).  The
codes of the other suites (k = 3, 4, 5, 8, 10) all enter the loop.
ReedSolomon(1, p) is accepted by the constructor, so both run.

RS(k, 2) is one row group of two rows, RS(k, 5) a full group of four and one
of a single row.  3 blocks of shard_len = 4096 + 16 + 5: one full 4 KiB tile,
then a tail of one whole 16-byte chunk and one partial one.  Two layouts: the
aligned pitch layout (shard pitch above shard_len, the padding random bytes
that are no codeword) and the packed block at an odd base address that
tests/test_gpu_verify.py test_misaligned_packed_block uses (shard i at i * S).

Through the parity check, the checked reconstruct and the location, against
the CPU oracle (oracle.c_oracle).
"""
import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle

pytestmark = pytest.mark.gpu

B = 3
L = 4096 + 16 + 5
GUARD, SENT = 256, 0xC3
FLIP = 0x41


def _bit(r):
    return 1 << min(r, 31)


class Blocks:
    """B codewords of RS(k, p), every shard of a block side by side."""

    def __init__(self, k, p, packed, gpu):
        import torch
        self.k, self.p, self.t = k, p, k + p
        self.pitch = L if packed else (L // 64 + 1) * 64
        self.off = GUARD + 1 if packed else GUARD
        t, pitch = self.t, self.pitch
        rng = np.random.default_rng(1000 * k + 10 * p + packed)
        img = np.full(self.off + B * t * pitch + GUARD, SENT, np.uint8)
        blocks = img[self.off:self.off + B * t * pitch].reshape(B, t, pitch)
        blocks[:] = rng.integers(0, 256, blocks.shape, dtype=np.uint8)      # the padding too
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(blocks[:, :k, :L]), par, B, L, 8)
        blocks[:, k:, :L] = par
        self.img = img
        self.buf = torch.from_numpy(img.copy()).to(gpu)
        self.shards = torch.as_strided(self.buf, (B, t, pitch), (t * pitch, pitch, 1), self.off)
        assert self.shards.data_ptr() % 16 == (1 if packed else 0)
        self.rs = shmr_amd.ReedSolomon(k, p)

    def host(self):
        """The pristine blocks [B, t, pitch] (a view of the host image)."""
        return self.img[self.off:self.off + B * self.t * self.pitch].reshape(B, self.t, self.pitch)

    def want_words(self, flips):
        """The oracle's verify words after the flips [(block, shard, col)]."""
        k, p = self.k, self.p
        cw = self.host()[:, :, :L].copy()
        for b, s, col in flips:
            cw[b, s, col] ^= FLIP
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k]), par, B, L, 8)
        return [sum(_bit(r) for r in range(p) if not np.array_equal(par[b, r], cw[b, k + r])) for b in range(B)]

    def flip(self, flips):
        for b, s, col in flips:
            self.shards[b, s, col] ^= FLIP

    def words(self, t):
        return t.cpu().numpy().view(np.uint32).tolist()

    def unchanged(self):
        return np.array_equal(self.buf.cpu().numpy(), self.img)


CASES = [(k, p, packed) for k in (1, 2) for p in (2, 5) for packed in (False, True)]
IDS = ["k%d-p%d-%s" % (k, p, "packed" if packed else "pitch") for k, p, packed in CASES]


@pytest.fixture(params=CASES, ids=IDS)
def blocks(request, gpu):
    k, p, packed = request.param
    return Blocks(k, p, packed, gpu)


def test_verify_words_are_the_oracles(blocks):
    c, k, t = blocks, blocks.k, blocks.t
    assert c.words(c.rs.verify_shards_dev(c.shards, shard_len=L)) == [0] * B
    # the first byte, the last byte, a data shard, a parity shard
    for flips in ([(0, 0, 0)], [(1, k - 1, L - 1)], [(2, k, 0)], [(0, t - 1, L - 1)], [(1, k - 1, 4096 + 16)],
                  [(2, 0, 4095), (2, k + 1, 4096)]):
        want = c.want_words(flips)
        assert any(want)
        c.flip(flips)
        got = c.words(c.rs.verify_shards_dev(c.shards, shard_len=L))
        c.flip(flips)
        assert got == want, (flips, got, want)
    assert c.unchanged(), "verify wrote a byte"


def test_checked_reconstruct_rebuilds_and_reports(blocks):
    """Data shard 0 absent: the inputs are the next k present shards, the
    surplus shards the parity rows behind them."""
    c, k, p, t = blocks, blocks.k, blocks.p, blocks.t
    present = np.ones((B, t), np.uint8)
    present[:, 0] = 0
    first_surplus = k + 1                      # shards 1 .. k are the k inputs
    surplus_rows = list(range(first_surplus - k, p))

    def run(flips):
        c.shards[:, 0, :L] = 0x99              # the absent shard's slot holds junk
        c.flip(flips)
        got = c.words(c.rs.reconstruct_checked_batch_dev(c.shards, present, shard_len=L))
        c.flip(flips)
        return got

    assert run([]) == [0] * B
    assert c.unchanged(), "the rebuilt shard differs, or a byte outside it was written"
    for row, col in ((surplus_rows[0], 0), (surplus_rows[-1], L - 1), (surplus_rows[-1], 4096 + 16)):
        got = run([(1, k + row, col)])
        assert got == [0, _bit(row), 0], (row, col, got)
        assert c.unchanged(), "a flipped surplus shard reached the rebuilt bytes"


def test_locate_names_the_flipped_data_shard(blocks):
    c, k = blocks, blocks.k
    for b, shard, col in ((0, 0, 0), (1, k - 1, L - 1), (2, 0, 4096 + 16)):
        c.flip([(b, shard, col)])
        words, located = c.rs.locate_shards_dev(c.shards, shard_len=L)
        c.flip([(b, shard, col)])
        want = [-1] * B
        want[b] = shard
        assert located.cpu().numpy().tolist() == want, (b, shard, col)
        assert c.words(words) == c.want_words([(b, shard, col)])
    assert c.unchanged(), "locate wrote a byte"


def test_bytes_past_shard_len_take_no_part(blocks):
    """Damage in the shard padding (pitch layout) or, in the packed layout, at
    a shorter shard_len in the bytes behind it, changes no answer and is not
    written over."""
    c, k, p, t = blocks, blocks.k, blocks.p, blocks.t
    n = L if c.pitch > L else L - 3            # packed: the last 3 bytes of every shard are "past the end"
    flips = [(b, s, col) for b in range(B) for s in range(t) for col in (n, c.pitch - 1)]
    c.flip(flips)
    try:
        held = c.buf.clone()
        assert c.words(c.rs.verify_shards_dev(c.shards, shard_len=n)) == [0] * B
        words, located = c.rs.locate_shards_dev(c.shards, shard_len=n)
        assert c.words(words) == [0] * B and located.cpu().numpy().tolist() == [-1] * B
        present = np.ones((B, t), np.uint8)
        present[:, 0] = 0
        assert c.words(c.rs.reconstruct_checked_batch_dev(c.shards, present, shard_len=n)) == [0] * B
        import torch
        assert torch.equal(c.buf, held), "a byte was written: the rebuilt shard differs, or bytes past shard_len"
    finally:
        c.flip(flips)
