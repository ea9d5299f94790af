"""Single-shard location in degraded blocks on the GPU (gf_locate.hip's degraded
kernels through shmr_ec_locate_checked_batch_dev), bit-exact against the numpy
reference written from the definition (tests/locate_checked_ref.py) and the
oracle's codewords.

Layout of every batch: B blocks of k + p shards in one device buffer with
sentinel guards in front and behind, a shard pitch above len whose padding holds
random bytes that are no codeword, absent slots filled with a sentinel over
their whole pitch.  Every run also makes the checked reconstruct's call on a
copy of the same buffer: the words must be that call's words and the buffer
that call's buffer, byte for byte, guards and padding included.

Expected answers: a block that was not touched is a codeword, so CLEAN; every
damaged block goes through the reference.
"""
import numpy as np
import pytest

import shmr_amd
from locate_checked_ref import CLEAN, NONE, check_word, locate_checked_ref
from oracle import c_oracle

pytestmark = pytest.mark.gpu

GUARD, SENT, ABSENT = 256, 0xC3, 0xA5


def lost(t, *gone):
    pr = np.ones(t, np.uint8)
    pr[list(gone)] = 0
    return pr


class Batch:
    def __init__(self, k, p, L, present, gpu, odd=False):
        self.k, self.p, self.t, self.L, self.gpu = k, p, k + p, L, gpu
        t = k + p
        self.present = np.array(present, np.uint8).reshape(-1, t)
        self.B = B = len(self.present)
        self.pitch = pitch = (L // 64 + 1) * 64 + (1 if odd else 0)     # above len
        self.off = off = GUARD + (1 if odd else 0)
        rng = np.random.default_rng([k, p, L, B, int(odd)])
        self.img = img = np.full(off + B * t * pitch + GUARD, SENT, np.uint8)
        cw = self.view(img)
        cw[:] = rng.integers(0, 256, cw.shape, dtype=np.uint8)         # padding past len: random, no codeword
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k, :L]), par, B, L, 8)
        cw[:, k:, :L] = par
        self.codeword = img.copy()                                     # every shard in place, nothing damaged
        cw[self.present == 0] = ABSENT
        self.rs = shmr_amd.ReedSolomon(k, p)
        self.damaged = set()

    def view(self, img):
        return img[self.off:self.off + self.B * self.t * self.pitch].reshape(self.B, self.t, self.pitch)

    def dev_view(self, buf):
        import torch
        return torch.as_strided(buf, (self.B, self.t, self.pitch), (self.t * self.pitch, self.pitch, 1), self.off)

    def damage(self, b, shard, col, x=0x41):
        assert self.present[b, shard] and col < self.L
        self.view(self.img)[b, shard, col] ^= x
        self.damaged.add(b)

    def expected(self):
        want = np.full(self.B, CLEAN, np.int32)
        v = self.view(self.img)
        for b in self.damaged:
            want[b] = locate_checked_ref(self.k, self.p, v[b, :, :self.L], self.present[b])
        return want

    def expected_words(self):
        want = np.zeros(self.B, np.uint32)
        v = self.view(self.img)
        for b in self.damaged:
            want[b] = check_word(self.k, self.p, v[b, :, :self.L], self.present[b])
        return want

    def run(self, rebuild=True, data_only=False):
        """-> (words uint32 [B], located int32 [B], the buffer after the call)."""
        import torch
        start = torch.from_numpy(self.img).to(self.gpu)
        buf, ref = start.clone(), start.clone()
        mism, loc = self.rs.locate_checked_batch_dev(self.dev_view(buf), self.present, shard_len=self.L,
                                                     data_only=data_only, rebuild=rebuild)
        words = self.rs.reconstruct_checked_batch_dev(self.dev_view(ref), self.present, shard_len=self.L,
                                                      data_only=data_only, rebuild=rebuild)
        torch.cuda.synchronize()
        assert mism.dtype == torch.int32 and loc.dtype == torch.int32 and mism.shape == loc.shape == (self.B,)
        assert torch.equal(mism, words), "d_mismatch is not the checked reconstruct's word"
        assert torch.equal(buf, ref), "the shards are not what the checked reconstruct leaves"
        if not rebuild:
            assert torch.equal(buf, start), "rebuild=False wrote a byte"
        got = mism.cpu().numpy().view(np.uint32)
        assert np.array_equal(got, self.expected_words()), "d_mismatch is not the reference's word"
        return got, loc.cpu().numpy(), buf

    def masks(self):
        return np.array([self.rs.checked_rows(pr) for pr in self.present], np.uint32)


def _single_damage_batch(gpu, L=4096):
    """RS(4,3): each of the 7 shards absent in turn, each of the 6 survivors
    damaged in turn by one byte; clean degraded blocks and complete blocks
    (clean and damaged) in between, so no pattern's blocks are an arithmetic
    sequence."""
    k, p, t = 4, 3, 7
    present, plan = [], []
    n = 0
    for a in range(t):
        for e in range(t):
            if e == a:
                continue
            present.append(lost(t, a))
            plan.append((len(present) - 1, e))
            n += 1
            if n % 3 == 0:
                present.append(np.ones(t, np.uint8))                    # complete; every other one damaged
                if n % 2 == 0:
                    plan.append((len(present) - 1, n % t))
            if n % 5 == 0:
                present.append(lost(t, (a + 3) % t))                    # degraded and clean
    batch = Batch(k, p, L, present, gpu)
    rng = np.random.default_rng(1)
    for b, e in plan:
        batch.damage(b, e, int(rng.integers(0, L)), x=int(rng.integers(1, 256)))
    return batch, plan


def test_single_damage_every_position_of_rs43(gpu):
    import torch
    batch, plan = _single_damage_batch(gpu)
    words, loc, buf = batch.run()
    want = batch.expected()
    assert [int(want[b]) for b, _ in plan] == [e for _, e in plan]          # the reference names what was damaged
    assert loc.tolist() == want.tolist()
    masks = batch.masks()
    for b, e in plan:
        inputs = np.flatnonzero(batch.present[b])[:4]
        assert words[b] == (masks[b] if e in inputs else 1 << (e - 4)), (b, e)
    clean = sorted(set(range(batch.B)) - batch.damaged)
    assert not words[clean].any() and (loc[clean] == CLEAN).all()
    # complete blocks: locate_batch_dev's answer and word
    start = torch.from_numpy(batch.img).to(gpu)
    m2, l2 = batch.rs.locate_shards_dev(batch.dev_view(start), shard_len=batch.L)
    full = np.flatnonzero(batch.present.all(axis=1))
    assert len(full) >= 10
    assert loc[full].tolist() == l2.cpu().numpy()[full].tolist()
    assert words[full].tolist() == m2.cpu().numpy().view(np.uint32)[full].tolist()
    # rebuilt bytes: reconstruct_batch_dev's for the same batch
    batch.rs.reconstruct_batch_dev(batch.dev_view(start), batch.present, shard_len=batch.L)
    torch.cuda.synchronize()
    assert torch.equal(buf, start)


def test_rebuild_false_writes_nothing_and_answers_the_same(gpu):
    batch, _ = _single_damage_batch(gpu, L=1000)
    want = batch.expected()
    words, loc, _ = batch.run(rebuild=True)
    words2, loc2, _ = batch.run(rebuild=False)                              # (run compares against sentinels and start)
    assert loc.tolist() == want.tolist() == loc2.tolist() and words.tolist() == words2.tolist()
    words3, loc3, _ = batch.run(data_only=True)
    assert loc3.tolist() == want.tolist() and words3.tolist() == words.tolist()


@pytest.mark.parametrize("k,p", [(4, 4), (10, 4)])
def test_three_surplus_two_damaged_in_one_column_is_none(gpu, k, p):
    t, L = k + p, 4096 + 200
    present = [lost(t, 1), lost(t, k + 1), lost(t, 0), lost(t, 1), lost(t, t - 1)]
    batch = Batch(k, p, L, present, gpu)
    batch.damage(0, 0, 77)
    batch.damage(0, 2, 77, x=0x13)                                          # two inputs, one column
    batch.damage(1, 3, 4100)
    batch.damage(1, k + 2, 4100, x=0x99)                                    # an input and a surplus shard
    batch.damage(2, k + 1, 9)
    batch.damage(2, k + 3, 9, x=0x07)                                       # two surplus shards
    batch.damage(3, 2, 500)                                                 # one input: located
    words, loc, _ = batch.run()
    want = batch.expected()
    assert want.tolist() == [NONE, NONE, NONE, 2, CLEAN]
    assert loc.tolist() == want.tolist()
    masks = batch.masks()
    assert words[0] == masks[0] and words[3] == masks[3] and words[4] == 0 and words[2] == (1 << 1) | (1 << 3)


def test_two_surplus_rs83(gpu):
    """s = 2: two survivors damaged in different columns give NONE -- in one
    tile at different lanes, and in different tiles; one survivor damaged in
    two tiles is named."""
    k, p, t, L = 8, 3, 11, 2 * 4096
    present = [lost(t, 3)] * 4 + [lost(t, 9)] * 3
    batch = Batch(k, p, L, present, gpu)
    batch.damage(0, 0, 5)
    batch.damage(0, 6, 40, x=0x22)                                          # one tile, lanes 0 and 2
    batch.damage(1, 1, 5)
    batch.damage(1, 7, 4096 + 7, x=0x22)                                    # tiles 0 and 1
    batch.damage(2, 4, 100)
    batch.damage(2, 4, 4096 + 3000, x=0x77)                                 # one input, both tiles
    batch.damage(3, 2, 2000)
    batch.damage(3, 10, 6000, x=0x05)                                       # an input, and a surplus shard elsewhere
    batch.damage(4, 8, 4095)
    batch.damage(4, 8, 4096, x=0x31)                                        # a surplus shard in both tiles
    batch.damage(5, 7, 8191)                                                # the last byte
    words, loc, _ = batch.run()
    want = batch.expected()
    assert want.tolist() == [NONE, NONE, 4, NONE, 8, 7, CLEAN]
    assert loc.tolist() == want.tolist()
    assert words.tolist() == [6, 6, 6, 6, 1, 5, 0]


def test_one_and_no_surplus_locate_nothing(gpu):
    """RS(4,3) with two absent (s = 1): damage gives a non-zero word and NONE;
    three absent (s = 0): nothing is compared, the answer is CLEAN."""
    t, L = 7, 4096 + 10
    present = [lost(t, 0, 5), lost(t, 0, 5), lost(t, 0, 5), lost(t, 1, 2, 4), lost(t, 1, 2, 4), lost(t, 4, 5, 6)]
    batch = Batch(4, 3, L, present, gpu)
    batch.damage(0, 2, 4100)                                                # an input
    batch.damage(1, 6, 17)                                                  # the surplus shard
    batch.damage(3, 3, 50)                                                  # s = 0: not seen
    words, loc, _ = batch.run()
    assert batch.expected().tolist() == [NONE, NONE, CLEAN, CLEAN, CLEAN, CLEAN]
    assert loc.tolist() == [NONE, NONE, CLEAN, CLEAN, CLEAN, CLEAN]
    assert words.tolist() == [4, 4, 0, 0, 0, 0]


def test_row_groups_rs66(gpu):
    """s = 5: the fifth surplus row lies in the second row group of the check."""
    t, L = 12, 4096 + 300
    present = [lost(t, 0)] * 3 + [lost(t, 7)] * 2
    batch = Batch(6, 6, L, present, gpu)
    batch.damage(0, 11, 4200)                                               # the surplus shard of the second group
    batch.damage(1, 3, 123)                                                 # an input: all five bits
    batch.damage(3, 2, 4096)                                                # an input; parity row 1 absent
    batch.damage(4, 6, 4097)                                                # parity row 0, a surplus shard here
    words, loc, _ = batch.run()
    assert batch.expected().tolist() == [11, 3, CLEAN, 2, 6]
    assert loc.tolist() == [11, 3, CLEAN, 2, 6]
    assert words.tolist() == [1 << 5, 0b111110, 0, 0b111101, 1]


def test_two_bitmap_words_rs403(gpu):
    """RS(40,3), data shard 5 absent: inputs at plan positions 0, 31, 32 and 39."""
    k, p, t, L = 40, 3, 43, 600
    pr = lost(t, 5)
    inputs = np.flatnonzero(pr)[:k]
    batch = Batch(k, p, L, [pr] * 6, gpu)
    for b, pos in enumerate((0, 31, 32, 39)):
        batch.damage(b, int(inputs[pos]), 100 + 7 * b)
    batch.damage(4, 42, 599)
    words, loc, _ = batch.run()
    want = [int(inputs[0]), int(inputs[31]), int(inputs[32]), int(inputs[39]), 42, CLEAN]
    assert want == [0, 32, 33, 40, 42, CLEAN]
    assert batch.expected().tolist() == want
    assert loc.tolist() == want
    assert words.tolist() == [6, 6, 6, 6, 4, 0]


@pytest.mark.parametrize("k,p,odd", [(8, 3, False), (4, 3, False), (8, 3, True), (6, 6, True)])
def test_tails_padding_and_alignment(gpu, k, p, odd):
    """len = 2 * 4096 + 83: full tiles, the partial tile and an odd tail; damage
    at byte len - 1; the pitch padding at and past len is garbage in every
    shard.  odd: the base off by one byte and an odd pitch."""
    t, L = k + p, 2 * 4096 + 83
    present = [lost(t, 1), lost(t, 1), np.ones(t, np.uint8), lost(t, 1), lost(t, k), lost(t, k)]
    batch = Batch(k, p, L, present, gpu, odd=odd)
    batch.damage(0, 0, L - 1)                                               # an input, the last byte
    batch.damage(3, t - 1, L - 1)                                           # a surplus shard, the last byte
    batch.damage(4, 2, 2 * 4096)                                            # the first byte of the partial tile
    batch.damage(2, 3, 4095)
    words, loc, _ = batch.run()
    want = batch.expected()
    assert want.tolist() == [0, CLEAN, 3, t - 1, 2, CLEAN]
    assert loc.tolist() == want.tolist()
    masks = batch.masks()
    assert words.tolist() == [masks[0], 0, masks[2], 1 << (p - 1), masks[4], 0]
    # the padding decides nothing: other garbage, same answers
    v = batch.view(batch.img)
    v[:, :, L:][batch.present == 1] ^= 0x5A
    words2, loc2, _ = batch.run()
    assert loc2.tolist() == want.tolist() and words2.tolist() == words.tolist()


def test_grid_stride(gpu):
    """RS(4,3), 16 KiB shards, 640 blocks: 2,560 tiles, more than the bounded
    grid of the locate launch.  Damage in the first tile of the first block and
    in the last tile of the last."""
    t, L, B = 7, 16384, 640
    batch = Batch(4, 3, L, [lost(t, 1)] * B, gpu)
    batch.damage(0, 0, 3)
    batch.damage(B - 1, 3, L - 1)
    batch.damage(B // 2, 6, 8000)
    words, loc, _ = batch.run()
    want = batch.expected()
    assert want[0] == 0 and want[B - 1] == 3 and want[B // 2] == 6 and (want == CLEAN).sum() == B - 3
    assert loc.tolist() == want.tolist()
    assert words[0] == 6 and words[B - 1] == 6 and words[B // 2] == 4 and np.count_nonzero(words) == 3


def test_block_lists_past_one_chunk(gpu):
    """RS(4,3), len 32, 70,000 blocks: one pattern on all but an irregular
    sprinkling of four others, so its block list is no arithmetic sequence and
    longer than a 65,536-entry chunk.  Damage on both sides of the boundary."""
    t, L, B = 7, 32, 70000
    others = [np.ones(t, np.uint8), lost(t, 0), lost(t, 1, 4), lost(t, 0, 1, 2)]
    rng = np.random.default_rng(5)
    pick = rng.integers(0, 100, B)
    present = np.tile(lost(t, 2), (B, 1))
    for i, pr in enumerate(others):
        present[pick == i] = pr
    main = np.flatnonzero(pick >= len(others))
    assert len(main) > 65536 + 100
    batch = Batch(4, 3, L, present, gpu)
    hits = {}
    for n, pos in enumerate((0, 1, 65534, 65535, 65536, 65537, len(main) - 1)):
        shard = [0, 1, 3, 4, 5, 6][n % 6]
        hits[int(main[pos])] = shard
        batch.damage(int(main[pos]), shard, (5 * n + 1) % L)
    for i in range(len(others) - 1):                                        # and in the sparse patterns
        b = int(np.flatnonzero(pick == i)[-1])
        shard = int(np.flatnonzero(others[i])[1])
        batch.damage(b, shard, 31)
    words, loc, _ = batch.run()
    want = batch.expected()
    for b, shard in hits.items():
        assert want[b] == shard
    assert np.array_equal(loc, want)
    assert np.count_nonzero(words) == len(batch.damaged)


def test_capturing_stream_is_refused(gpu):
    """On a stream that is being captured the call returns InvalidArgument and
    enqueues nothing: the buffer is unchanged, nothing is counted."""
    import torch
    t, L = 11, 4096 + 48
    batch = Batch(8, 3, L, [lost(t, 2), np.ones(t, np.uint8), lost(t, 9)], gpu)
    batch.damage(0, 4, 10)
    _, loc, _ = batch.run()                                                 # device init and plan uploads outside
    assert loc.tolist() == [4, CLEAN, CLEAN]
    start = torch.from_numpy(batch.img).to(gpu)
    buf = start.clone()
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        for rebuild in (True, False):
            with pytest.raises(shmr_amd.Error) as e:
                batch.rs.locate_checked_batch_dev(batch.dev_view(buf), batch.present, shard_len=L, rebuild=rebuild)
            assert e.value.name == "InvalidArgument"
    assert shmr_amd.device_stats(0) == st, "a refused call counted or made a blocking call"
    torch.cuda.synchronize()
    assert torch.equal(buf, start)
    _, loc, _ = batch.run()
    assert loc.tolist() == [4, CLEAN, CLEAN]
