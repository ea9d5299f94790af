"""Parity delta update of degraded device-resident blocks on the GPU
(gf_update_degraded.hip through shmr_ec_update_degraded_batch_dev) against the
CPU oracle.

Every expected byte comes from oracle/c_oracle.py.  For a stored image and its
presence flags: ``old`` = the oracle's first-k-present reconstruct of the data,
``new`` = ``old`` with the writes applied, and the present shards must become
``stored ^ cw(old) ^ cw(new)``, cw(x) the oracle's encode of data x.  For blocks
that hold codewords that is cw(new) itself, which the helper asserts.  The
comparison is bit-exact and covers the whole device buffer: the absent slots
keep their poison bytes, the pitch padding past S, the guards and the other
blocks keep theirs.

Shapes: shard_len = 4117 is one full 4 KiB tile, one more 16-byte chunk and a
5-byte tail.  The aligned layout has a shard pitch of 4128 on a 16-byte aligned
base; the packed layout has shard_pitch = shard_len (odd) on a base off by one.
Five blocks with five presence patterns share every call, one of them whole.
The piece table travels in chunks of 5,461 pieces (one 256 KiB slot of the
upload ring, 48 bytes a piece).
"""
import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle

pytestmark = pytest.mark.gpu

S = 4117
GUARD, SENT, POISON = 256, 0xC3, 0xEE
OFFSETS = [0, 1, 15, 16, 17, 4096, 4097]            # and shard_len - len
LENGTHS = [1, 15, 16, 17, 4096, 4101, S]
CODES = [(4, 2), (8, 3), (10, 4), (5, 5), (3, 9), (2, 34)]
TABLE_CHUNK = 256 * 1024 // 48


def patterns_of(k, p):
    """all present; a lost data shard; lost parity shards (rows 0 and p - 1, and
    31, 32, 33 where the code has them); data and parity lost together; p lost,
    as many data shards among them as there are -- every survivor is an input
    then, parity shards among the inputs."""
    t = k + p

    def drop(*idx):
        assert len(set(idx)) <= p
        return [0 if i in idx else 1 for i in range(t)]
    par = [k + r for r in sorted({0, 31, 32, 33, p - 1}) if r < p]
    nd = min(k, p)
    return [drop(), drop(min(1, k - 1)), drop(*par), drop(k - 1, *par[:max(1, min(len(par), p - 1))]),
            drop(*range(nd), *range(k, k + p - nd))]


def cw(k, p, data):
    """Oracle codewords [B, t, S] of data [B, k, S]."""
    B = data.shape[0]
    data = np.ascontiguousarray(data)
    parity = np.zeros((B, p, data.shape[2]), np.uint8)
    c_oracle.encode_batch(k, p, data, parity, B, data.shape[2], 4)
    return np.concatenate([data, parity], axis=1)


def first_k_data(k, p, stored, present):
    """The data [B, k, S] the oracle's data-only reconstruct leaves: the first
    k present shards are the inputs, whatever the absent slots hold."""
    work = np.ascontiguousarray(stored).copy()
    c_oracle.reconstruct_batch(k, p, work, present, work.shape[2], 4, data_only=True)
    return work[:, :k].copy()


class Case:
    """Blocks of one codec and pattern list on the device: `packed` = shard pitch
    S on a base off by one, else pitch 4128 on a 16-byte aligned base.  Absent
    slots hold `fill` (a byte, or (seed,) for random bytes), the pitch padding
    SENT.  `img` follows the device image: it is what the buffer must hold."""

    def __init__(self, k, p, patterns, gpu, packed=False, fill=POISON, seed=7, damage=()):
        import torch
        self.k, self.p, self.t, self.gpu, self.packed = k, p, k + p, gpu, packed
        self.present = np.array(patterns, dtype=np.uint8)
        self.B = len(patterns)
        rng = np.random.default_rng(seed)
        self.rng = rng
        full = cw(k, p, rng.integers(0, 256, (self.B, k, S), dtype=np.uint8))
        for b, i, col, x in damage:                                     # flips in survivors
            assert self.present[b, i]
            full[b, i, col] ^= x
        self.codewords = not damage
        self.pitch = S if packed else 4128
        self.off = GUARD + (1 if packed else 0)
        self.span = self.B * self.t * self.pitch
        img = np.full(self.off + self.span + GUARD, SENT, np.uint8)
        v = self.view(img)
        v[:, :, :S] = full
        if isinstance(fill, int):
            v[self.present == 0] = fill
        else:
            v[self.present == 0] = np.random.default_rng(fill[0]).integers(0, 256, self.pitch, dtype=np.uint8)
        self.img = img
        self.buf = torch.from_numpy(img.copy()).to(gpu)
        assert self.buf.data_ptr() % 16 == 0
        self.shards = self.buf[self.off:self.off + self.span].view(self.B, self.t, self.pitch)
        self.rs = shmr_amd.ReedSolomon(k, p)

    def view(self, img):
        return img[self.off:self.off + self.span].reshape(self.B, self.t, self.pitch)

    def place(self, writes, start=5, gap=3):
        """[(block, shard, offset, len)] -> (updates with src offsets `gap` bytes
        apart, the new bytes)."""
        ups, pos = [], start
        for b, s, off, n in writes:
            ups.append((b, s, off, n, pos))
            pos += n + gap
        return ups, self.rng.integers(0, 256, pos + 7, dtype=np.uint8)

    def expected(self, ups, src):
        """(image, new data) after the updates, from self.img."""
        k, p = self.k, self.p
        img = self.img.copy()
        v = self.view(img)
        stored = v[:, :, :S].copy()
        old = first_k_data(k, p, stored, self.present)
        new = old.copy()
        for b, s, off, n, so in ups:
            new[b, s, off:off + n] = src[so:so + n]
        cw_old, cw_new = cw(k, p, old), cw(k, p, new)
        there = self.present.astype(bool)
        want = stored ^ cw_old ^ cw_new
        if self.codewords:
            assert np.array_equal(stored[there], cw_old[there])         # the image held punctured codewords
            assert np.array_equal(want[there], cw_new[there])
        stored[there] = want[there]
        v[:, :, :S] = stored
        return img, new

    def apply(self, ups, src, what):
        """The call; checks every byte of the buffer and that src is unchanged.
        The device image is carried forward as self.img."""
        import torch
        src_t = torch.from_numpy(src).to(self.gpu)
        self.rs.update_degraded_batch_dev(self.shards, self.present, ups, src_t, shard_len=S)
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        want, new = self.expected(ups, src)
        bad = np.flatnonzero(got != want)
        if bad.size:
            at = int(bad[0]) - self.off
            where = divmod(at, self.pitch) if 0 <= at < self.span else None
            where = (where[0] // self.t, where[0] % self.t, where[1]) if where else "a guard"
            raise AssertionError(f"{what}: {bad.size} bytes differ, first at (block, shard, column) {where}")
        assert np.array_equal(src_t.cpu().numpy(), src), f"{what}: src was written"
        self.img = want
        return new

    def reset(self, img):
        import torch
        self.img = img.copy()
        self.buf.copy_(torch.from_numpy(self.img))


def grid():
    """Every (offset, len) of the alignment grid that fits."""
    return [(off, n) for n in LENGTHS for off in sorted(set(OFFSETS + [S - n])) if off + n <= S]


def targets_of(present, k):
    """Per block: its absent data shards, and its first and last present data shards."""
    out = []
    for b, pat in enumerate(present):
        there = [s for s in range(k) if pat[s]]
        out += [(b, s) for s in range(k) if not pat[s]] + [(b, s) for s in sorted({there[0], there[-1]} if there else [])]
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["aligned", "packed"])
@pytest.mark.parametrize("k,p", CODES, ids=lambda v: str(v))
def test_codes_patterns_and_alignment(gpu, k, p, packed):
    """Five blocks, five patterns, one call per (offset, len) of the alignment
    grid: the range into every absent data shard and into the first and last
    present data shard of every block (as many rounds as a block has targets)."""
    patterns = patterns_of(k, p)
    assert len({tuple(x) for x in patterns}) == 5 and all(sum(x) >= k for x in patterns) and sum(patterns[4]) == k
    if p > 32:
        assert [patterns[2][k + r] for r in (0, 31, 32, 33)] == [0, 0, 0, 0] and sum(patterns[2][k:]) == p - 4
    c = Case(k, p, patterns, gpu, packed=packed)
    targets = targets_of(patterns, k)
    per_block = max(sum(1 for b, _ in targets if b == blk) for blk in range(c.B))
    for i, (off, n) in enumerate(grid()):
        ups, src = c.place([(b, s, off, n) for b, s in targets], start=i % 16)
        round_of, nrounds, rebuilt, npieces, nchunks = c.rs.update_degraded_plan(c.present, ups, S, len(src))
        assert rebuilt.tolist() == [0 if patterns[b][s] else 1 for b, s in targets]
        assert 0 < rebuilt.sum() < len(ups) and nrounds == per_block and nchunks == 1
        before = shmr_amd.device_stats(0)["launches"]
        c.apply(ups, src, f"RS({k},{p}) [{off}, {off + n})")
        assert shmr_amd.device_stats(0)["launches"] == before + nrounds       # every pattern in one launch per round


def test_all_present_equals_plain_update(gpu):
    """Blocks with every shard present get exactly the bytes update_shards_dev
    writes to a copy, padding and guards included."""
    import torch
    k, p = 8, 3
    for packed in (False, True):
        c = Case(k, p, [[1] * (k + p)] * 3, gpu, packed=packed)
        writes = [(b, s, off, n) for b, (off, n) in enumerate([(13, 4096 + 6), (0, S), (4097, 20)]) for s in (0, 3, k - 1)]
        writes += [(1, 5, 1, 15), (2, 1, 16, 4096)]
        ups, src = c.place(writes)
        twin = c.buf.clone()
        src_t = torch.from_numpy(src).to(gpu)
        c.rs.update_shards_dev(twin[c.off:c.off + c.span].view(c.B, c.t, c.pitch), ups, src_t, shard_len=S)
        c.apply(ups, src, f"all present, packed={packed}")
        assert torch.equal(c.buf, twin)


def test_then_it_reads_back(gpu):
    """After the call read_batch_dev of the written ranges returns the new bytes,
    and a reconstruct leaves codewords: verify_shards_dev gives word 0."""
    import torch
    k, p = 8, 3
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    writes = [(b, s, off, n) for (b, s), (off, n) in zip(targets_of(patterns, k), [(13, 4096 + 6), (0, S), (4097, 20),
                                                                                   (1, 15), (16, 4096), (4090, 23)] * 4)]
    ups, src = c.place(writes)
    new = c.apply(ups, src, "degraded writes")
    reads, pos = [], 3
    for b, s, off, n, so in ups:
        reads.append((b, s, off, n, pos))
        pos += n + 1
    dst = torch.full((pos,), 0x5A, dtype=torch.uint8, device=gpu)
    c.rs.read_batch_dev(c.shards, c.present, reads, dst, shard_len=S)
    got = dst.cpu().numpy()
    for (b, s, off, n, so), (_, _, _, _, d) in zip(ups, reads):
        assert np.array_equal(got[d:d + n], src[so:so + n]), (b, s, off, n)
    c.rs.reconstruct_batch_dev(c.shards, c.present, shard_len=S)
    assert c.rs.verify_shards_dev(c.shards, shard_len=S).cpu().tolist() == [0] * c.B
    torch.cuda.synchronize()
    assert np.array_equal(c.view(c.buf.cpu().numpy())[:, :, :S], cw(k, p, new))


def test_rounds(gpu):
    """In one block over the same columns: two absent data shards; an absent and
    a present shard; partly overlapping ranges of three shards."""
    k, p = 8, 3
    t = k + p
    patterns = [[0 if i in (1, 4) else 1 for i in range(t)], [0 if i in (2, k + 1) else 1 for i in range(t)],
                [0 if i in (0, 5, k) else 1 for i in range(t)]]
    for packed in (False, True):
        c = Case(k, p, patterns, gpu, packed=packed)
        for writes, want_rounds in [([(0, 1, 13, 4096 + 6), (0, 4, 13, 4096 + 6)], 2),
                                    ([(1, 2, 0, S), (1, 3, 0, S)], 2),
                                    ([(2, 0, 0, 2000), (2, 3, 1000, 2000), (2, 5, 1999, 2118)], 3),
                                    ([(0, 1, 5, 100), (0, 4, 5, 100), (1, 2, 7, 50), (1, 0, 7, 50), (2, 0, 0, 17),
                                      (2, 5, 17, 1), (2, 7, 16, 17)], 2)]:
            ups, src = c.place(writes)
            nrounds = c.rs.update_degraded_plan(c.present, ups, S, len(src))[1]
            assert nrounds == want_rounds
            start = c.img.copy()
            c.apply(ups, src, f"{writes} packed={packed}")
            # the list in reverse order from the same start gives the same image
            image = c.img.copy()
            c.reset(start)
            c.apply(ups[::-1], src, f"{writes} reversed, packed={packed}")
            assert np.array_equal(c.img, image)


def test_absent_slots_are_never_read(gpu):
    """The same call over two fills of the absent slots gives the same present shards."""
    k, p = 8, 3
    patterns = patterns_of(k, p)
    writes = [(b, s, off, n) for (b, s), (off, n) in zip(targets_of(patterns, k), [(13, 4096 + 6), (0, S), (4097, 20),
                                                                                   (1, 15), (16, 4096), (4090, 23)] * 4)]
    got = []
    for fill in (0x00, (11,)):
        c = Case(k, p, patterns, gpu, packed=True, fill=fill)
        ups, src = c.place(writes)
        c.apply(ups, src, f"fill {fill}")
        got.append(c.view(c.img)[c.present.astype(bool)])
    assert np.array_equal(got[0], got[1])


@pytest.mark.parametrize("k,p,lost", [(8, 3, (2,)), (10, 4, (0, 11))], ids=["rs8_3_one_lost", "rs10_4_two_lost"])
def test_damage_is_preserved(gpu, k, p, lost):
    """Bytes flipped in one survivor, inside and outside the written columns: the
    word of reconstruct_checked_batch_dev(rebuild=False) is the same before and
    after, and the present shards are stored ^ cw(new data) ^ cw(old data), old
    data the oracle's first-k-present reconstruct of the damaged block (Case.expected)."""
    t = k + p
    pattern = [0 if i in lost else 1 for i in range(t)]
    # block 0: an input damaged; block 1: clean; block 2: a surplus parity shard damaged
    damage = [(0, 1, 100, 0x41), (0, 1, 3000, 0x80), (2, t - 1, 120, 0x07), (2, t - 1, S - 1, 0xFF)]
    c = Case(k, p, [pattern] * 3, gpu, damage=damage)
    before = c.rs.reconstruct_checked_batch_dev(c.shards, c.present, shard_len=S, rebuild=False).cpu().numpy()
    assert before[0] != 0 and before[1] == 0 and before[2] != 0
    writes = [(b, s, off, n) for b in range(3) for s, off, n in [(lost[0], 64, 1000), (1, 90, 40), (k - 1, 0, 200)]]
    ups, src = c.place(writes)
    c.apply(ups, src, "damaged survivors")
    after = c.rs.reconstruct_checked_batch_dev(c.shards, c.present, shard_len=S, rebuild=False).cpu().numpy()
    assert np.array_equal(before, after), (before, after)


def test_more_than_one_table_chunk(gpu):
    """One-byte updates, one more than a table chunk holds, over five blocks of
    five patterns, absent and present shards mixed: several rounds, each split
    over the chunks; the whole image is checked."""
    k, p = 8, 3
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    n = TABLE_CHUNK + 1
    rng = np.random.default_rng(77)
    flat = rng.choice(c.B * k * S, size=n, replace=False)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    order = rng.permutation(n)                                  # the new bytes in another order than the updates
    ups = [(int(f // (k * S)), int(f // S % k), int(f % S), 1, int(order[i])) for i, f in enumerate(flat)]
    round_of, nrounds, rebuilt, npieces, nchunks = c.rs.update_degraded_plan(c.present, ups, S, n)
    assert npieces == n and nchunks >= 2 and nrounds >= 2 and 0 < rebuilt.sum() < n
    before = shmr_amd.device_stats(0)["launches"]
    c.apply(ups, src, f"{n} one-byte updates")
    assert nrounds <= shmr_amd.device_stats(0)["launches"] - before <= nrounds + nchunks - 1


def test_stream_order(gpu):
    """A fill of the source buffer, the copy of the new bytes over it, the update
    and a copy of the image enqueued on one side stream with no synchronisation
    in between: the call sees what the preceding fill and copy wrote."""
    import torch
    k, p = 8, 3
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    writes = [(b, s, 13, S - 13) for b, s in targets_of(patterns, k)]
    ups, src = c.place(writes)
    want, new = c.expected(ups, src)
    src_t = torch.from_numpy(src).to(gpu)
    staged = torch.zeros_like(src_t)
    shmr_amd.device_init(0)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        staged.fill_(0x99)
        staged.copy_(src_t)
        c.rs.update_degraded_batch_dev(c.shards, c.present, ups, staged, shard_len=S)
        got = c.buf.clone()
    stream.synchronize()
    assert np.array_equal(got.cpu().numpy(), want)


def test_capturing_stream_is_refused(gpu):
    """On a stream that is being captured the call returns InvalidArgument,
    enqueues nothing and makes no blocking call; the image is unchanged."""
    import torch
    k, p = 8, 3
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    ups, src = c.place([(1, 1, 13, 4096 + 6), (1, 0, 0, S), (0, 0, 0, S), (3, k - 1, 5, 100)])
    start = c.img.copy()
    c.apply(ups, src, "outside the capture")                   # plan uploads outside the capture
    c.reset(start)
    src_t = torch.from_numpy(src).to(gpu)
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(shmr_amd.Error) as e:
            c.rs.update_degraded_batch_dev(c.shards, c.present, ups, src_t, shard_len=S)
    assert e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now["launches"] == st["launches"]
    assert now["blocking_calls"] == st["blocking_calls"], "a blocking HIP call inside the capture"
    torch.cuda.synchronize()
    assert np.array_equal(c.buf.cpu().numpy(), start)
    c.apply(ups, src, "after the capture")


def test_second_call_makes_no_blocking_call(gpu):
    """After the first call a repeat with already seen patterns adds 0 to
    blocking_calls and uploads no plan image; its launches are counted (one per
    round and table chunk)."""
    import torch
    k, p = 10, 4
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    ups, src = c.place([(1, 1, 0, S), (1, 0, 0, S), (4, 0, 13, 4096 + 6), (2, 3, 1, 15), (0, 9, 16, 17)])
    start = c.img.copy()
    c.apply(ups, src, "first call")
    want = c.img.copy()
    c.reset(start)
    src_t = torch.from_numpy(src).to(gpu)
    torch.cuda.synchronize()
    st = shmr_amd.device_stats(0)
    c.rs.update_degraded_batch_dev(c.shards, c.present, ups, src_t, shard_len=S)
    now = shmr_amd.device_stats(0)
    torch.cuda.synchronize()
    assert now["blocking_calls"] == st["blocking_calls"]
    assert now["launches"] == st["launches"] + 2                  # two rounds, one chunk
    assert now["plan_images"] == st["plan_images"]
    assert np.array_equal(c.buf.cpu().numpy(), want)
