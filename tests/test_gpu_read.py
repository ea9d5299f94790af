"""Ranged reads from device-resident blocks on the GPU (gf_read.hip through
shmr_ec_read_batch_dev) against the CPU oracle.

Every expected byte comes from oracle/rs_oracle.py: the blocks are encoded, the
absent shards dropped, ``reconstruct_data`` run on what is left, and the result
sliced.  The comparison is bit-exact and covers the whole destination buffer
(a canary outside the requests, gaps between them) and the whole shard buffer
(unchanged by the call, guards included).

Shapes: shard_len = 4117 is one full 4 KiB tile, one more 16-byte chunk and a
5-byte tail.  The aligned layout has a shard pitch of 4128 on a 16-byte aligned
base; the packed layout has shard_pitch = shard_len (odd), base and destination
off by one.  The piece table travels in chunks of 6,553 pieces (one 256 KiB slot
of the upload ring, 40 bytes a piece); the chunk test uses 7,000 requests.
"""
import numpy as np
import pytest

import shmr_amd
from oracle import rs_oracle

pytestmark = pytest.mark.gpu

S = 4117
GUARD, SENT, CANARY = 256, 0xC3, 0x5A
OFFSETS = [0, 1, 15, 16, 17, 4096, 4097]            # and shard_len - len
LENGTHS = [1, 15, 16, 17, 4096, 4101, S]
TABLE_CHUNK = 256 * 1024 // 40

_blocks = {}


def patterns_of(k, p):
    """all present; one data shard absent; two data shards absent; one data and
    one parity shard absent (a parity shard is an input); p shards absent."""
    t = k + p

    def drop(*idx):
        return [0 if i in idx else 1 for i in range(t)]
    return [drop(), drop(1), drop(0, k - 1), drop(2, k), drop(*range(1, 1 + p))]


def oracle_blocks(k, p, patterns, seed):
    """(full, data): the codewords [B, t, S], and per block the data shards the
    oracle's reconstruct_data leaves for the block's pattern [B, k, S]."""
    key = (k, p, tuple(map(tuple, patterns)), seed)
    if key not in _blocks:
        rs = rs_oracle.ReedSolomon(k, p)
        rng = np.random.default_rng(seed)
        B, t = len(patterns), k + p
        full = np.zeros((B, t, S), np.uint8)
        full[:, :k] = rng.integers(0, 256, (B, k, S), dtype=np.uint8)
        data = np.zeros((B, k, S), np.uint8)
        for b, pat in enumerate(patterns):
            rs.encode([full[b, i] for i in range(t)])
            left = [full[b, i].copy() if pat[i] else None for i in range(t)]
            rs.reconstruct_data(left)
            data[b] = np.stack(left[:k])
        full.setflags(write=False)
        data.setflags(write=False)
        _blocks[key] = (full, data)
    return _blocks[key]


class Case:
    """The blocks of one codec and pattern list on the device: `packed` = shard
    pitch S on a base off by one, else pitch 4128 on a 16-byte aligned base.
    Absent slots hold `fill`, never shard bytes."""

    def __init__(self, k, p, patterns, gpu, packed=False, fill=0xEE, seed=7):
        import torch
        self.k, self.p, self.gpu, self.packed = k, p, gpu, packed
        self.present = np.array(patterns, dtype=np.uint8)
        self.B, t = len(patterns), k + p
        self.full, self.data = oracle_blocks(k, p, patterns, seed)
        self.pitch = S if packed else 4128
        self.off = GUARD + (1 if packed else 0)
        img = np.full(self.off + self.B * t * self.pitch + GUARD, SENT, np.uint8)
        v = img[self.off:self.off + self.B * t * self.pitch].reshape(self.B, t, self.pitch)
        v[:, :, :S] = self.full
        if isinstance(fill, int):
            v[self.present == 0] = fill
        else:                                                          # random bytes in the absent slots
            v[self.present == 0] = np.random.default_rng(fill[0]).integers(0, 256, self.pitch, dtype=np.uint8)
        self.img = img
        self.buf = torch.from_numpy(img).to(gpu)
        assert self.buf.data_ptr() % 16 == 0
        self.shards = self.buf[self.off:self.off + self.B * t * self.pitch].view(self.B, t, self.pitch)
        self.rs = shmr_amd.ReedSolomon(k, p)

    def place(self, ranges, start=None, gap=3):
        """[(block, shard, offset, len)] -> requests with destinations `gap`
        bytes apart from `start` (default: 1 in the packed layout, else 16)."""
        pos = (1 if self.packed else 16) if start is None else start
        reads = []
        for b, s, off, n in ranges:
            reads.append((b, s, off, n, pos))
            pos += n + gap
        return reads, pos + 16

    def run(self, reads, dst_bytes, what=""):
        """The call into a canary-filled destination; checks every destination
        byte and that the shard buffer is untouched."""
        import torch
        dst = torch.full((dst_bytes,), CANARY, dtype=torch.uint8, device=self.gpu)
        self.rs.read_batch_dev(self.shards, self.present, reads, dst, shard_len=S)
        torch.cuda.synchronize()
        want = np.full(dst_bytes, CANARY, np.uint8)
        for b, s, off, n, d in reads:
            want[d:d + n] = self.data[b, s, off:off + n]
        got = dst.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} destination bytes differ, first at {bad[0]}"
        assert np.array_equal(self.buf.cpu().numpy(), self.img), f"{what}: the shards were written"
        return got


def grid_ranges(targets):
    """Every (offset, len) of the alignment grid that fits, for every target (block, shard)."""
    out = []
    for b, s in targets:
        for n in LENGTHS:
            for off in sorted(set(OFFSETS + [S - n])):
                if off + n <= S:
                    out.append((b, s, off, n))
    return out


def targets_of(present, k):
    """Per block: its absent data shards, and its first and last present data shards."""
    out = []
    for b, pat in enumerate(present):
        absent = [s for s in range(k) if not pat[s]]
        there = [s for s in range(k) if pat[s]]
        out += [(b, s) for s in absent] + [(b, s) for s in {there[0], there[-1]}]
    return out


@pytest.mark.parametrize("packed", [False, True], ids=["aligned", "packed"])
@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (10, 4)])
def test_codecs_patterns_and_alignment(gpu, k, p, packed):
    """Five blocks, five patterns, one call: the alignment grid into every absent
    data shard and into present shards of whole and degraded blocks."""
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu, packed=packed)
    ranges = grid_ranges(targets_of(patterns, k))
    reads, dst_bytes = c.place(ranges)
    rebuilt, npieces, nchunks = c.rs.read_plan(c.present, reads, S, dst_bytes)
    assert rebuilt.tolist() == [0 if patterns[b][s] else 1 for b, s, *_ in reads]
    assert 0 < rebuilt.sum() < len(reads) and nchunks == 1 and npieces > len(reads)
    before = shmr_amd.device_stats(0)["launches"]
    c.run(reads, dst_bytes, f"RS({k},{p})")
    assert shmr_amd.device_stats(0)["launches"] == before + 1       # every pattern in one launch


@pytest.mark.parametrize("k,p,lost", [(5, 5, [0, 1, 2, 3, 4]), (20, 4, [0, 7, 16, 19])],
                         ids=["rs5_5_all_data", "rs20_4_k_over_16"])
def test_wider_shapes(gpu, k, p, lost):
    """More absent rows than a row group holds (every input a parity shard), and
    more inputs than 16."""
    t = k + p
    patterns = [[0 if i in lost else 1 for i in range(t)], [1] * t, [0 if i == lost[-1] else 1 for i in range(t)]]
    for packed in (False, True):
        c = Case(k, p, patterns, gpu, packed=packed)
        ranges = [(0, s, off, n) for s in lost for off, n in [(0, S), (1, 4101), (17, 15), (4096, 21)]]
        ranges += [(1, 0, 0, S), (2, lost[-1], 3, 4100), (2, 0, 4097, 20)]
        reads, dst_bytes = c.place(ranges)
        c.run(reads, dst_bytes, f"RS({k},{p}) packed={packed}")


def test_absent_slots_are_never_read(gpu):
    """The same requests over two fills of the absent slots give the same bytes."""
    k, p = 8, 3
    patterns = patterns_of(k, p)
    ranges = grid_ranges([(b, s) for b, s in targets_of(patterns, k) if not patterns[b][s]])
    got = []
    for fill in (0x00, (11,)):
        c = Case(k, p, patterns, gpu, packed=True, fill=fill)
        reads, dst_bytes = c.place(ranges)
        got.append(c.run(reads, dst_bytes, f"fill {fill}"))
    assert np.array_equal(got[0], got[1])


def test_several_pieces_and_shared_sources(gpu):
    """Several requests per block and shard, touching destinations (no gap), the
    same source range to two destinations, list order unrelated to either."""
    k, p = 8, 3
    patterns = patterns_of(k, p)
    c = Case(k, p, patterns, gpu)
    ranges = []
    for b in range(c.B):
        for s in (0, 1, k - 1):
            ranges += [(b, s, 0, 100), (b, s, 50, 100), (b, s, 4000, 117), (b, s, 50, 100), (b, s, 0, S)]
    order = np.random.default_rng(3).permutation(len(ranges))
    reads, dst_bytes = c.place([ranges[i] for i in order], start=5, gap=0)
    c.run(reads, dst_bytes, "shared sources")
    # block_range_reads: a payload range across shard boundaries of a degraded block
    reads = c.rs.block_range_reads(2, S - 10, 2 * S + 30, S, dst_offset=9)
    assert [r[1] for r in reads] == [0, 1, 2, 3]
    got = c.run(reads, 9 + 2 * S + 30 + 7, "block range")
    payload = c.data[2].reshape(-1)
    assert np.array_equal(got[9:9 + 2 * S + 30], payload[S - 10:3 * S + 20])


def test_more_than_one_table_chunk(gpu):
    """7,000 sixteen-byte requests over four blocks: more pieces than a ring slot
    holds, so at least two uploads and two launches; every request is checked."""
    k, p = 8, 3
    patterns = patterns_of(k, p)[1:]
    c = Case(k, p, patterns, gpu)
    n = 7000
    ranges = [(i % c.B, (i // c.B) % k, 16 * ((i * 7) % 256) + (3 if i % 5 == 0 else 0), 16) for i in range(n)]
    reads, dst_bytes = c.place(ranges, gap=1)
    rebuilt, npieces, nchunks = c.rs.read_plan(c.present, reads, S, dst_bytes)
    assert npieces > TABLE_CHUNK and nchunks == -(-npieces // TABLE_CHUNK) >= 2
    before = shmr_amd.device_stats(0)["launches"]
    c.run(reads, dst_bytes, "two chunks")
    assert shmr_amd.device_stats(0)["launches"] == before + nchunks


def test_whole_shard_equals_reconstruct_out(gpu):
    """A whole-shard request returns the shard reconstruct_batch_dev_out(data_only) writes."""
    import torch
    k, p = 8, 3
    pattern = [0 if i == 3 else 1 for i in range(k + p)]
    c = Case(k, p, [pattern] * 3, gpu)
    out = torch.zeros((c.B, 1, 4128), dtype=torch.uint8, device=gpu)
    c.rs.reconstruct_batch_dev_out(c.shards, c.present, out, shard_len=S, data_only=True)
    reads = [(b, 3, 0, S, b * S) for b in range(c.B)]
    got = c.run(reads, c.B * S, "whole shard")
    torch.cuda.synchronize()
    assert np.array_equal(got.reshape(c.B, S), out.cpu().numpy()[:, 0, :S])


def test_read_after_update_of_the_same_range(gpu):
    """A range written by update_shards_dev and read back, lost shard and present:
    bytes [4090, 4113) of a shard are a 6-byte head, one vector piece at column
    4096 and a 1-byte tail in both kernels, whose pieces share one table lookup."""
    import torch
    k, p, b, s, off, n, src_off, dst_off = 4, 2, 1, 1, 4090, 23, 7, 33
    c = Case(k, p, [[1] * (k + p)] * 3, gpu)                         # pitch 4128 over shard_len 4117
    new = np.random.default_rng(5).integers(0, 256, 64, dtype=np.uint8)
    want = np.array(c.full)
    want[b, s, off:off + n] = new[src_off:src_off + n]
    rs_oracle.ReedSolomon(k, p).encode([want[b, i] for i in range(k + p)])
    c.rs.update_shards_dev(c.shards, [(b, s, off, n, src_off)], torch.from_numpy(new).to(gpu), shard_len=S)
    assert c.rs.verify_shards_dev(c.shards, shard_len=S).cpu().tolist() == [0, 0, 0]
    img = c.img.copy()
    img[c.off:c.off + c.B * (k + p) * c.pitch].reshape(c.B, k + p, c.pitch)[:, :, :S] = want
    assert np.array_equal(c.buf.cpu().numpy(), img), "the update wrote other bytes than the oracle's"
    for present in ([0 if (i, j) == (b, s) else 1 for i in range(c.B) for j in range(k + p)], [1] * (c.B * (k + p))):
        dst = torch.full((96,), CANARY, dtype=torch.uint8, device=gpu)
        c.rs.read_batch_dev(c.shards, np.array(present, np.uint8), [(b, s, off, n, dst_off)], dst, shard_len=S)
        expect = np.full(96, CANARY, np.uint8)
        expect[dst_off:dst_off + n] = want[b, s, off:off + n]
        assert np.array_equal(dst.cpu().numpy(), expect), f"present={present[b * (k + p) + s]}"
    assert np.array_equal(c.buf.cpu().numpy(), img), "a read wrote the shards"


def test_capturing_stream_is_refused(gpu):
    """On a stream that is being captured the call returns InvalidArgument and
    enqueues nothing; the destination is untouched."""
    import torch
    k, p = 8, 3
    c = Case(k, p, patterns_of(k, p), gpu)
    reads, dst_bytes = c.place([(1, 1, 13, 4096), (0, 0, 0, S)])
    c.run(reads, dst_bytes, "outside the capture")             # plan uploads outside the capture
    dst = torch.full((dst_bytes,), CANARY, dtype=torch.uint8, device=gpu)
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(shmr_amd.Error) as e:
            c.rs.read_batch_dev(c.shards, c.present, reads, dst, shard_len=S)
    assert e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now["launches"] == st["launches"]
    assert now["blocking_calls"] == st["blocking_calls"], "a blocking HIP call inside the capture"
    torch.cuda.synchronize()
    assert (dst.cpu().numpy() == CANARY).all()
    c.run(reads, dst_bytes, "after the capture")


def test_second_call_makes_no_blocking_call(gpu):
    k, p = 10, 4
    c = Case(k, p, patterns_of(k, p), gpu)
    reads, dst_bytes = c.place(grid_ranges([(1, 1), (4, 0)]))
    c.run(reads, dst_bytes, "first")
    st = shmr_amd.device_stats(0)
    c.run(reads, dst_bytes, "second")
    now = shmr_amd.device_stats(0)
    assert now["blocking_calls"] == st["blocking_calls"] and now["launches"] == st["launches"] + 1
    assert now["plan_images"] == st["plan_images"]
