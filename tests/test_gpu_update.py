"""Parity delta update on the GPU (gf_update.hip through
shmr_ec_update_batch_dev) against the CPU oracle.

Codewords come from oracle.c_oracle.encode_batch.  The expected image of every
case is the host image with the new bytes copied into the data shards and the
parity [:L] replaced by the oracle's encode of the new data; the comparison
covers the whole device buffer byte for byte, so a store outside an update's
footprint -- another shard, the pitch padding, a guard, another block -- fails it.

Layout (as tests/test_gpu_verify.py): B = 5 blocks, separate data and parity
regions in one device buffer, guard bytes in front of, between and behind them,
a shard pitch above len (rounded up to 64) whose padding holds random bytes
that are not a codeword.  `shift` moves both regions off 16-byte alignment.

The piece table travels in chunks of 8,192 pieces (one 256 KiB slot of the
upload ring, 32 bytes a piece: update_plan.hpp kTablePieces); the many-pieces
test uses 8,192 + 1,025 one-byte updates, more than one chunk.
"""
import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle

pytestmark = pytest.mark.gpu

CODES = [(4, 2), (8, 3), (10, 4), (5, 5), (3, 9), (2, 1)]
LENGTHS = [16, 1000, 4096 + 48, 12288 - 16]
B = 5
GUARD, SENT = 256, 0xC3
TABLE_CHUNK = 8192


def _pitch(L):
    return (L // 64 + 1) * 64            # above len, a multiple of 64


def _encode(k, p, d):
    """Oracle parity [B, p, L] of data [B, k, L]."""
    out = np.zeros((d.shape[0], p, d.shape[2]), np.uint8)
    c_oracle.encode_batch(k, p, np.ascontiguousarray(d), out, d.shape[0], d.shape[2], 8)
    return out


class Case:
    """Codewords of one (k, p, L) in the guarded two-region device layout
    (blocks: the batch's block count, B unless given)."""

    def __init__(self, k, p, L, gpu, seed, shift=0, blocks=B):
        import torch
        self.B = B = blocks
        self.k, self.p, self.L, self.pitch, self.gpu = k, p, L, _pitch(L), gpu
        rng = np.random.default_rng(seed)
        self.rng = rng
        pitch = self.pitch
        self.data_off = GUARD + shift
        self.par_off = self.data_off + B * k * pitch + GUARD
        total = self.par_off + B * p * pitch + GUARD
        img = np.full(total, SENT, np.uint8)
        d = img[self.data_off:self.data_off + B * k * pitch].reshape(B, k, pitch)
        q = img[self.par_off:self.par_off + B * p * pitch].reshape(B, p, pitch)
        d[:] = rng.integers(0, 256, d.shape, dtype=np.uint8)       # padding past len: random, not a codeword
        q[:] = rng.integers(0, 256, q.shape, dtype=np.uint8)
        q[:, :, :L] = _encode(k, p, d[:, :, :L])
        self.img = img                                             # the reference image: never changed
        self.buf = torch.from_numpy(img.copy()).to(gpu)
        assert self.buf.data_ptr() % 16 == 0
        self.data = self.buf[self.data_off:self.data_off + B * k * pitch].view(B, k, pitch)
        self.parity = self.buf[self.par_off:self.par_off + B * p * pitch].view(B, p, pitch)
        self.rs = shmr_amd.ReedSolomon(k, p)

    def views(self, img):
        k, p, pitch = self.k, self.p, self.pitch
        return (img[self.data_off:self.data_off + self.B * k * pitch].reshape(self.B, k, pitch),
                img[self.par_off:self.par_off + self.B * p * pitch].reshape(self.B, p, pitch))

    def reset(self, img=None):
        import torch
        self.buf.copy_(torch.from_numpy(self.img if img is None else img))

    def place(self, writes, residue=None):
        """[(block, shard, offset, len)] -> (updates with src offsets, src bytes).
        residue: None = src_offset = offset (mod 16); else that residue mod 16.
        A few bytes of slack separate the ranges in src."""
        ups, pos = [], 5
        for b, s, off, n in writes:
            want = off % 16 if residue is None else residue
            pos += (want - pos) % 16
            ups.append((b, s, off, n, pos))
            pos += n + 1
        return ups, self.rng.integers(0, 256, pos + 7, dtype=np.uint8)

    def expected(self, ups, src, start=None):
        """The image after the updates: new bytes in, parity = old parity ^
        enc(old data) ^ enc(new data) on [:L] (= enc(new data) for codewords)."""
        img = (self.img if start is None else start).copy()
        d, q = self.views(img)
        old = _encode(self.k, self.p, d[:, :, :self.L])
        for b, s, off, n, so in ups:
            d[b, s, off:off + n] = src[so:so + n]
        new = _encode(self.k, self.p, d[:, :, :self.L])
        q[:, :, :self.L] ^= old ^ new
        if start is None:
            assert np.array_equal(q[:, :, :self.L], new)           # the reference image holds codewords
        return img

    def apply(self, ups, src, what, start=None):
        import torch
        self.reset(start)
        src_t = torch.from_numpy(src).to(self.gpu)
        self.rs.update_batch_dev(self.data, self.parity, ups, src_t, shard_len=self.L)
        torch.cuda.synchronize()
        got = self.buf.cpu().numpy()
        want = self.expected(ups, src, start)
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0])} " \
                              f"(data region at {self.data_off}, parity region at {self.par_off}, pitch {self.pitch})"
        assert np.array_equal(src_t.cpu().numpy(), src), f"{what}: src was written"
        return got


def shapes(k, L):
    """name -> ([(block, shard, offset, len)], src residue) for one (k, L)."""
    out = {}
    out["first and last byte"] = ([(0, 0, 0, 1)] + ([(0, 0, L - 1, 1), (4, k - 1, L - 1, 1), (2, 1, 0, 1)] if L > 1 else []), None)
    out["inside one chunk [5, 9)"] = ([(1, k - 1, 5, 4)], None)
    if L >= 4096 + 19:
        out["across a tile, both ends unaligned [13, 4096 + 19)"] = ([(2, 0, 13, 4096 + 6)], None)
        out["across a tile, src 3 vs offset 13"] = ([(2, 0, 13, 4096 + 6)], 3)
    out["a whole shard"] = ([(3, 1, 0, L)], None)
    out["a whole shard, src off by 7"] = ([(3, 1, 0, L)], 7)
    out["src 3 vs offset 13"] = ([(0, 1, 13, L - 13)], 3)
    out["src = offset (mod 16)"] = ([(0, 1, 13, L - 13), (1, 0, 0, L), (2, 1, L // 2, L - L // 2)], None)
    n = min(L, 4096 + 19)
    out["two shards of a block, same columns"] = ([(1, 0, 0, n), (1, 1, 0, n), (3, k - 1, L - n, n), (3, 0, L - n, n)], 3)
    out["neighbours in a chunk, same shard"] = ([(4, 0, 0, 8), (4, 0, 8, 8), (0, 1, 3, 1), (0, 1, 4, 1), (0, 1, 5, 9)], None)
    out["neighbours in a chunk, different shards"] = ([(4, 0, 5, 4), (4, 1, 9, min(14, L - 9)), (2, 1, 0, 3), (2, 0, 3, 13)], 3)
    out["all k shards of every block"] = ([(b, s, 0, L) for b in range(B) for s in range(k)], None)
    return out


_cases = {}


def _case(key, gpu):
    if key not in _cases:
        _cases[key] = Case(*key[:3], gpu, seed=hash(key) & 0xffff, shift=key[3])
    return _cases[key]


@pytest.fixture(params=[(k, p, L) for k, p in CODES for L in LENGTHS], ids=lambda c: "rs%d_%d-len%d" % c)
def case(request, gpu):
    return _case(request.param + (0,), gpu)


@pytest.fixture(params=[(k, p, L) for k, p in CODES for L in LENGTHS], ids=lambda c: "rs%d_%d-len%d" % c)
def shifted(request, gpu):
    return _case(request.param + (3,), gpu)


def test_update_shapes(case):
    """Every write shape of the issue on 16-byte aligned regions."""
    for what, (writes, residue) in shapes(case.k, case.L).items():
        ups, src = case.place(writes, residue)
        case.apply(ups, src, what)


def test_update_shapes_misaligned_base(shifted):
    """The same shapes with both regions 3 bytes off 16-byte alignment."""
    assert shifted.data.data_ptr() % 16 == 3 and shifted.parity.data_ptr() % 16 == 3
    for what, (writes, residue) in shapes(shifted.k, shifted.L).items():
        ups, src = shifted.place(writes, residue)
        shifted.apply(ups, src, what)


def test_all_shards_equal_a_fresh_encode(case):
    """All k shards of every block rewritten over [0, L): the parity is the
    oracle's encode of the new data alone, whatever the old parity was."""
    k, p, L = case.k, case.p, case.L
    ups, src = case.place([(b, s, 0, L) for b in range(B) for s in range(k)], 7)
    got = case.apply(ups, src, "all shards")
    d, q = case.views(got)
    assert np.array_equal(q[:, :, :L], _encode(k, p, d[:, :, :L]))
    assert not case.rs.verify_batch_dev(case.data, case.parity, shard_len=L).cpu().numpy().any()


@pytest.mark.parametrize("k,p,L", [(8, 3, 4096 + 48), (5, 5, 1000), (2, 1, 12288 - 16)])
def test_syndrome_is_preserved(gpu, k, p, L):
    """One parity byte and one data byte flipped in different blocks before the
    update: the parity afterwards is old parity ^ enc(old data) ^ enc(new data),
    and verify_batch_dev returns the same words as before the update."""
    import torch
    c = _case((k, p, L, 0), gpu)
    start = c.img.copy()
    d, q = c.views(start)
    q[1, p - 1, L - 1] ^= 0x41
    d[3, k - 1, 17 % L] ^= 0x80
    c.reset(start)
    before = c.rs.verify_batch_dev(c.data, c.parity, shard_len=L).cpu().numpy()
    assert before[1] != 0 and before[3] != 0 and not before[[0, 2, 4]].any()
    writes = [(1, 0, 0, L), (3, k - 1, 0, L), (3, 0, 5, min(L - 5, 4096 + 14)), (0, 1, 13, 3), (1, 1, L - 1, 1)]
    ups, src = c.place(writes, 3)
    c.apply(ups, src, "damaged blocks", start=start)
    after = c.rs.verify_batch_dev(c.data, c.parity, shard_len=L).cpu().numpy()
    assert np.array_equal(before, after), (before, after)
    torch.cuda.synchronize()


def test_many_one_byte_updates(gpu):
    """More pieces than one table chunk holds (8,192): 9,217 one-byte updates at
    distinct (block, shard, column), several shards of a block at one column
    among them (several rounds, each split over the chunks)."""
    k, p, L = 8, 3, 1000
    c = _case((k, p, L, 0), gpu)
    n = TABLE_CHUNK + 1025
    rng = np.random.default_rng(77)
    flat = rng.choice(B * k * L, size=n, replace=False)
    src = rng.integers(0, 256, n, dtype=np.uint8)
    order = rng.permutation(n)                                  # the new bytes in another order than the updates
    ups = [(int(f // (k * L)), int(f // L % k), int(f % L), 1, int(order[i])) for i, f in enumerate(flat)]
    round_of, nrounds = c.rs.update_rounds(ups, B, L, len(src))
    assert nrounds >= 2 and len(round_of) == n
    c.apply(ups, src, "9217 one-byte updates")


def test_stream_order(gpu):
    """encode, update and verify enqueued on one side stream with no
    synchronisation in between: every word is 0."""
    import torch
    k, p, L = 8, 3, 4096 + 48
    c = _case((k, p, L, 0), gpu)
    c.reset()
    ups, src = c.place([(b, s, 13, L - 13) for b in range(B) for s in (0, 3, 7)] + [(2, 1, 0, L)], 3)
    src_t = torch.from_numpy(src).to(gpu)
    shmr_amd.device_init(0)
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.stream(stream):
        c.parity.fill_(0x99)
        c.rs.encode_batch_dev(c.data, c.parity, shard_len=L)
        c.rs.update_batch_dev(c.data, c.parity, ups, src_t, shard_len=L)
        words = c.rs.verify_batch_dev(c.data, c.parity, shard_len=L)
    stream.synchronize()
    assert not words.cpu().numpy().any()
    d, _ = c.views(c.buf.cpu().numpy())
    for b, s, off, n, so in ups:
        assert np.array_equal(d[b, s, off:off + n], src[so:so + n])


def test_capturing_stream_is_refused(gpu):
    """On a stream that is being captured the call returns InvalidArgument,
    enqueues nothing and makes no blocking call; the image is unchanged."""
    import torch
    k, p, L = 8, 3, 4096 + 48
    c = _case((k, p, L, 0), gpu)
    ups, src = c.place([(0, 0, 13, 4096 + 6), (4, 7, 0, L)], None)
    c.apply(ups, src, "outside the capture")                   # plan uploads outside the capture
    c.reset()
    src_t = torch.from_numpy(src).to(gpu)
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        with pytest.raises(shmr_amd.Error) as e:
            c.rs.update_batch_dev(c.data, c.parity, ups, src_t, shard_len=L)
    assert e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now["launches"] == st["launches"]
    assert now["blocking_calls"] == st["blocking_calls"], "a blocking HIP call inside the capture"
    torch.cuda.synchronize()
    assert np.array_equal(c.buf.cpu().numpy(), c.img)
    c.apply(ups, src, "after the capture")


def test_second_call_makes_no_blocking_call(gpu):
    """After the first call on a device a repeat of the same call adds 0 to
    blocking_calls; its launches are counted (one per round and table chunk)."""
    import torch
    k, p, L = 10, 4, 4096 + 48
    c = _case((k, p, L, 0), gpu)
    ups, src = c.place([(1, 0, 0, L), (1, 1, 0, L), (2, 9, 13, 4096 + 6)], 3)
    c.apply(ups, src, "first call")
    c.reset()
    src_t = torch.from_numpy(src).to(gpu)
    torch.cuda.synchronize()
    st = shmr_amd.device_stats(0)
    c.rs.update_batch_dev(c.data, c.parity, ups, src_t, shard_len=L)
    now = shmr_amd.device_stats(0)
    torch.cuda.synchronize()
    assert now["blocking_calls"] == st["blocking_calls"]
    assert now["launches"] == st["launches"] + 2                  # two rounds, one chunk
    assert np.array_equal(c.buf.cpu().numpy(), c.expected(ups, src))


def test_shards_form_and_src_checks(gpu):
    """update_shards_dev on one [B, k + p, pitch] tensor; src must be a 1-D uint8
    tensor on the tensors' device; a refused list changes nothing."""
    import torch
    k, p, L, pitch = 4, 2, 1000, 1024
    rng = np.random.default_rng(5)
    host = rng.integers(0, 256, (B, k + p, pitch), dtype=np.uint8)
    host[:, k:, :L] = _encode(k, p, host[:, :k, :L])
    shards = torch.from_numpy(host.copy()).to(gpu)
    rs = shmr_amd.ReedSolomon(k, p)
    src = rng.integers(0, 256, 3000, dtype=np.uint8)
    src_t = torch.from_numpy(src).to(gpu)
    ups = np.array([(0, 0, 0, L, 0), (0, 3, 0, L, 1000), (4, 2, 13, 900, 2003)], dtype=np.int64)
    for bad in (src_t.float(), src_t.view(30, 100), src, src_t.cpu()):
        with pytest.raises(TypeError):
            rs.update_shards_dev(shards, ups, bad, shard_len=L)
    for bad_ups in ([(0, 0, 0, L, 0), (0, 0, L - 1, 1, 0)], [(5, 0, 0, 1, 0)], [(0, 0, 0, 8, 2993)]):
        with pytest.raises(shmr_amd.Error) as e:
            rs.update_shards_dev(shards, bad_ups, src_t, shard_len=L)
        assert e.value.name == "InvalidArgument"
    rs.update_shards_dev(shards, [], src_t, shard_len=L)
    torch.cuda.synchronize()
    assert np.array_equal(shards.cpu().numpy(), host)
    rs.update_shards_dev(shards, ups, src_t, shard_len=L)
    torch.cuda.synchronize()
    want = host.copy()
    for b, s, off, n, so in ups.tolist():
        want[b, s, off:off + n] = src[so:so + n]
    want[:, k:, :L] = _encode(k, p, want[:, :k, :L])
    assert np.array_equal(shards.cpu().numpy(), want)
