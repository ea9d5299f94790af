"""ReedSolomon::verify on the GPU (gf_compare.hip through
shmr_ec_verify_batch_dev / shmr_ec_verify) against the CPU oracle.

Codewords come from oracle.c_oracle.encode_batch; they are damaged on the
device and the expected word of every block is computed on the host: bit
min(r, 31) for each parity row r whose oracle parity (of the data as it now
stands) differs from the stored parity within [0, len).

Layout of every pitch case: B = 5 blocks, separate data and parity regions in
one device buffer, guard bytes in front of, between and behind them, and a
shard pitch above len (rounded up to 64) whose padding holds random bytes that
are not a codeword.  The lengths are those at which a tail-only launch, one
full tile, and the 4 KiB and 8 KiB tile sizes disagree.

`launches` (include/shmr_ec.h SHMR_EC_DEV_LAUNCHES) counts launch groups of
<= 4 rows, one per group whatever the length splits into, so a verify of p
parity rows adds ceil(p / 4).
"""
import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle
from oracle import rs_oracle as O

pytestmark = pytest.mark.gpu

CODES = [(4, 2), (8, 3), (10, 4), (5, 5), (3, 9)]       # RS(5,5): row groups 4+1, RS(3,9): 4+4+1
LENGTHS = [16, 1000, 4096, 4096 + 48, 8192 + 48, 12288 - 16]
B = 5
GUARD, SENT = 256, 0xC3
WORD_SENT = 0x5A5A5A5A


def _bit(r):
    return 1 << min(r, 31)


def _pitch(L):
    return (L // 64 + 1) * 64            # above len, a multiple of 64


class Case:
    """Codewords of one (k, p, L) in the guarded two-region device layout."""

    def __init__(self, k, p, L, gpu, seed):
        import torch
        self.k, self.p, self.L, self.pitch = k, p, L, _pitch(L)
        rng = np.random.default_rng(seed)
        pitch = self.pitch
        self.data_off = GUARD
        self.par_off = GUARD + B * k * pitch + GUARD
        total = self.par_off + B * p * pitch + GUARD
        img = np.full(total, SENT, np.uint8)
        d = img[self.data_off:self.data_off + B * k * pitch].reshape(B, k, pitch)
        q = img[self.par_off:self.par_off + B * p * pitch].reshape(B, p, pitch)
        d[:] = rng.integers(0, 256, d.shape, dtype=np.uint8)       # padding past len: random, not a codeword
        q[:] = rng.integers(0, 256, q.shape, dtype=np.uint8)
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(d[:, :, :L]), par, B, L, 8)
        q[:, :, :L] = par
        self.img = img
        self.buf = torch.from_numpy(img.copy()).to(gpu)
        self.data = self.buf[self.data_off:self.data_off + B * k * pitch].view(B, k, pitch)
        self.parity = self.buf[self.par_off:self.par_off + B * p * pitch].view(B, p, pitch)
        self.words = torch.full((B + 2,), WORD_SENT, dtype=torch.int32, device=gpu)
        self.rs = shmr_amd.ReedSolomon(k, p)

    def host(self):
        """(data [B, k, L], parity [B, p, L]) of the pristine image."""
        k, p, pitch, L = self.k, self.p, self.pitch, self.L
        d = self.img[self.data_off:self.data_off + B * k * pitch].reshape(B, k, pitch)[:, :, :L]
        q = self.img[self.par_off:self.par_off + B * p * pitch].reshape(B, p, pitch)[:, :, :L]
        return d, q

    def expected(self, flips):
        """Oracle words after the flips [(block, shard, col)]."""
        d, q = self.host()
        d, q = d.copy(), q.copy()
        for b, s, col in flips:
            (d if s < self.k else q)[b, s if s < self.k else s - self.k, col] ^= 0x41
        want = np.zeros((B, self.p, self.L), np.uint8)
        c_oracle.encode_batch(self.k, self.p, np.ascontiguousarray(d), want, B, self.L, 8)
        words = np.zeros(B, np.uint32)
        for b in range(B):
            for r in range(self.p):
                if not np.array_equal(want[b, r], q[b, r]):
                    words[b] |= _bit(r)
        return words

    def run(self):
        """One verify_batch_dev; -> the B words (uint32), sentinels checked."""
        import torch
        self.words.fill_(WORD_SENT)
        out = self.rs.verify_batch_dev(self.data, self.parity, shard_len=self.L, out=self.words[1:B + 1])
        assert out.dtype == torch.int32 and out.shape == (B,) and out.data_ptr() == self.words[1:].data_ptr()
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().view(np.uint32)
        assert w[0] == WORD_SENT and w[B + 1] == WORD_SENT, "a word next to d_mismatch was written"
        return w[1:B + 1].copy()

    def flipped(self, flips):
        """Words of a verify with the flips applied on the device; the bytes
        are restored afterwards."""
        for b, s, col in flips:
            (self.data[b, s] if s < self.k else self.parity[b, s - self.k])[col] ^= 0x41
        try:
            return self.run()
        finally:
            for b, s, col in flips:
                (self.data[b, s] if s < self.k else self.parity[b, s - self.k])[col] ^= 0x41

    def unchanged(self):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.img)
        assert bad.size == 0, f"{bad.size} bytes of the shard buffer changed, first at {int(bad[0])}"


_cases = {}


@pytest.fixture(params=[(k, p, L) for k, p in CODES for L in LENGTHS], ids=lambda c: "rs%d_%d-len%d" % c)
def case(request, gpu):
    key = request.param
    if key not in _cases:
        _cases[key] = Case(*key, gpu, seed=hash(key) & 0xffff)
    return _cases[key]


def _columns(L):
    return [c for c in (0, L - 1, 4095, 4096) if 0 <= c < L]


def test_clean_is_zero_and_writes_nothing(case):
    """Every word 0 although the padding past len of every shard is random; the
    shard buffer (guards and padding included) is untouched."""
    w = case.run()
    assert not w.any(), w
    # a fresh result tensor, on the tensors' device
    out = case.rs.verify_batch_dev(case.data, case.parity, shard_len=case.L)
    assert out.shape == (B,) and out.device == case.buf.device and not out.cpu().numpy().any()
    case.unchanged()


def test_single_byte_flips(case):
    """One flipped byte in block 2 -- first and last column, the columns around
    the 4 KiB tile boundary, in the first and last data shard and the first
    and last parity row -- gives the oracle's word there and 0 elsewhere."""
    k, p, L = case.k, case.p, case.L
    for shard in sorted({0, k - 1, k, k + p - 1}):
        for col in _columns(L):
            flips = [(2, shard, col)]
            want = case.expected(flips)
            assert want[2] != 0 and not want[[0, 1, 3, 4]].any()
            if shard >= k:
                assert want[2] == _bit(shard - k)
            got = case.flipped(flips)
            assert np.array_equal(got, want), (shard, col, got, want)
    case.unchanged()


def test_two_flips_in_one_block(case):
    """Different parity rows, different tiles where the length has two."""
    k, p, L = case.k, case.p, case.L
    flips = [(3, k, 0), (3, k + p - 1, L - 1)]
    want = case.expected(flips)
    assert want[3] == _bit(0) | _bit(p - 1)
    got = case.flipped(flips)
    assert np.array_equal(got, want), (got, want)
    # ... and a data flip beside a parity flip
    flips = [(1, k - 1, L // 2), (1, k, L - 1)]
    want = case.expected(flips)
    got = case.flipped(flips)
    assert np.array_equal(got, want), (got, want)


def test_flips_in_two_blocks(case):
    k, p, L = case.k, case.p, case.L
    flips = [(0, k + p - 1, L - 1), (4, 0, 0)]
    want = case.expected(flips)
    assert want[0] == _bit(p - 1) and want[4] == (1 << p) - 1 and not want[1:4].any()
    got = case.flipped(flips)
    assert np.array_equal(got, want), (got, want)
    case.unchanged()


def test_padding_does_not_take_part(case):
    """A flip at column len (the first padding byte) of a data and of a parity
    shard changes nothing."""
    L = case.L
    case.data[2, 0][L] ^= 0xFF
    case.parity[2, case.p - 1][L] ^= 0xFF
    try:
        assert not case.run().any()
    finally:
        case.data[2, 0][L] ^= 0xFF
        case.parity[2, case.p - 1][L] ^= 0xFF


def test_combined_tensor_form(gpu):
    """verify_shards_dev: one [B, k + p, pitch] tensor split into its regions."""
    import torch
    k, p, L = 8, 3, 4096 + 48
    c = Case(k, p, L, gpu, seed=77)
    d, q = c.host()
    shards = torch.zeros((B, k + p, c.pitch), dtype=torch.uint8, device=gpu)
    shards[:, :k, :L] = torch.from_numpy(d.copy()).to(gpu)
    shards[:, k:, :L] = torch.from_numpy(q.copy()).to(gpu)
    assert not c.rs.verify_shards_dev(shards, shard_len=L).cpu().numpy().any()
    shards[4, k + 1, 4100] ^= 1
    assert c.rs.verify_shards_dev(shards, shard_len=L).cpu().numpy().view(np.uint32).tolist() == [0, 0, 0, 0, 2]


# ---- misaligned: the reference's packed block (shard i at i * S), odd base ----------
@pytest.fixture
def byte_granular():
    """Misaligned shards as a device that failed the unaligned-access probe
    runs them: the byte-granular kernel (knob uvec = 0)."""
    shmr_amd.set_tuning(uvec=0)
    try:
        yield
    finally:
        shmr_amd.set_tuning(uvec=-2)


def _packed(k, p, S, gpu, seed):
    import torch
    t = k + p
    rng = np.random.default_rng(seed)
    cw = np.empty((B, t, S), np.uint8)
    cw[:, :k] = rng.integers(0, 256, (B, k, S), dtype=np.uint8)
    par = np.zeros((B, p, S), np.uint8)
    c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k]), par, B, S, 8)
    cw[:, k:] = par
    off = GUARD + 1                        # odd base
    img = np.full(off + B * t * S + GUARD, SENT, np.uint8)
    img[off:off + B * t * S] = cw.reshape(-1)
    buf = torch.from_numpy(img.copy()).to(gpu)
    data = torch.as_strided(buf, (B, k, S), (t * S, S, 1), off)
    parity = torch.as_strided(buf, (B, p, S), (t * S, S, 1), off + k * S)
    return cw, img, buf, data, parity


def _misaligned(k, p, S, gpu):
    rs = shmr_amd.ReedSolomon(k, p)
    cw, img, buf, data, parity = _packed(k, p, S, gpu, seed=S + k)
    assert data.data_ptr() % 2 == 1
    got = rs.verify_batch_dev(data, parity, shard_len=S).cpu().numpy()
    assert not got.any(), got
    for shard, col in ((0, 0), (k - 1, S - 1), (k + p - 1, S - 1), (k, min(4096, S - 1))):
        t = data[2, shard] if shard < k else parity[2, shard - k]
        t[col] ^= 0x80
        got = rs.verify_batch_dev(data, parity, shard_len=S).cpu().numpy().view(np.uint32)
        t[col] ^= 0x80
        want = [0] * B
        want[2] = (1 << p) - 1 if shard < k else _bit(shard - k)     # MDS: a data byte reaches every parity row
        assert got.tolist() == want, (shard, col, got, want)
    assert np.array_equal(buf.cpu().numpy(), img)


@pytest.mark.parametrize("S", [1000, 4099])
@pytest.mark.parametrize("k,p", [(10, 4), (5, 5)])
def test_misaligned_packed_block(gpu, k, p, S):
    _misaligned(k, p, S, gpu)


@pytest.mark.parametrize("S", [1000, 4099])
def test_misaligned_byte_granular(gpu, byte_granular, S):
    _misaligned(5, 5, S, gpu)


def test_saturating_bit(gpu):
    """RS(4,40): parity rows 31 and above share bit 31."""
    import torch
    k, p, L = 4, 40, 64
    rs = shmr_amd.ReedSolomon(k, p)
    rng = np.random.default_rng(40)
    d = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    q = np.zeros((B, p, L), np.uint8)
    c_oracle.encode_batch(k, p, d, q, B, L, 8)
    data, parity = torch.from_numpy(d).to(gpu), torch.from_numpy(q).to(gpu)
    assert not rs.verify_batch_dev(data, parity).cpu().numpy().any()
    parity[2, 35, 17] ^= 4
    got = rs.verify_batch_dev(data, parity).cpu().numpy().view(np.uint32)
    assert got.tolist() == [0, 0, 1 << 31, 0, 0]
    parity[1, 30, 0] ^= 4
    parity[1, 31, 63] ^= 4
    got = rs.verify_batch_dev(data, parity).cpu().numpy().view(np.uint32)
    assert got.tolist() == [0, (1 << 30) | (1 << 31), 1 << 31, 0, 0]


def test_host_call_matches_the_oracle(gpu):
    """shmr_ec_verify / ReedSolomon.verify on numpy shards: the oracle's answer,
    shards unmodified."""
    k, p, L = 8, 3, 1000
    rs, ors = shmr_amd.ReedSolomon(k, p), O.ReedSolomon(k, p)
    rng = np.random.default_rng(83)
    shards = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(p)]
    c_oracle.encode(k, p, shards)
    before = [s.copy() for s in shards]
    assert ors.verify(shards) is True and rs.verify(shards) is True
    assert rs.verify([bytes(s) for s in shards]) is True
    for shard, col in ((0, 0), (k - 1, L - 1), (k, 500), (k + p - 1, L - 1)):
        shards[shard][col] ^= 1
        held = [s.copy() for s in shards]
        assert ors.verify(shards) is False
        assert rs.verify(shards) is False, (shard, col)
        assert all(np.array_equal(a, b) for a, b in zip(shards, held)), "verify wrote a shard"
        shards[shard][col] ^= 1
    assert rs.verify(shards) is True
    assert all(np.array_equal(a, b) for a, b in zip(shards, before))
    # larger than one tile, and a length that is not a multiple of 16
    L2 = 8192 + 4096 + 5
    big = [rng.integers(0, 256, L2, dtype=np.uint8) for _ in range(k)] + [np.zeros(L2, np.uint8) for _ in range(p)]
    c_oracle.encode(k, p, big)
    assert rs.verify(big) is True
    big[k + 1][L2 - 1] ^= 0x10
    assert rs.verify(big) is False and ors.verify(big) is False


@pytest.mark.parametrize("k,p", CODES)
def test_counters(gpu, k, p):
    """blocks_verified grows by B and launches by one per group of <= 4 parity
    rows; no kernel_inventory row (the encode / reconstruct kernels) moves."""
    c = Case(k, p, 8192 + 48, gpu, seed=3)
    c.run()                                               # device init, plan upload
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}
    st = shmr_amd.device_stats(0)
    for n in (1, 2):
        assert not c.run().any()
        now = shmr_amd.device_stats(0)
        assert now["blocks_verified"] - st["blocks_verified"] == n * B
        assert now["launches"] - st["launches"] == n * ((p + 3) // 4)
        assert now["blocks_encoded"] == st["blocks_encoded"] and now["blocking_calls"] == st["blocking_calls"]
    after = {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}
    assert after == inv


def test_graph_capture(gpu):
    """One captured verify_batch_dev replays right on changing data: the zeroing
    of the result words is part of the graph (memset node -> kernels, a single
    chain on the capture stream)."""
    import torch
    c = Case(8, 3, 4096 + 48, gpu, seed=11)
    shmr_amd.device_init(0)
    blocking = shmr_amd.device_stats(0)["blocking_calls"]
    torch.cuda.synchronize()
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    with torch.cuda.graph(graph, stream=stream):
        c.rs.verify_batch_dev(c.data, c.parity, shard_len=c.L, out=c.words[1:B + 1])
    assert shmr_amd.device_stats(0)["blocking_calls"] == blocking, "a blocking HIP call inside the capture"

    def replay():
        graph.replay()
        torch.cuda.synchronize()
        w = c.words.cpu().numpy().view(np.uint32)
        assert w[0] == WORD_SENT and w[B + 1] == WORD_SENT
        return w[1:B + 1].tolist()

    assert replay() == [0] * B
    c.parity[3, 1, 4100] ^= 8
    assert replay() == [0, 0, 0, 2, 0]
    c.parity[3, 1, 4100] ^= 8
    assert replay() == [0] * B, "the words are not zeroed inside the graph"
    c.data[0, 7, 5] ^= 8
    assert replay() == [7, 0, 0, 0, 0]
    c.data[0, 7, 5] ^= 8
    c.unchanged()
