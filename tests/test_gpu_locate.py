"""Single-shard location on the GPU (gf_locate.hip through
shmr_ec_locate_batch_dev) against the numpy reference tests/locate_ref.py.

Layout of every case, as tests/test_gpu_verify.py: B = 5 blocks, separate data
and parity regions in one device buffer, guard bytes (0xC3) in front of,
between and behind them, and a shard pitch above len (rounded up to 64) whose
padding holds random bytes that are not a codeword.  The result arrays are two
entries longer than B and the scratch has guard bytes around it; all carry
sentinels.  The lengths are tail-only, sub-tile, one full 4 KiB tile plus tail,
and two tiles plus tail.

Damage per case (DAMAGE below): block 0 untouched, block 1 one byte of data
shard 0, block 2 two bytes of data shard k-1 (in different tiles where the
length has two), block 3 one byte of parity shard p-1, block 4 one byte in each
of data shards 0 and 1 at the same column (p >= 3: not locatable) or one byte
of parity row 0 (p = 2, where two damaged shards may pass for one).
"""
import ctypes

import numpy as np
import pytest

import shmr_amd
from locate_cases import GUARD, SENT, HostCase
from locate_ref import CLEAN, NONE, locate_ref

pytestmark = pytest.mark.gpu

CODES = [(4, 2), (8, 3), (10, 4), (5, 5), (3, 9)]       # RS(5,5), RS(3,9): parity rows beyond the first row group
LENGTHS = [16, 1000, 4096 + 48, 8192 + 48]
B = 5
WORD_SENT = 0x5A5A5A5A
INVALID = -100


def damage_of(k, p, L):
    """[(block, shard, column, xor)] and the answers the issue's table expects."""
    d = [(1, 0, 0, 0x41),
         (2, k - 1, L - 1, 0xFF), (2, k - 1, min(5, L - 2), 0x41),
         (3, k + p - 1, L // 2, 0x41)]
    if p >= 3:
        d += [(4, 0, L // 3, 0x41), (4, 1, L // 3, 0x17)]
    else:
        d += [(4, k, L // 3, 0x41)]
    return d, [CLEAN, 0, k - 1, k + p - 1, NONE if p >= 3 else k]


class Case(HostCase):
    """Codewords of one (k, p, L) in the guarded two-region device layout
    (locate_cases.HostCase, nblk blocks); `odd` puts both regions at an odd
    byte offset."""

    def __init__(self, k, p, L, gpu, seed, odd=False, nblk=B, pitch=None):
        import torch
        super().__init__(k, p, L, seed, nblk=nblk, odd=odd, pitch=pitch)
        self.gpu = gpu
        self.rs = shmr_amd.ReedSolomon(k, p)
        self.words = torch.empty(nblk + 2, dtype=torch.int32, device=gpu)
        self.located = torch.empty(nblk + 2, dtype=torch.int32, device=gpu)
        self.need = self.rs.locate_work_size(nblk)
        self.work = torch.empty(self.need + 2 * GUARD, dtype=torch.uint8, device=gpu)
        self.load(self.pristine)

    def load(self, img):
        """Puts a host image on the device: self.img is what the device holds."""
        import torch
        B, k, p, pitch = self.B, self.k, self.p, self.pitch
        self.img = img.copy()
        self.buf = torch.from_numpy(self.img.copy()).to(self.gpu)
        self.data = torch.as_strided(self.buf, (B, k, pitch), (k * pitch, pitch, 1), self.data_off)
        self.parity = torch.as_strided(self.buf, (B, p, pitch), (p * pitch, pitch, 1), self.par_off)

    def reference(self):
        """locate_ref of every block of the host copy of what the device holds."""
        d, q = self.regions(self.img)
        return [locate_ref(self.k, self.p, d[b, :, :self.L], q[b, :, :self.L]) for b in range(self.B)]

    def locate(self, work_bytes=None, rs=None, work_fill=SENT):
        """One shmr_ec_locate_batch_dev into the guarded result arrays ->
        (status, words [B] uint32, located [B] int32); sentinels checked.
        `work_fill`: what the scratch between its guards holds before the call."""
        import torch
        B = self.B
        self.words.fill_(WORD_SENT)
        self.located.fill_(WORD_SENT)
        self.work.fill_(SENT)
        if work_fill != SENT:
            self.work[GUARD:GUARD + self.need].fill_(work_fill)
        v = ctypes.c_void_p
        rs = rs or self.rs
        rc = rs._L.shmr_ec_locate_batch_dev(
            rs._h, v(self.data.data_ptr()), self.pitch, self.k * self.pitch, v(self.parity.data_ptr()), self.pitch,
            self.p * self.pitch, B, self.L, v(self.words.data_ptr() + 4), v(self.located.data_ptr() + 4),
            v(self.work.data_ptr() + GUARD), self.need if work_bytes is None else work_bytes, 0,
            v(torch.cuda.current_stream().cuda_stream))
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().view(np.uint32)
        loc = self.located.cpu().numpy()
        work = self.work.cpu().numpy()
        assert w[0] == WORD_SENT and w[B + 1] == WORD_SENT, "a word next to d_mismatch was written"
        assert loc[0] == WORD_SENT and loc[B + 1] == WORD_SENT, "an entry next to d_located was written"
        assert (work[:GUARD] == SENT).all() and (work[GUARD + self.need:] == SENT).all(), "the scratch was overrun"
        return rc, w[1:B + 1].copy(), loc[1:B + 1].copy()

    def unchanged(self):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.img)
        assert bad.size == 0, f"{bad.size} bytes of the shard buffer changed, first at {int(bad[0])}"


def _check(c, want=None):
    """Locate what the device holds: the reference's answers (and the table's),
    verify's words, nothing else written."""
    rc, words, located = c.locate()
    assert rc == 0
    ref = c.reference()
    if want is not None:
        assert ref == want, "the reference disagrees with the expected answers"
    assert located.tolist() == ref
    verify = c.rs.verify_batch_dev(c.data, c.parity, shard_len=c.L).cpu().numpy().view(np.uint32)
    assert np.array_equal(words, verify), (words, verify)
    c.unchanged()
    return located


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", CODES)
def test_damage_table(gpu, k, p, L):
    c = Case(k, p, L, gpu, seed=(k * 64 + p) * 7 + L)
    # pristine: every block clean although the padding of every shard is random
    _check(c, [CLEAN] * B)
    damage, want = damage_of(k, p, L)
    c.load(c.damaged(damage))
    _check(c, want)
    # the tensor forms return the same
    mismatch, located = c.rs.locate_batch_dev(c.data, c.parity, shard_len=c.L)
    assert mismatch.shape == (B,) and located.shape == (B,) and located.device == c.buf.device
    assert located.cpu().numpy().tolist() == want
    c.unchanged()


@pytest.mark.parametrize("k,p,L", [(8, 3, 4096 + 48), (5, 5, 8192 + 48), (4, 2, 1000)])
def test_whole_shard_replaced(gpu, k, p, L):
    """Every byte of one data shard replaced by random bytes (every column of
    every tile carries a syndrome), and of one parity shard in another block."""
    c = Case(k, p, L, gpu, seed=91 + k)
    img = c.pristine.copy()
    d, q = c.regions(img)
    d[2, k // 2, :L] = c.rng.integers(0, 256, L, dtype=np.uint8)
    q[4, 1, :L] = c.rng.integers(0, 256, L, dtype=np.uint8)
    c.load(img)
    _check(c, [CLEAN, CLEAN, k // 2, CLEAN, k + 1])


def test_combined_tensor_form(gpu):
    """locate_shards_dev: one [B, k + p, pitch] tensor split into its regions."""
    import torch
    k, p, L = 8, 3, 4096 + 48
    c = Case(k, p, L, gpu, seed=77)
    d, q = c.regions(c.pristine)
    shards = torch.zeros((B, k + p, c.pitch), dtype=torch.uint8, device=gpu)
    shards[:, :k, :L] = torch.from_numpy(d[:, :, :L].copy()).to(gpu)
    shards[:, k:, :L] = torch.from_numpy(q[:, :, :L].copy()).to(gpu)
    shards[1, 6, 4100] ^= 1
    shards[4, k + 1, 7] ^= 1
    mismatch, located = c.rs.locate_shards_dev(shards, shard_len=L)
    assert mismatch.cpu().numpy().tolist() == [0, 7, 0, 0, 2]
    assert located.cpu().numpy().tolist() == [CLEAN, 6, CLEAN, CLEAN, k + 1]


@pytest.fixture(params=["device", "byte_granular"])
def misaligned_path(request):
    """Misaligned shards as the device runs them (the vector kernels where it
    passed the unaligned-access probe), and as a device that failed the probe
    does: the byte-granular kernel (knob uvec = 0)."""
    if request.param == "byte_granular":
        shmr_amd.set_tuning(uvec=0)
    try:
        yield request.param
    finally:
        shmr_amd.set_tuning(uvec=-2)


@pytest.mark.parametrize("k,p,L", [(10, 4, 4096 + 48), (5, 5, 1000)])
def test_odd_byte_offset(gpu, misaligned_path, k, p, L):
    c = Case(k, p, L, gpu, seed=5 + L, odd=True)
    assert c.data.data_ptr() % 2 == 1 and c.parity.data_ptr() % 2 == 1
    damage, want = damage_of(k, p, L)
    c.load(c.damaged(damage))
    _check(c, want)


def test_refused_calls_enqueue_nothing(gpu):
    """p = 1 and a scratch one byte short: InvalidArgument, and neither the
    result arrays nor the scratch are touched."""
    c = Case(4, 2, 1000, gpu, seed=13)
    rc, words, located = c.locate(work_bytes=c.need - 1)
    assert rc == INVALID
    assert (words == WORD_SENT).all() and (located == WORD_SENT).all()
    one = Case(4, 1, 1000, gpu, seed=14)
    assert one.need == 0
    rc, words, located = one.locate(work_bytes=1 << 16)
    assert rc == INVALID
    assert (words == WORD_SENT).all() and (located == WORD_SENT).all()
    with pytest.raises(shmr_amd.Error) as e:
        one.rs.locate_batch_dev(one.data, one.parity, shard_len=one.L)
    assert e.value.name == "InvalidArgument"


def test_capturing_stream_is_refused(gpu):
    """locate and scrub stay out of graphs (include/shmr_ec.h): on a stream that
    is being captured both return InvalidArgument, nothing is enqueued and no
    blocking call is made; the same calls work once the capture has ended."""
    import torch
    k, p, L = 8, 3, 4096 + 48
    c = Case(k, p, L, gpu, seed=11)
    shmr_amd.device_init(0)
    assert c.locate()[0] == 0                          # plan uploads outside the capture
    st = shmr_amd.device_stats(0)
    v = ctypes.c_void_p
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    c.words.fill_(WORD_SENT)
    c.located.fill_(WORD_SENT)
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        rc = c.rs._L.shmr_ec_locate_batch_dev(
            c.rs._h, v(c.data.data_ptr()), c.pitch, k * c.pitch, v(c.parity.data_ptr()), c.pitch, p * c.pitch, B, L,
            v(c.words.data_ptr() + 4), v(c.located.data_ptr() + 4), v(c.work.data_ptr() + GUARD), c.need, 0,
            v(torch.cuda.current_stream().cuda_stream))
        with pytest.raises(shmr_amd.Error) as e:
            c.rs.scrub_batch_dev(c.data, c.parity, shard_len=L)
    assert rc == INVALID and e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now["launches"] == st["launches"] and now["blocks_verified"] == st["blocks_verified"]
    assert now["blocking_calls"] == st["blocking_calls"], "a blocking HIP call inside the capture"
    torch.cuda.synchronize()
    assert (c.words.cpu().numpy() == WORD_SENT).all() and (c.located.cpu().numpy() == WORD_SENT).all()
    c.data[3, 5, 4100] ^= 8
    rc, words, located = c.locate()
    assert rc == 0 and words.tolist() == [0, 0, 0, 7, 0] and located.tolist() == [CLEAN, CLEAN, CLEAN, 5, CLEAN]
