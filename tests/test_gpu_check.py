"""Checked reconstruct on the GPU (gf_compare.hip through
shmr_ec_reconstruct_checked_batch_dev) against oracle/rs_oracle.py.

Layout of every case: B = 6 blocks of k + p shards in one device buffer with
sentinel guards in front and behind, a shard pitch above len whose padding
holds random bytes that are no codeword, absent slots filled with a sentinel
over their whole pitch, and sentinel words on both sides of the B result words.

Patterns of the plain arrangement (they differ per block within the batch):
  block 0     every shard present (the word must be verify's);
  block 1     exactly k present: data shard 1 and the parity rows 1 .. p-1
              absent, so there is no surplus and the word stays 0;
  blocks 2,4  one absent data shard (one pattern; an arithmetic sequence);
  block 3     parity row 0 absent: the surplus rows are 1 .. p-1, so a compare
              row's bit is not its row number in the plan;
  block 5     data shard 0 and parity row 1 absent -- for RS(4,6) parity rows
              1 .. 4 (5 absent: 5 stored + 1 compared row, the boundary falls
              between the launch groups; RS(5,6) with one absent shard has 1
              stored + 5 compared, the boundary inside group 0).
The list arrangement gives the one-absent-data pattern to blocks 0, 1 and 3 --
two blocks are always an arithmetic sequence, three at these places are not --
so that pattern's blocks travel as an uploaded list; with B = 6 that leaves
room for three more patterns, and the exactly-k pattern (no compare row) is
the one left out there.

Expected values: words from ReedSolomon.checked_rows (tests/test_check_abi.py
checks it against numpy) and bit min(r, 31); rebuilt bytes from the oracle's
reconstruct of the shards as they stand, and from reconstruct_batch_dev on a
copy of the same buffer.
"""
import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle
from oracle import rs_oracle as O

pytestmark = pytest.mark.gpu

B = 6
GUARD, SENT, ABSENT = 256, 0xC3, 0xA5
WORD_SENT = 0x5A5A5A5A
LENGTHS = {(4, 2): [100, 4096, 4096 + 48, 8192 + 48], (8, 3): [100, 4096, 4096 + 48, 8192 + 48],
           (5, 6): [100, 4096 + 48], (4, 6): [100, 4096 + 48], (2, 34): [100]}
CASES = [(k, p, L) for (k, p), ls in LENGTHS.items() for L in ls]


def _bit(r):
    return 1 << min(r, 31)


def _patterns(k, p, arrangement):
    t = k + p
    full = np.ones(t, np.uint8)
    exactly_k = full.copy()
    exactly_k[[1] + list(range(k + 1, t))] = 0
    one_data = full.copy()
    one_data[min(2, k - 1)] = 0
    one_parity = full.copy()
    one_parity[k] = 0
    both = full.copy()
    both[[0] + (list(range(k + 1, k + 5)) if (k, p) == (4, 6) else [k + 1])] = 0
    if arrangement == "plain":
        return np.stack([full, exactly_k, one_data, one_parity, one_data, both])
    return np.stack([one_data, one_data, full, one_data, one_parity, both])


class Case:
    def __init__(self, k, p, L, gpu, arrangement="plain", odd=False, present=None):
        """present: a [blocks, k + p] array of the batch's own patterns (any
        block count) in place of an arrangement's six."""
        import torch
        self.k, self.p, self.t, self.L = k, p, k + p, L
        t = k + p
        self.present = _patterns(k, p, arrangement) if present is None else np.array(present, np.uint8)
        self.B = B = len(self.present)
        self.pitch = pitch = (L // 64 + 1) * 64 + (1 if odd else 0)     # above len
        self.off = off = GUARD + (1 if odd else 0)
        rng = np.random.default_rng([k, p, L, int(odd)])
        img = np.full(off + B * t * pitch + GUARD, SENT, np.uint8)
        cw = img[off:off + B * t * pitch].reshape(B, t, pitch)
        cw[:] = rng.integers(0, 256, cw.shape, dtype=np.uint8)         # padding past len: random, no codeword
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k, :L]), par, B, L, 8)
        cw[:, k:, :L] = par
        self.clean = img                                               # every shard in place
        self.start = img.copy()                                        # absent slots hold the sentinel
        self.view(self.start)[self.present == 0] = ABSENT
        self.rs, self.ors = shmr_amd.ReedSolomon(k, p), O.ReedSolomon(k, p)
        self.rows = [self.rs.checked_rows(pr) for pr in self.present]
        self.inputs = [np.flatnonzero(pr)[:k] for pr in self.present]
        self.surplus = [np.flatnonzero(pr)[k:] for pr in self.present]
        self.start_dev = torch.from_numpy(self.start).to(gpu)
        self.buf = self.start_dev.clone()
        self.shards = self.dev_view(self.buf)
        self.words = torch.full((B + 2,), WORD_SENT, dtype=torch.int32, device=gpu)

    def view(self, img):
        return img[self.off:self.off + self.B * self.t * self.pitch].reshape(self.B, self.t, self.pitch)

    def dev_view(self, buf):
        import torch
        return torch.as_strided(buf, (self.B, self.t, self.pitch), (self.t * self.pitch, self.pitch, 1), self.off)

    def reset(self):
        self.buf.copy_(self.start_dev)

    def run(self, data_only=False, rebuild=True):
        """One checked call; -> the B words (uint32), the sentinel words checked."""
        import torch
        self.words.fill_(WORD_SENT)
        out = self.rs.reconstruct_checked_batch_dev(self.shards, self.present, shard_len=self.L, data_only=data_only,
                                                    rebuild=rebuild, out=self.words[1:self.B + 1])
        assert out.dtype == torch.int32 and out.shape == (self.B,) and out.data_ptr() == self.words[1:].data_ptr()
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().view(np.uint32)
        assert w[0] == WORD_SENT and w[self.B + 1] == WORD_SENT, "a word next to d_mismatch was written"
        return w[1:self.B + 1].copy()

    def flip(self, flips, x=0x41):
        for b, s, col in flips:
            self.shards[b, s, col] ^= x

    def image(self, flips=(), data_only=False, rebuilt=True, x=0x41):
        """The buffer a call must leave: the start image with the flips, and
        (rebuilt) [0, len) of every rebuilt slot from the oracle's reconstruct
        of the block as it then stands.  Guards, padding, present shards and
        slots that are not rebuilt keep their bytes."""
        img = self.start.copy()
        v = self.view(img)
        for b, s, col in flips:
            v[b, s, col] ^= x
        if not rebuilt:
            return img
        for b in range(self.B):
            pr = self.present[b]
            if pr.all():
                continue
            shards = [v[b, i, :self.L].copy() if pr[i] else None for i in range(self.t)]
            (self.ors.reconstruct_data if data_only else self.ors.reconstruct)(shards)
            for i in np.flatnonzero(pr == 0):
                if shards[i] is not None:
                    v[b, i, :self.L] = shards[i]
        return img

    def same(self, want, what):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != want)
        assert bad.size == 0, f"{what}: {bad.size} bytes differ, first at {int(bad[0])} (shards start at {self.off})"

    def plain_reconstruct(self, data_only=False):
        """reconstruct_batch_dev on a copy of the buffer as it stands -> its bytes."""
        import torch
        copy = self.buf.clone()
        self.rs.reconstruct_batch_dev(self.dev_view(copy), self.present, shard_len=self.L, data_only=data_only)
        torch.cuda.synchronize()
        return copy.cpu().numpy()


_cases = {}


def _case(key, gpu):
    if key not in _cases:
        _cases[key] = Case(*key[:3], gpu, *key[3:])
    c = _cases[key]
    c.reset()
    return c


@pytest.fixture(params=CASES, ids=lambda c: "rs%d_%d-len%d" % c)
def case(request, gpu):
    return _case(request.param, gpu)


def _columns(L):
    """First, last, and one in the second 4 KiB tile."""
    return [c for c in (0, L - 1, 4096 + 5) if c < L]


def test_clean_codewords(case):
    """Every word 0; rebuilt bytes are the oracle's and reconstruct_batch_dev's;
    rebuild=False writes nothing; data_only leaves absent parity at its sentinel."""
    c = case
    want = c.image()
    for b in range(B):                                            # the oracle rebuilt the codeword
        for i in np.flatnonzero(c.present[b] == 0):
            assert np.array_equal(c.view(want)[b, i, :c.L], c.view(c.clean)[b, i, :c.L])
    plain = c.plain_reconstruct()
    assert np.array_equal(plain, want)
    w = c.run()
    assert not w.any(), w
    c.same(want, "rebuild")
    c.reset()
    assert not c.run(rebuild=False).any()
    c.same(c.start, "rebuild=False")
    assert not c.run(data_only=True, rebuild=False).any()
    c.same(c.start, "data_only, rebuild=False")
    want = c.image(data_only=True)
    v = c.view(want)
    for b in range(B):
        for i in np.flatnonzero(c.present[b, c.k:] == 0):
            assert (v[b, c.k + i] == ABSENT).all()
    assert not c.run(data_only=True).any()
    c.same(want, "data_only")
    assert np.array_equal(c.plain_reconstruct(data_only=True), want)   # (nothing left to rebuild but absent parity)
    # a fresh result tensor, on the tensors' device
    out = c.rs.reconstruct_checked_batch_dev(c.shards, c.present, shard_len=c.L, rebuild=False)
    assert out.shape == (B,) and out.device == c.buf.device and not out.cpu().numpy().any()


def test_flipped_input_byte(case):
    """One flipped byte in an input shard of every block: every surplus row
    differs (the word is checked_rows of the block's pattern; 0 for block 1,
    which has no surplus), the rebuilt bytes are still what the oracle and
    reconstruct_batch_dev make of the damaged inputs, and the all-present
    block's word is verify's."""
    c = case
    for n, col in enumerate(_columns(c.L)):
        c.reset()
        flips = [(b, int(c.inputs[b][(b + n) % c.k]), col) for b in range(B)]
        c.flip(flips)
        want_words = np.array(c.rows, np.uint32)
        if n == 0:
            plain = c.plain_reconstruct()
            got = c.run()
            want = c.image(flips)
            c.same(want, f"column {col}")
            assert np.array_equal(plain, want)
            verify = c.rs.verify_shards_dev(c.shards, shard_len=c.L).cpu().numpy().view(np.uint32)
            full = np.flatnonzero(c.present.all(axis=1))
            assert full.size and np.array_equal(got[full], verify[full])
        else:
            got = c.run(rebuild=False)
            c.same(c.image(flips, rebuilt=False), f"column {col}, rebuild=False")
        assert np.array_equal(got, want_words), (col, got, want_words)
        assert got[c.present.sum(axis=1) == c.k].tolist() == [0] * int((c.present.sum(axis=1) == c.k).sum())


def test_flipped_surplus_byte(case):
    """One flipped byte in surplus shard k + r: exactly bit min(r, 31); the
    first and the last surplus shard of every block that has one."""
    c = case
    cols = _columns(c.L)
    for n, pick in enumerate((0, -1)):
        c.reset()
        flips, want = [], np.zeros(B, np.uint32)
        for b in range(B):
            if len(c.surplus[b]):
                s = int(c.surplus[b][pick])
                flips.append((b, s, cols[(b + n) % len(cols)]))
                want[b] = _bit(s - c.k)
        c.flip(flips, x=0x80)
        got = c.run(rebuild=bool(n))
        assert np.array_equal(got, want), (pick, got, want)
        c.same(c.image(flips, rebuilt=bool(n), x=0x80), "surplus flip")
        verify = c.rs.verify_shards_dev(c.shards, shard_len=c.L).cpu().numpy().view(np.uint32)
        full = np.flatnonzero(c.present.all(axis=1))
        assert np.array_equal(got[full], verify[full])


def test_padding_and_absent_slots_do_not_take_part(case):
    """Flips at column len (the first padding byte) of an input and of a surplus
    shard, and in an absent slot before the call: every word 0, and the absent
    slot is rebuilt over the flipped byte."""
    c = case
    flips = [(b, int(c.inputs[b][0]), c.L) for b in range(B)]
    flips += [(b, int(c.surplus[b][-1]), c.L) for b in range(B) if len(c.surplus[b])]
    absent = [(b, int(np.flatnonzero(c.present[b] == 0)[0]), 0) for b in range(B) if not c.present[b].all()]
    c.flip(flips + absent)
    assert not c.run(rebuild=False).any()
    assert not c.run().any()
    c.same(c.image(flips), "padding and absent-slot flips")


@pytest.mark.parametrize("k,p,L", [(4, 2, 4096 + 48), (8, 3, 8192 + 48), (5, 6, 4096 + 48), (4, 6, 100), (2, 34, 100)])
def test_block_list_path(gpu, k, p, L):
    """The list arrangement: blocks 0, 1, 3 share a pattern and are no arithmetic
    sequence.  The word index is still the block's index in the batch."""
    c = _case((k, p, L, "list"), gpu)
    blocks = [b for b in range(B) if np.array_equal(c.present[b], c.present[0])]
    assert blocks == [0, 1, 3]
    assert not c.run().any()
    c.same(c.image(), "clean")
    for n, col in enumerate(_columns(L)):
        c.reset()
        flips = [(b, int(c.inputs[b][(b + n) % k]), col) for b in (1, 3, 5)]
        s = int(c.surplus[0][-1])
        flips.append((0, s, col))
        c.flip(flips)
        want = np.array([_bit(s - k), c.rows[1], 0, c.rows[3], 0, c.rows[5]], np.uint32)
        got = c.run()
        assert np.array_equal(got, want), (col, got, want)
        c.same(c.image(flips), f"column {col}")


@pytest.fixture(params=[0, -2], ids=["byte_granular", "vector"])
def uvec(request):
    """Misaligned shards as a device that failed the unaligned-access probe runs
    them (knob uvec = 0: the byte-granular kernel, MODE 2), and as probed."""
    shmr_amd.set_tuning(uvec=request.param)
    try:
        yield request.param
    finally:
        shmr_amd.set_tuning(uvec=-2)


def test_misaligned(gpu, uvec):
    """RS(8,3), base and pitch odd, len = 4099."""
    c = _case((8, 3, 4099, "plain", True), gpu)
    assert c.shards.data_ptr() % 2 == 1 and c.pitch % 2 == 1
    assert np.array_equal(c.plain_reconstruct(), c.image())
    assert not c.run().any()
    c.same(c.image(), "clean")
    for n, col in enumerate(_columns(c.L)):
        c.reset()
        flips = [(b, int(c.inputs[b][(b + n) % c.k]), col) for b in (0, 1, 2, 3)]
        s = int(c.surplus[4][n % len(c.surplus[4])])
        flips.append((4, s, col))
        c.flip(flips)
        want = np.array(c.rows[:4] + [_bit(s - c.k), 0], np.uint32)
        got = c.run()
        assert np.array_equal(got, want), (col, got, want)
        c.same(c.image(flips), f"column {col}")
    c.reset()
    pad = [(2, int(c.inputs[2][0]), c.L), (2, int(c.surplus[2][0]), c.L)]
    c.flip(pad)
    assert not c.run(rebuild=False).any()
    c.same(c.image(pad, rebuilt=False), "rebuild=False")


def test_capturing_stream_is_refused(gpu):
    """On a stream that is being captured the call returns InvalidArgument,
    enqueues nothing and makes no blocking call; buffer and words are unchanged."""
    import torch
    c = _case((8, 3, 4096 + 48), gpu)
    c.run()                                                       # device init and plan uploads outside the capture
    c.reset()
    c.words.fill_(WORD_SENT)
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    torch.cuda.synchronize()
    with torch.cuda.graph(graph, stream=stream):
        for rebuild in (True, False):
            with pytest.raises(shmr_amd.Error) as e:
                c.rs.reconstruct_checked_batch_dev(c.shards, c.present, shard_len=c.L, rebuild=rebuild,
                                                   out=c.words[1:B + 1])
            assert e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now == st, "a refused call counted or made a blocking call"
    torch.cuda.synchronize()
    c.same(c.start, "refused call")
    assert (c.words.cpu().numpy().view(np.uint32) == WORD_SENT).all()
    assert not c.run().any()
    c.same(c.image(), "after the capture")


@pytest.mark.parametrize("k,p,arrangement", [(8, 3, "plain"), (5, 6, "plain"), (4, 6, "plain"), (2, 34, "plain"),
                                             (8, 3, "list")])
def test_counters(gpu, k, p, arrangement):
    """Every block counts as verified, those with an absent shard also as
    reconstructed; launches grow by one per pattern and group of <= 4 plan rows;
    no slot was added and no kernel_inventory row (encode / reconstruct) moves."""
    c = _case((k, p, 100, arrangement), gpu)
    c.run()                                                       # device init, plan uploads
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}
    degraded = int((~c.present.all(axis=1)).sum())
    for data_only, rebuild in ((False, True), (True, True), (False, False)):
        patterns = {tuple(pr) for pr in c.present}
        groups = 0
        for pr in patterns:
            out_idx = c.rs.checked_plan(list(pr), data_only=data_only, rebuild=rebuild)[1]
            groups += (len(out_idx) + 3) // 4
        c.reset()
        st = shmr_amd.device_stats(0)
        assert not c.run(data_only=data_only, rebuild=rebuild).any()
        now = shmr_amd.device_stats(0)
        assert now["blocks_verified"] - st["blocks_verified"] == B
        assert now["blocks_reconstructed"] - st["blocks_reconstructed"] == degraded
        assert now["launches"] - st["launches"] == groups, (data_only, rebuild)
        assert now["blocks_encoded"] == st["blocks_encoded"] and now["blocking_calls"] == st["blocking_calls"]
        assert list(now) == list(shmr_amd.reed_solomon.DEVICE_COUNTERS) and len(now) == 12
    after = {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}
    assert after == inv
