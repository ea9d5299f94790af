"""Two-shard location and repair on the GPU (gf_locate.hip through
shmr_ec_locate_pair_batch_dev and shmr_ec_scrub_pair_batch_dev) against the
first-group rule of tests/locate_pair_ref.py on the same bytes.

Layout of every case, as tests/test_gpu_locate.py: separate data and parity
regions in one device buffer with guard bytes around them, a shard pitch above
len whose padding holds random bytes that are not a codeword, result arrays
with sentinel entries around them and guarded scratch.

The damage table (damage_of), 12 blocks: clean; one data shard; one parity
shard; two parity shards; two data shards in one column; in columns of
different tiles; in different waves of one tile; a data and a parity shard in
the last valid byte; two data shards in the bytes of the partial tile only; a
data shard with parity shard 0; a data shard with the last parity shard (for
p > 4 beyond the group: reported as the data shard alone); three shards.  The
answers of blocks 0-10 follow from the construction and are asserted; block 11
is compared with the rule only (p = 4: three shards can pass for two).
"""
import ctypes

import numpy as np
import pytest

import shmr_amd
from locate_cases import GUARD, SENT, TILE, WAVE, HostCase
from locate_pair_ref import CLEAN, NONE, locate_pair_rule

pytestmark = pytest.mark.gpu

MAX_DATA = 29                                             # locate_plan.hpp pair_max_data
CODES = [(10, 4), (4, 4), (5, 5), (MAX_DATA, 4)]          # RS(5,5): a row beyond the group; RS(29,4): 17 bitmap words
LENGTHS = [TILE, 2 * TILE + 48, TILE + 3, 17, 1]          # one mode and boundary each; TILE + 3 at an odd base offset
B = 12
WORD_SENT = 0x5A5A5A5A
INVALID = -100


def damage_of(k, p, L):
    """[(block, shard, column, xor)] and the answers of blocks 0 .. 10."""
    last = L - 1
    col = lambda c: min(c, last)
    tail0 = min(L // TILE * TILE, last)                   # first byte of the partial tile (of the last tile without one)
    a, b = 1, k - 1
    d = [(1, a, col(L // 2), 0x41),
         (2, k + 1, col(L // 3), 0x41),
         (3, k, col(5), 0x41), (3, k + 3, col(L // 2), 0x17),
         (4, a, col(L // 3), 0x41), (4, b, col(L // 3), 0x17),
         (5, a, col(7), 0x41), (5, b, last, 0x17),
         (6, 0, col(7), 0x5B), (6, b, col(3 * WAVE + 9), 0x22),
         (7, 2, last, 0x9D), (7, k + 2, last, 0x41),
         (8, 0, tail0, 0x41), (8, a, last, 0xFF),
         (9, b, col(9), 0x33), (9, k, col(2 * WAVE + 1), 0x41),
         (10, a, col(11), 0x41), (10, k + p - 1, col(WAVE + 5), 0x17),
         (11, 0, col(3), 0x41), (11, 2, col(L // 2), 0x17), (11, k + 1, last, 0x5B)]
    want = [(CLEAN, CLEAN), (a, CLEAN), (k + 1, CLEAN), (k, k + 3), (a, b), (a, b), (0, b), (2, k + 2), (0, a),
            (b, k), (a, k + p - 1) if p == 4 else (a, CLEAN)]
    return d, want


class Case(HostCase):
    """Codewords of one (k, p, L) in the guarded two-region device layout."""

    def __init__(self, k, p, L, gpu, seed, odd=False, nblk=B, pitch=None):
        import torch
        super().__init__(k, p, L, seed, nblk=nblk, odd=odd, pitch=pitch)
        self.gpu = gpu
        self.rs = shmr_amd.ReedSolomon(k, p)
        self.words = torch.empty(nblk + 2, dtype=torch.int32, device=gpu)
        self.located = torch.empty(2 * nblk + 4, dtype=torch.int32, device=gpu)
        self.need = self.rs.locate_pair_work_size(nblk)
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

    def rule(self, blocks=None, cols=None):
        """locate_pair_rule of the host copy of what the device holds ->
        {block: (first, second)}; `cols`: only these columns (every other column
        of the block must be a codeword column: it eliminates nobody)."""
        d, q = self.regions(self.img)
        cols = slice(0, self.L) if cols is None else cols
        return {int(b): locate_pair_rule(self.k, self.p, d[b][:, cols], q[b][:, cols])
                for b in (range(self.B) if blocks is None else blocks)}

    def locate(self, stream=None):
        """One shmr_ec_locate_pair_batch_dev into the guarded result arrays ->
        (status, words [B] uint32, located [B, 2] int32); sentinels checked."""
        import torch
        B = self.B
        self.words.fill_(WORD_SENT)
        self.located.fill_(WORD_SENT)
        self.work.fill_(SENT)
        v = ctypes.c_void_p
        rc = self.rs._L.shmr_ec_locate_pair_batch_dev(
            self.rs._h, v(self.data.data_ptr()), self.pitch, self.k * self.pitch, v(self.parity.data_ptr()),
            self.pitch, self.p * self.pitch, B, self.L, v(self.words.data_ptr() + 4), v(self.located.data_ptr() + 8),
            v(self.work.data_ptr() + GUARD), self.need, 0,
            v(torch.cuda.current_stream().cuda_stream if stream is None else stream))
        torch.cuda.synchronize()
        w = self.words.cpu().numpy().view(np.uint32)
        loc = self.located.cpu().numpy()
        work = self.work.cpu().numpy()
        assert w[0] == WORD_SENT and w[B + 1] == WORD_SENT, "a word next to d_mismatch was written"
        assert (loc[:2] == WORD_SENT).all() and (loc[2 * B + 2:] == WORD_SENT).all(), "an entry next to d_located was written"
        assert (work[:GUARD] == SENT).all() and (work[GUARD + self.need:] == SENT).all(), "the scratch was overrun"
        return rc, w[1:B + 1].copy(), loc[2:2 * B + 2].reshape(B, 2).copy()

    def unchanged(self):
        got = self.buf.cpu().numpy()
        bad = np.flatnonzero(got != self.img)
        assert bad.size == 0, f"{bad.size} bytes of the shard buffer changed, first at {int(bad[0])}"


def _check(c, rule, want=None):
    """Locate what the device holds: the rule's answers (and the table's),
    verify's words, locate's answers wherever it has one, nothing else written."""
    rc, words, located = c.locate()
    assert rc == 0
    if want is not None:
        assert [rule[b] for b in range(len(want))] == want, "the rule disagrees with the constructed answers"
    got = {b: tuple(int(x) for x in located[b]) for b in rule}
    assert got == rule, {b: (got[b], rule[b]) for b in rule if got[b] != rule[b]}
    verify = c.rs.verify_batch_dev(c.data, c.parity, shard_len=c.L).cpu().numpy().view(np.uint32)
    assert np.array_equal(words, verify), (words, verify)
    _, single = c.rs.locate_batch_dev(c.data, c.parity, shard_len=c.L)
    single = single.cpu().numpy()
    has = single != NONE
    assert np.array_equal(located[has, 0], single[has]) and (located[has, 1] == CLEAN).all()
    c.unchanged()
    return located


@pytest.fixture(params=["device", "byte_granular"])
def misaligned_path(request):
    """Misaligned shards as the device runs them, and as a device without
    unaligned vector access does: the byte-granular kernel (knob uvec = 0)."""
    if request.param == "byte_granular":
        shmr_amd.set_tuning(uvec=0)
    try:
        yield request.param
    finally:
        shmr_amd.set_tuning(uvec=-2)


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", CODES)
def test_damage_table(gpu, k, p, L):
    odd = L == TILE + 3
    if odd:
        shmr_amd.set_tuning(uvec=0)                       # the byte-granular kernel (MODE 2)
    try:
        c = Case(k, p, L, gpu, seed=(k * 64 + p) * 7 + L, odd=odd)
        _check(c, {b: (CLEAN, CLEAN) for b in range(B)})   # pristine, although every shard's padding is random
        damage, want = damage_of(k, p, L)
        c.load(c.damaged(damage))
        located = _check(c, c.rule(), want)
        # the tensor forms return the same
        mismatch, loc = c.rs.locate_pair_batch_dev(c.data, c.parity, shard_len=c.L)
        assert mismatch.shape == (B,) and loc.shape == (B, 2) and loc.device == c.buf.device
        assert np.array_equal(loc.cpu().numpy(), located)
        c.unchanged()
    finally:
        shmr_amd.set_tuning(uvec=-2)


def test_misaligned_shards_on_both_paths(gpu, misaligned_path):
    k, p, L = 10, 4, TILE + 48
    c = Case(k, p, L, gpu, seed=5, odd=True)
    damage, want = damage_of(k, p, L)
    c.load(c.damaged(damage))
    _check(c, c.rule(), want)


def test_without_the_skip_shortcut(gpu):
    """Every candidate tested in every damaged tile (knob pair_skip = 0): the same answers."""
    k, p, L = 10, 4, 2 * TILE + 48
    c = Case(k, p, L, gpu, seed=6)
    damage, want = damage_of(k, p, L)
    c.load(c.damaged(damage))
    shmr_amd.set_tuning(pair_skip=0)
    try:
        _check(c, c.rule(), want)
    finally:
        shmr_amd.set_tuning(pair_skip=-2)


def test_more_tiles_than_the_grid(gpu):
    """RS(10,4), worklist x tiles_per_block above the bounded grid (8 workgroups
    per CU): damage in the first and the last tile of each block.  The rule is
    evaluated on the damaged columns: every other column is a codeword column
    of the oracle's, which eliminates nobody."""
    import torch
    k, p = 10, 4
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    nblk = 12
    tiles = -(-(cus * 8 + 1) // nblk)                     # tiles per block: nblk * tiles > cus * 8
    L = tiles * TILE
    assert nblk * (L // TILE) > cus * 8
    c = Case(k, p, L, gpu, seed=77, nblk=nblk, pitch=L)
    damage, want = [], {}
    for b in range(nblk):
        e, f = b % k, (b + 3) % k if b % 2 else k + b % 4
        e, f = min(e, f), max(e, f)
        damage += [(b, e, 17 + b, 0x41), (b, f, L - 1 - 16 * b, 0x17)]
        want[b] = (e, f)
    c.load(c.damaged(damage))
    cols = sorted({col for _, _, col, _ in damage})
    rule = c.rule(cols=cols)
    assert rule == want
    _check(c, rule)


def test_worklist_among_clean_blocks(gpu):
    """40 damaged-pair blocks among 100 in shuffled positions: the worklist's
    order does not matter and blocks that are not on it keep locate's answers."""
    k, p, L, nblk = 10, 4, TILE + 16, 100
    c = Case(k, p, L, gpu, seed=78, nblk=nblk)
    rng = np.random.default_rng(9)
    order = rng.permutation(nblk)
    damage, want = [], {int(b): (CLEAN, CLEAN) for b in range(nblk)}
    for i, b in enumerate(order[:40]):
        e, f = sorted(rng.choice(k + 4, 2, replace=False).tolist())
        ce, cf = int(rng.integers(0, L)), int(rng.integers(0, L))
        damage += [(int(b), e, ce, 0x41), (int(b), f, cf, 0x17)]
        want[int(b)] = (e, f)
    for i, b in enumerate(order[40:60]):                  # single shards in between
        e = int(rng.integers(0, k + p))
        damage.append((int(b), e, int(rng.integers(0, L)), 0x5B))
        want[int(b)] = (e, CLEAN)
    c.load(c.damaged(damage))
    cols = sorted({col for _, _, col, _ in damage})
    rule = c.rule(cols=cols)
    assert rule == want
    _check(c, rule)


@pytest.mark.parametrize("k,p,L", [(10, 4, 2 * TILE + 48), (5, 5, TILE + 3), (MAX_DATA, 4, 17)])
def test_scrub_pair(gpu, k, p, L):
    c = Case(k, p, L, gpu, seed=k * 100 + p)
    damage, want = damage_of(k, p, L)
    c.load(c.damaged(damage))
    rule = c.rule()
    located, counts = c.rs.scrub_pair_batch_dev(c.data, c.parity, shard_len=L)
    assert located.shape == (B, 2) and sum(counts) == B
    after = c.buf.cpu().numpy()
    d0, q0 = c.regions(c.pristine)
    d1, q1 = c.regions(after)
    di, qi = c.regions(c.img)
    expect = [0, 0, 0, 0]
    for b in range(B):
        got = tuple(int(x) for x in located[b])
        hit_beyond = p > 4 and b == 10                    # a data shard and parity shard p - 1, beyond the group
        if rule[b] == (CLEAN, CLEAN):
            assert got == rule[b]
            expect[0] += 1
        elif rule[b] == (NONE, NONE) or hit_beyond:
            assert got == (NONE, NONE), (b, got)
            expect[3] += 1
        elif b == 11:                                     # three shards: whatever the closing verify says
            expect[3 if got == (NONE, NONE) else (2 if got[1] >= 0 else 1)] += 1
            continue
        else:
            assert got == rule[b] == want[b], (b, got)
            expect[2 if got[1] >= 0 else 1] += 1
        if got[0] >= 0 or rule[b] == (CLEAN, CLEAN):      # repaired (or clean): the oracle's original bytes
            assert np.array_equal(d1[b, :, :L], d0[b, :, :L]) and np.array_equal(q1[b, :, :L], q0[b, :, :L]), b
        elif hit_beyond:                                  # demoted: the located data shard has been rewritten
            a = rule[b][0]
            keep = [i for i in range(k) if i != a]
            assert np.array_equal(d1[b, keep, :L], di[b, keep, :L]) and np.array_equal(q1[b, :, :L], qi[b, :, :L])
        else:                                             # reported NONE: not written
            assert np.array_equal(d1[b], di[b]) and np.array_equal(q1[b], qi[b]), b
    assert list(counts) == expect, (counts, expect)
    # nothing outside [0, L) of any shard, and no guard byte, was written
    mask = np.ones(after.size, bool)
    for off, n in ((c.data_off, k), (c.par_off, p)):
        region = mask[off:off + B * n * c.pitch].reshape(B, n, c.pitch)
        region[:, :, :L] = False
    assert np.array_equal(after[mask], c.img[mask])


def test_capturing_stream_is_refused(gpu):
    """The pair calls stay out of graphs, as locate and scrub: on a capturing
    stream both return InvalidArgument and nothing is enqueued."""
    import torch
    k, p, L = 10, 4, TILE + 48
    c = Case(k, p, L, gpu, seed=12)
    shmr_amd.device_init(0)
    assert c.locate()[0] == 0                             # plan uploads outside the capture
    st = shmr_amd.device_stats(0)
    graph = torch.cuda.CUDAGraph()
    stream = torch.cuda.Stream()
    c.words.fill_(WORD_SENT)
    c.located.fill_(WORD_SENT)
    torch.cuda.synchronize()
    v = ctypes.c_void_p
    with torch.cuda.graph(graph, stream=stream):
        rc = c.rs._L.shmr_ec_locate_pair_batch_dev(
            c.rs._h, v(c.data.data_ptr()), c.pitch, k * c.pitch, v(c.parity.data_ptr()), c.pitch, p * c.pitch, B, L,
            v(c.words.data_ptr() + 4), v(c.located.data_ptr() + 8), v(c.work.data_ptr() + GUARD), c.need, 0,
            v(torch.cuda.current_stream().cuda_stream))
        with pytest.raises(shmr_amd.Error) as e:
            c.rs.scrub_pair_batch_dev(c.data, c.parity, shard_len=L)
    assert rc == INVALID and e.value.name == "InvalidArgument"
    now = shmr_amd.device_stats(0)
    assert now["launches"] == st["launches"] and now["blocks_verified"] == st["blocks_verified"]
    assert now["blocking_calls"] == st["blocking_calls"], "a blocking HIP call inside the capture"
    torch.cuda.synchronize()
    assert (c.words.cpu().numpy() == WORD_SENT).all() and (c.located.cpu().numpy() == WORD_SENT).all()
    c.data[3, 5, 4100] ^= 8
    c.data[3, 7, 20] ^= 9
    rc, words, located = c.locate()
    assert rc == 0 and words.tolist() == [0, 0, 0, 15] + [0] * 8
    assert located[3].tolist() == [5, 7] and (np.delete(located, 3, 0) == CLEAN).all()
