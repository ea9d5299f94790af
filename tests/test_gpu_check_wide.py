"""Checked reconstruct past tests/test_gpu_check.py's six blocks and five
patterns: the whole store / compare matrix of gf_check_kernel, the union of
difference bits across waves, tiles and launches, the block-list splitter in
three parts, and the input ring's odd tail.  Bit-exact against
oracle/rs_oracle.py and oracle/c_oracle.py; the layout (guards, random padding
that is no codeword, sentinel-filled absent slots, sentinel words around the
result) is test_gpu_check.Case's.

A1  launch_check instantiates gf_check_kernel<R, 1, MODE, F> for R = 1..4 and
    MODE = 0, 1, 2, and nstore in 0..R splits the R rows of a launch group into
    stored and compared ones: 14 (R, nstore) pairs.  RS(4,4) has four parity
    rows, so every plan is one row group, and with a absent shards, d of them
    data,
        a plain call        has 4 rows,          nstore = a;
        rebuild=False       has 4 - a rows,      nstore = 0;
        data_only=True      has d + 4 - a rows,  nstore = d.
    Three batches (plain a = 0..4; rebuild=False a = 1, 2, 3; data_only (d, a)
    = (1,2) (2,3) (3,4) (1,3) (2,4) (1,4)), two blocks per pattern, reach every
    pair; the pairs are derived from ReedSolomon.checked_plan and compared
    with the 14, so a change in plan construction fails here.  Layouts: len =
    4096 + 48 aligned (MODE 0 + MODE 1), len = 100 (MODE 1 only), and base and
    pitch odd at len = 4099 under the knob uvec = 0 (MODE 2 throughout) and as
    probed.
A2  The word of a block is the OR over the waves of a tile, the tiles of a
    block, the full-tile and the partial-tile launch of a row group, and the
    row groups.  len = 8192 + 48: two full tiles and a partial one.
A3  checked_on_device uploads the block list of a pattern whose blocks are no
    arithmetic sequence in parts of CAP = 65,536 blocks; 2 * CAP + 1 blocks
    make three parts, the last of one block.
A4  k = 3 (the input ring's loop runs once, then the odd tail) and k = 1 (no
    loop trip, no look-ahead input).
"""
import time

import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle
from test_gpu_check import ABSENT, GUARD, SENT, WORD_SENT, Case, _bit, _columns, uvec  # noqa: F401  (uvec: the fixture)

pytestmark = pytest.mark.gpu

# ---- the product constants under test, mirrored once ----------------------------
SLOT_BYTES = 256 * 1024     # ec_core.hpp:353  UploadRing::kSlotBytes
CAP = SLOT_BYTES // 4       # ec_core.cpp with_block_lists: u32 block indices per part
MAX_ROWS = 4                # gf_apply.hpp     kern::kMaxRowsPerLaunch

# ---- A1: the absent shards of every pattern, RS(4,4) ----------------------------
K4 = 4
ABSENT_SETS = {
    "plain": [[], [2], [1, 5], [0, 3, 4], [0, 2, 5, 7]],
    "no_rebuild": [[4], [3, 6], [1, 2, 7]],               # parity 0 absent: a compare row's bit is not its row number
    "data_only": [[1, 5], [0, 3, 6], [0, 1, 3, 4], [2, 4, 7], [1, 3, 4, 6], [0, 5, 6, 7]],
}
FLAGS = {"plain": dict(data_only=False, rebuild=True), "no_rebuild": dict(data_only=False, rebuild=False),
         "data_only": dict(data_only=True, rebuild=True)}
ALL_PAIRS = {(r, n) for r in range(1, 5) for n in range(r + 1)}


def _want_pair(kind, absent):
    """(rows, nstore) of one RS(4,4) pattern, from the arithmetic above."""
    a, d = len(absent), sum(1 for i in absent if i < K4)
    return {"plain": (4, a), "no_rebuild": (4 - a, 0), "data_only": (d + 4 - a, d)}[kind]


def _present(kind):
    """Two blocks per pattern: blocks i and i + npat share pattern i."""
    sets = ABSENT_SETS[kind]
    pr = np.ones((len(sets), 2 * K4), np.uint8)
    for i, absent in enumerate(sets):
        pr[i, absent] = 0
    return np.tile(pr, (2, 1))


def _plan_pairs(rs, present, flags):
    """The (rows, nstore) of every row group the call launches, from checked_plan."""
    pairs = []
    for pr in {tuple(p) for p in present.tolist()}:
        out_idx, n_store = rs.checked_plan(list(pr), **flags)[1::2]
        m = len(out_idx)
        for row0 in range(0, m, MAX_ROWS):
            rows = min(MAX_ROWS, m - row0)
            pairs.append((rows, min(max(n_store - row0, 0), rows)))
    return pairs


def _check_calls(c, data_only, rebuild):
    """Clean codewords, one flipped input byte per block, one flipped byte in
    each surplus shard in turn: the words, the whole image, the sentinels."""
    k, B, L = c.k, c.B, c.L
    flags = dict(data_only=data_only, rebuild=rebuild)
    img = dict(data_only=data_only, rebuilt=rebuild)
    cols = _columns(L)
    npat = len({tuple(p) for p in c.present.tolist()})

    def col(b, n):                                                   # rotated over blocks, patterns and rounds
        return cols[(b + b // npat + n) % len(cols)]

    c.reset()
    want = c.image(**img)
    v, clean = c.view(want), c.view(c.clean)
    for b in range(B):
        for i in np.flatnonzero(c.present[b] == 0):
            if rebuild and (i < k or not data_only):
                assert np.array_equal(v[b, i, :L], clean[b, i, :L])       # the oracle rebuilt the codeword
                assert (v[b, i, L:] == ABSENT).all()
            else:
                assert (v[b, i] == ABSENT).all()                          # not rebuilt: the sentinel, whole pitch
    got = c.run(**flags)
    assert not got.any(), got
    c.same(want, "clean")

    c.reset()
    flips = [(b, int(c.inputs[b][b % k]), col(b, 0)) for b in range(B)]
    c.flip(flips)
    got = c.run(**flags)
    assert np.array_equal(got, np.array(c.rows, np.uint32)), (got, c.rows)
    c.same(c.image(flips, **img), "input flips")

    for n in range(max(len(s) for s in c.surplus)):
        c.reset()
        flips, want_words = [], np.zeros(B, np.uint32)
        for b in range(B):
            if len(c.surplus[b]) > n:
                s = int(c.surplus[b][n])
                flips.append((b, s, col(b, n + 1)))
                want_words[b] = _bit(s - k)
        c.flip(flips, x=0x80)
        got = c.run(**flags)
        assert np.array_equal(got, want_words), (n, got, want_words)
        c.same(c.image(flips, x=0x80, **img), f"surplus shard {n}")


_wide = {}


def _matrix_case(kind, L, odd, gpu):
    key = (kind, L, odd)
    if key not in _wide:
        _wide[key] = Case(K4, 4, L, gpu, odd=odd, present=_present(kind))
    return _wide[key]


def test_matrix_is_all_14_pairs():
    """The three batches launch exactly the 14 (R, nstore) pairs, each as the
    only row group of its pattern -- from checked_plan, against the arithmetic."""
    rs = shmr_amd.ReedSolomon(K4, 4)
    seen = set()
    for kind, sets in ABSENT_SETS.items():
        present = _present(kind)
        pairs = _plan_pairs(rs, present, FLAGS[kind])
        assert len(pairs) == len(sets), "a pattern has more than one row group"
        assert sorted(pairs) == sorted(_want_pair(kind, a) for a in sets), kind
        seen |= set(pairs)
    assert seen == ALL_PAIRS and len(ALL_PAIRS) == 14


def _run_matrix(kind, L, odd, gpu):
    c = _matrix_case(kind, L, odd, gpu)
    assert set(_plan_pairs(c.rs, c.present, FLAGS[kind])) == {_want_pair(kind, a) for a in ABSENT_SETS[kind]}
    _check_calls(c, **FLAGS[kind])
    return c


@pytest.mark.parametrize("L", [4096 + 48, 100], ids=["len4144", "len100"])
@pytest.mark.parametrize("kind", list(ABSENT_SETS))
def test_store_compare_matrix(gpu, kind, L):
    """Aligned layout: full tile + partial tile (len 4144), partial tile only (len 100)."""
    c = _run_matrix(kind, L, False, gpu)
    assert c.shards.data_ptr() % 16 == 0 and c.pitch % 16 == 0


@pytest.mark.parametrize("kind", list(ABSENT_SETS))
def test_store_compare_matrix_misaligned(gpu, kind, uvec):
    """Base and pitch odd, len = 4099: the byte-granular kernel at R = 1..4
    under uvec = 0, the vector kernels on unaligned addresses as probed."""
    c = _run_matrix(kind, 4099, True, gpu)
    assert c.shards.data_ptr() % 2 == 1 and c.pitch % 2 == 1


# ---- A2 --------------------------------------------------------------------------
L_OR = 8192 + 48
OR_COLS = [5, 3 * 1024 + 17, 4096 + 2048 + 9, 8192 + 40]   # tile 0 wave 0; tile 0 wave 3; tile 1; the partial tile


@pytest.mark.parametrize("k,p,absent,picks", [(4, 4, [], [4, 5, 6, 7]), (4, 6, [4], [5, 7, 8, 9])],
                         ids=["rs4_4-full", "rs4_6-parity0_absent"])
def test_or_across_waves_tiles_and_launches(gpu, k, p, absent, picks):
    """Block 1: one byte in each of four surplus shards, in four different waves
    of three tiles and two launches (RS(4,6): of both row groups) -- the OR of
    the four bits.  Block 2: one shard flipped at all four places -- its bit.
    Block 4: two shards flipped in the partial tile only.  Blocks 0, 3, 5 clean."""
    present = np.ones((6, k + p), np.uint8)
    present[:, absent] = 0
    c = Case(k, p, L_OR, gpu, present=present)
    assert all(set(picks) <= set(s.tolist()) for s in c.surplus)
    for flags in (dict(rebuild=False), dict(rebuild=True)):
        groups = [g for g in _plan_pairs(c.rs, present[:1], dict(data_only=False, **flags))]
        assert len(groups) == (1 if p == 4 else 2)
        c.reset()
        flips = [(1, s, col) for s, col in zip(picks, OR_COLS)]
        flips += [(2, picks[1], col) for col in OR_COLS]
        flips += [(4, picks[0], OR_COLS[3]), (4, picks[3], 8192 + 1)]
        want = np.zeros(6, np.uint32)
        for b, s, _ in flips:
            want[b] |= _bit(s - k)
        assert bin(int(want[1])).count("1") == 4 and bin(int(want[2])).count("1") == 1
        c.flip(flips, x=0x80)
        got = c.run(**flags)
        assert np.array_equal(got, want), (flags, [hex(x) for x in got], [hex(x) for x in want])
        c.same(c.image(flips, rebuilt=flags["rebuild"], x=0x80), str(flags))


# ---- A3 --------------------------------------------------------------------------
def test_block_list_in_three_parts(gpu):
    """RS(2,2), len 48, pitch 64.  Every block whose index is no multiple of 7
    lacks data shard 1 (one stored + one compared row): 2 * CAP + 1 blocks, no
    arithmetic sequence, so their list is uploaded in parts of CAP, CAP and 1.
    The multiples of 7 in between are all-present (first / stride, no list).
    Damage at the list positions on both sides of each part boundary; every
    word and the whole buffer are compared; the launches counter proves the
    three parts (one per part and row group, plus the all-present pattern's).
    Measured on an MI355X: the call over the 152,919 blocks takes 0.006 s, the
    whole test 0.2 s, so the all-present filler stays."""
    import torch
    k, p, t, L, pitch = 2, 2, 4, 48, 64
    listed = np.flatnonzero(np.arange(3 * CAP) % 7 != 0)[:2 * CAP + 1]
    N = int(listed[-1]) + 1
    full = np.arange(0, N, 7)
    assert len(listed) == 2 * CAP + 1 and len(listed) + len(full) == N
    assert len(set(np.diff(listed[:8]).tolist())) > 1, "the listed blocks must be no arithmetic sequence"
    present = np.ones((N, t), np.uint8)
    present[listed, 1] = 0

    rng = np.random.default_rng(2 * CAP + 1)
    img = np.full(GUARD + N * t * pitch + GUARD, SENT, np.uint8)
    cw = img[GUARD:GUARD + N * t * pitch].reshape(N, t, pitch)
    cw[:] = np.frombuffer(rng.bytes(cw.size), np.uint8).reshape(cw.shape)     # padding: random, no codeword
    par = np.zeros((N, p, L), np.uint8)
    c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k, :L]), par, N, L, 8)
    cw[:, k:, :L] = par
    cw[listed, 1] = ABSENT

    # damage: (block, shard, column); the inputs of a listed block are shards 0 and 2, its surplus is shard 3
    surplus = [(int(listed[pos]), 3, col) for pos, col in
               zip((0, CAP - 1, CAP, 2 * CAP - 1, 2 * CAP), (0, L - 1, 17, 0, L - 1))]
    inputs = [(int(listed[CAP + 1]), 0, L - 1), (int(listed[2 * CAP - 2]), 2, 0)]
    in_full = [(int(full[1]), 1, 5), (int(full[len(full) // 2]), 0, L - 1)]
    want_words = np.zeros(N, np.uint32)
    for b, s, col in surplus + inputs + in_full:
        cw[b, s, col] ^= 0x41
    for b, _, _ in surplus + inputs:
        want_words[b] = _bit(3 - k)               # the one compared row is parity row 1
    for b, _, _ in in_full:
        want_words[b] = _bit(0) | _bit(1)         # a data byte shows in both parity rows
    start = img.copy()
    c_oracle.reconstruct_batch(k, p, cw, present, L, 8)                       # img: the oracle's rebuild, in place
    assert (cw[listed, 1, L:] == ABSENT).all() and not np.array_equal(img, start)

    rs = shmr_amd.ReedSolomon(k, p)
    buf = torch.from_numpy(start).to(gpu)
    shards = torch.as_strided(buf, (N, t, pitch), (t * pitch, pitch, 1), GUARD)
    words = torch.full((N + 2,), WORD_SENT, dtype=torch.int32, device=gpu)
    shmr_amd.device_init(0)
    torch.cuda.synchronize()
    st = shmr_amd.device_stats(0)
    t0 = time.perf_counter()
    rs.reconstruct_checked_batch_dev(shards, present, shard_len=L, out=words[1:N + 1])
    torch.cuda.synchronize()
    print(f"checked call over {N} blocks: {time.perf_counter() - t0:.3f} s")
    now = shmr_amd.device_stats(0)

    parts = -(-len(listed) // CAP)
    groups_listed = -(-(1 + 1) // MAX_ROWS)       # one stored + one compared row
    groups_full = -(-p // MAX_ROWS)
    assert parts == 3
    assert now["launches"] - st["launches"] == parts * groups_listed + groups_full
    assert now["blocks_verified"] - st["blocks_verified"] == N
    assert now["blocks_reconstructed"] - st["blocks_reconstructed"] == len(listed)

    w = words.cpu().numpy().view(np.uint32)
    assert w[0] == WORD_SENT and w[N + 1] == WORD_SENT, "a word next to the result was written"
    bad = np.flatnonzero(w[1:N + 1] != want_words)
    assert bad.size == 0, f"{bad.size} words differ, first at block {int(bad[0])}: " \
                          f"{int(w[1 + bad[0]]):#x}, expected {int(want_words[bad[0]]):#x}"
    assert int((want_words != 0).sum()) == 9
    got = buf.cpu().numpy()
    bad = np.flatnonzero(got != img)
    assert bad.size == 0, f"{bad.size} bytes differ, first at {int(bad[0])} " \
                          f"(block {(int(bad[0]) - GUARD) // (t * pitch)}, block pitch {t * pitch})"


# ---- A4 --------------------------------------------------------------------------
@pytest.mark.parametrize("L", [100, 4096 + 48], ids=["len100", "len4144"])
@pytest.mark.parametrize("k", [3, 1])
def test_input_ring_tails(gpu, k, L):
    """RS(3,2): one trip of the two-input loop, then the single-input tail.
    RS(1,2): the tail alone.  The six patterns of test_gpu_check.py."""
    c = Case(k, 2, L, gpu)
    for flags in FLAGS.values():
        _check_calls(c, **flags)
