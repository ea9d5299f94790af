"""Plans of more than four output rows, on every launch form, vs the CPU
oracle, bit-exact.

A launch handles at most four output rows (gf_apply.hpp kMaxRowsPerLaunch); an
encode with p > 4 parity shards or a rebuild of m > 4 shards runs as several
launches (ec_core.cpp launch_set), each with its own row0 and usually its own
kernel: m = 6 is a 4-row launch (U = 2, 8 KiB tiles) followed by a 2-row launch
(U = 1, 4 KiB tiles).  The follow-on launches use row0 arithmetic of their own
(the table index (t*m + row0 + r), out_idx[row0 + r] - out_bias, the pointer-
row entry bp[k + row0 + r]: gf_tile.hpp stage_plan / stage_issue) and see
another tile size than the first, so one shard length can be tail-only for the
first launch and full tiles plus a fused tail for the second.  The kernel sweep
(test_gpu_kernel_sweep.py) launches every kernel with row0 == 0; this module
crosses the row groups beyond the first with every launch form: pitch batches,
slot lattices in one run, in segment runs and past the segment limit, the
submission queue, scattered pointer tables, mapped host memory, the realigning
and byte-granular kernels, compact outputs and fresh buffers.

Every case checks (1) every output byte against the oracle, (2) that every
other byte of the buffers (guards, slot tails, free slots, present shards,
absent parity under data_only) still holds what it held -- the whole buffer is
compared with an expected image -- and (3) that the call took the path the
case is named for: the run count (a mirror of the run split, asserted exactly)
plus the ptr_table_grids counter and the kernel_inventory rows that gained
launches at rows == 4 and at the remainder row count.  The partial-tile kernel
(mode 1) serves every launch form and carries no flags, so a row group whose
tile is longer than the shard shows its form by run count and counter only.

Erasure patterns lose five data shards or more wherever the code has them
(data_only then still rebuilds m >= 5 rows); RS(3,9) has three data shards,
so its data_only rebuild is the one-group control of its nine-row rebuild."""
import ctypes

import numpy as np
import pytest

import shmr_amd
from shmr_amd.reed_solomon import _RawView, _ptr, _u8p
from oracle import c_oracle

pytestmark = pytest.mark.gpu

SENT, POISON = 0xC3, 0xEE     # bytes no call may touch; the content of lost shards

# m = 4+1, 4+2, 4+3, 4+4 and 4+4+1 rows, small and large k
CODES = [(5, 5), (10, 6), (4, 7), (6, 8), (3, 9)]
# the smallest lengths at which the two tile sizes (U = 2: 8 KiB, U = 1: 4 KiB) disagree
LENGTHS = [1000, 4096 + 48, 8192, 8192 + 48, 12288 - 16]
SPLIT = [4096 + 48, 8192 + 48, 12288 - 16]
BIG = [4096 + 48, 8192 + 48]      # pools and batches of 100 blocks or more

# kernel template flags (gf_apply.hpp: never renumbered)
K_NT_LOAD, K_FUSE, K_PTRS, K_SEGS, K_SC1 = 1, 1 << 18, 1 << 19, 1 << 20, 1 << 23
MODE3_FLAGS = 1 | 2 | 512         # the realigning kernel's instantiation

# shards lost per code: five data shards or more where the code has them
LOST = {(5, 5): [0, 1, 2, 3, 4], (10, 6): [0, 2, 3, 6, 9, 11], (6, 8): [0, 1, 2, 4, 5, 7, 10, 13],
        (3, 9): [0, 1, 2, 4, 5, 7, 8, 10, 11]}
# two 5-erasure patterns per code of the pool and queue cases (RS(10,6): all data)
FIVE = {(5, 5): ([0, 1, 2, 3, 4], [0, 1, 2, 3, 5]), (10, 6): ([0, 2, 3, 6, 9], [1, 2, 4, 7, 8])}
HOLES = (3, 4, 9, 15, 16, 17, 21)  # freed slots of the 24-slot pool: 17 live slots in 5 runs


# ---- oracle ---------------------------------------------------------------------
def _codewords(k, p, B, L, seed):
    rng = np.random.default_rng(seed)
    cw = np.empty((B, k + p, L), np.uint8)
    cw[:, :k] = rng.integers(0, 256, (B, k, L), dtype=np.uint8)
    par = np.zeros((B, p, L), np.uint8)
    c_oracle.encode_batch(k, p, np.ascontiguousarray(cw[:, :k]), par, B, L, 8)
    cw[:, k:] = par
    return cw


def _rebuilt(k, p, cw, present, data_only):
    """The oracle's reconstruct of every block from its present shards ->
    (shards [B, t, L], written [B, t]: the shards the call must write)."""
    work = cw.copy()
    work[present == 0] = 0
    c_oracle.reconstruct_batch(k, p, work, present, cw.shape[2], 8, data_only=data_only)
    written = present == 0
    if data_only:
        written[:, k:] = False
    return work, written


def _present(B, t, lost_of):
    pr = np.ones((B, t), np.uint8)
    for b in range(B):
        pr[b, list(lost_of(b))] = 0
    return pr


def _in_place(cw, present, work, written):
    """(start, want) shard bytes of an in-place rebuild: lost shards hold
    POISON, the written ones end as the oracle's."""
    start = cw.copy()
    start[present == 0] = POISON
    want = start.copy()
    want[written] = work[written]
    return start, want


def _same(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    at = tuple(int(x) for x in bad[0])
    raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {at}: {int(got[at]):#04x}, "
                         f"expected {int(want[at]):#04x}")


# ---- path checks ------------------------------------------------------------------
def _runs(slots):
    """Mirror of ec_core launch_slots' run split: maximal arithmetic runs of
    the ascending slots, greedily from the left."""
    s = sorted(int(x) for x in slots)
    runs, i = 0, 0
    while i < len(s):
        e = i + 1
        st = s[e] - s[i] if e < len(s) else 1
        while e < len(s) and s[e] - s[e - 1] == st:
            e += 1
        runs += 1
        i = e
    return runs


def _pattern_runs(present, slots, k, data_only):
    """Mirror of ec_core reconstruct_on_device's grouping: blocks by erasure
    pattern, patterns by the number of rows they rebuild -> {m: (patterns,
    runs)}, the runs of each pattern's (ascending) slots added up."""
    by_pattern = {}
    for row, s in sorted(zip((bytes(r) for r in np.asarray(present)), (int(x) for x in slots)), key=lambda x: x[1]):
        if all(row):
            continue
        by_pattern.setdefault(row, []).append(s)
    by_m = {}
    for pat, sl in by_pattern.items():
        m = sum(1 for i, x in enumerate(pat) if not x and (i < k or not data_only))
        if m == 0:
            continue
        c = by_m.setdefault(m, [0, 0])
        c[0] += 1
        c[1] += _runs(sl)
    return {m: tuple(c) for m, c in by_m.items()}


def _inventory():
    return {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}


def _gained(before):
    after = _inventory()
    assert after.keys() == before.keys()
    gained = {key: after[key] - before[key] for key in after if after[key] != before[key]}
    print("kernels (rows, U, mode, flags) -> launches:", {(r, c, mode, hex(f)): v for (r, c, mode, f), v in gained.items()})
    return gained


def _row_groups(m):
    return [min(4, m - row0) for row0 in range(0, m, 4)]


def _assert_groups(gained, m, L, need=0, forbid=0):
    """Every row group of an m-row plan at shard length L ran the kernel its
    form and length call for: a full-tile kernel (mode 0, U = 2 for four rows)
    with the flags `need` and none of `forbid`, with fused tails exactly when
    the length leaves a partial tile -- or, where the shard is shorter than
    the group's tile, the partial-tile kernel (mode 1).  Two groups of the same
    row count (m = 8) must show as two launches."""
    want = {}
    for rows in _row_groups(m):
        want[rows] = want.get(rows, 0) + 1
    for rows, n in want.items():
        u = 2 if rows == 4 else 1
        tile = 4096 * u
        if L < tile:
            got = gained.get((rows, 1, 1, 0), 0)
        else:
            got = sum(v for (r, c, mode, f), v in gained.items()
                      if r == rows and c == u and mode == 0 and f & need == need and not f & forbid
                      and bool(f & K_FUSE) == (L % tile != 0))
        assert got >= n, (f"rows={rows} (m={m}, len={L}): {got} launches of the expected kernel "
                          f"(need {need:#x}, forbid {forbid:#x}), wanted {n}; gained {gained}")


def _no_flag(gained, flag):
    assert not [key for key in gained if key[2] == 0 and key[3] & flag], (hex(flag), gained)


def _grids():
    return shmr_amd.device_stats(0)["ptr_table_grids"]


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _tab(rows):
    arr = np.ascontiguousarray(np.asarray(rows, dtype=np.uint64).reshape(-1))
    return arr, arr.ctypes.data_as(ctypes.POINTER(_u8p))


def _pitch(L):
    return (L + 255) // 256 * 256 + 256


# ---- a pool with holes ----------------------------------------------------------------
class _Pool:
    """ShardPool(t, S, nslots) with every slot allocated, then `free` given
    back.  view: the whole slab as a [nslots, t, slot pitch] tensor."""

    def __init__(self, gpu, t, S, nslots, free):
        import torch
        self.pool = shmr_amd.ShardPool(t, S, nslots)
        self.blocks = [self.pool.alloc() for _ in range(nslots)]     # by slot
        self.P = int(self.blocks[0][1] - self.blocks[0][0])
        base = int(self.blocks[0][0])
        assert self.pool.stats() == {"slabs": 1, "slots": nslots, "in_use": nslots}
        for s, blk in enumerate(self.blocks):
            assert [int(a) for a in blk] == [base + (s * t + i) * self.P for i in range(t)]
        self.view = torch.as_tensor(_RawView(self.pool, base, (nslots, t, self.P)), device=gpu)
        for s in sorted(free, reverse=True):
            self.pool.free(self.blocks[s])
        self.live = [s for s in range(nslots) if s not in set(free)]
        self.nslots, self.t, self.S = nslots, t, S

    def image(self, shards):
        """Host image of the slab: SENT everywhere but the live slots' shards
        (shards [live blocks, t, S], slot order)."""
        img = np.full((self.nslots, self.t, self.P), SENT, np.uint8)
        img[self.live, :, :self.S] = shards
        return img

    def upload(self, img):
        import torch
        self.view.copy_(torch.from_numpy(img).to(self.view.device))
        torch.cuda.synchronize()

    def table(self, order):
        """Address rows of the live blocks live[order[0]], live[order[1]], ..."""
        return np.stack([self.blocks[self.live[int(j)]] for j in order])


def _encode_pool(gpu, k, p, S, nslots, free, seed):
    t = k + p
    pool = _Pool(gpu, t, S, nslots, free)
    cw = _codewords(k, p, len(pool.live), S, seed)
    start = cw.copy()
    start[:, k:] = POISON
    pool.upload(pool.image(start))
    return pool, cw


def _decode_pool(gpu, k, p, S, present, data_only, seed, pool=None):
    t = k + p
    pool = pool or _Pool(gpu, t, S, 24, HOLES)
    cw = _codewords(k, p, len(pool.live), S, seed)
    work, written = _rebuilt(k, p, cw, present, data_only)
    start, want = _in_place(cw, present, work, written)
    pool.upload(pool.image(start))
    return pool, want


# =================================== encode ===================================
def _run_encode_pitch(gpu, k, p, L, seed):
    import torch
    B, pitch = 6, _pitch(L)
    cw = _codewords(k, p, B, L, seed)
    dimg = np.full((B, k, pitch), SENT, np.uint8)
    dimg[:, :, :L] = cw[:, :k]
    pimg = np.full((B, p, pitch), SENT, np.uint8)
    data, parity = torch.from_numpy(dimg).to(gpu), torch.from_numpy(pimg).to(gpu)
    torch.cuda.synchronize()
    inv = _inventory()
    shmr_amd.ReedSolomon(k, p).encode_batch_dev(data, parity, shard_len=L)
    torch.cuda.synchronize()
    _assert_groups(_gained(inv), p, L, forbid=K_SEGS | K_PTRS)
    pimg[:, :, :L] = cw[:, k:]
    _same(parity.cpu().numpy(), pimg, "parity")
    _same(data.cpu().numpy(), dimg, "data")


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", CODES)
def test_e1_pitch_batch(gpu, k, p, L):
    """The control: a pitch batch of six blocks, aligned pitches.  If this
    passes and a later case fails, the fault is in the launch form."""
    _run_encode_pitch(gpu, k, p, L, [1, k, p, L])


@pytest.mark.parametrize("L", SPLIT)
@pytest.mark.parametrize("k,p", CODES)
def test_e2_slot_lattice_few_runs(gpu, k, p, L):
    """The 17 live blocks of a 24-slot pool with holes, in shuffled table
    order: one lattice call over 5 segment runs."""
    pool, cw = _encode_pool(gpu, k, p, L, 24, HOLES, [2, k, p, L])
    assert len(pool.live) == 17 and _runs(pool.live) == 5
    rs = shmr_amd.ReedSolomon(k, p)
    order = np.random.default_rng(L).permutation(len(pool.live))
    keep, tab = _tab(pool.table(order))
    g0, inv = _grids(), _inventory()
    assert rs._L.shmr_ec_encode_ptrs_dev(rs._h, tab, len(order), L, 0, _stream()) == 0
    import torch
    torch.cuda.synchronize()
    assert _grids() == g0 + 1
    gained = _gained(inv)
    _assert_groups(gained, p, L, need=K_SEGS, forbid=K_PTRS)
    _no_flag(gained, K_PTRS)
    _same(pool.view.cpu().numpy(), pool.image(cw), "slab")


@pytest.mark.parametrize("L", BIG)
@pytest.mark.parametrize("pairs", [32, 33])
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_e3_slot_lattice_at_the_run_limit(gpu, k, p, pairs, L):
    """Slots 3j and 3j + 1 live, 3j + 2 free: every pair is one run (a row of
    singletons would merge into one strided run).  32 runs stay on the lattice
    (segment kernels); 33 take the table kernels -- the same bytes."""
    import torch
    nslots = 3 * pairs
    pool, cw = _encode_pool(gpu, k, p, L, nslots, range(2, nslots, 3), [3, k, p, L, pairs])
    assert _runs(pool.live) == pairs
    rs = shmr_amd.ReedSolomon(k, p)
    order = np.random.default_rng(pairs).permutation(len(pool.live))
    keep, tab = _tab(pool.table(order))
    g0, inv = _grids(), _inventory()
    assert rs._L.shmr_ec_encode_ptrs_dev(rs._h, tab, len(order), L, 0, _stream()) == 0
    torch.cuda.synchronize()
    gained = _gained(inv)
    if pairs <= 32:
        assert _grids() == g0 + 1
        _assert_groups(gained, p, L, need=K_SEGS, forbid=K_PTRS)
        _no_flag(gained, K_PTRS)
    else:
        assert _grids() == g0
        _assert_groups(gained, p, L, need=K_PTRS, forbid=K_SEGS)
        _no_flag(gained, K_SEGS)
    _same(pool.view.cpu().numpy(), pool.image(cw), "slab")


def _queue_merged(q0, q1, requests):
    assert q1["requests"] - q0["requests"] == requests
    assert q1["batches"] - q0["batches"] < requests, "no call was merged"
    assert q1["max_batch"] > 1


@pytest.mark.parametrize("L", BIG)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_e4_through_the_queue(gpu, k, p, L):
    """One started shmr_ec_encode_dev per live block of the pool with holes,
    in shuffled order, under a coalescing window: merged batches over the
    slots, exact."""
    pool, cw = _encode_pool(gpu, k, p, L, 24, HOLES, [4, k, p, L])
    rs = shmr_amd.ReedSolomon(k, p)
    order = np.random.default_rng(L + 1).permutation(len(pool.live))
    q0, g0, inv = shmr_amd.queue_stats(0), _grids(), _inventory()
    shmr_amd.set_tuning(coalesce_us=3000)
    try:
        ops = [rs.encode_dev([(int(a), L) for a in row], start=True) for row in pool.table(order)]
        for op in ops:
            op.wait()
    finally:
        shmr_amd.set_tuning(coalesce_us=-2)
    _queue_merged(q0, shmr_amd.queue_stats(0), len(order))
    assert _grids() > g0
    gained = _gained(inv)
    assert sum(v for (r, c, mode, f), v in gained.items() if r == 4) >= 1 and \
        sum(v for (r, c, mode, f), v in gained.items() if r == p - 4) >= 1, gained
    _same(pool.view.cpu().numpy(), pool.image(cw), "slab")


def _scatter(B, t, L, seed, off3=None):
    """Byte offsets [B, t] of shards at unrelated places of one arena (cells in
    random order, each shard a random multiple of 16 into its cell; off3: one
    (block, shard) 3 bytes off alignment) and the arena's size."""
    rng = np.random.default_rng(seed)
    cell = _pitch(L) + 256
    offs = (rng.permutation(B * t) * cell + 64 + 16 * rng.integers(0, 12, B * t)).reshape(B, t)
    if off3 is not None:
        offs[off3] += 3
    return offs, B * t * cell + 64


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("form", ["aligned", "off3", "mapped"])
@pytest.mark.parametrize("k,p", [(4, 7), (10, 6)])
def test_e5_scattered_tables_and_mapped_host(gpu, k, p, form, L):
    """Shards at unrelated offsets of one arena, so no grid fits: the pointer-
    table kernels, every shard aligned or one second-group parity shard 3
    bytes off; and the same over mapped host memory (zero-copy)."""
    import torch
    B, t = 6, k + p
    cw = _codewords(k, p, B, L, [5, k, p, L])
    offs, size = _scatter(B, t, L, [k, L], off3=(1, k + 4) if form == "off3" else None)
    img = np.full(size, SENT, np.uint8)
    want = img.copy()
    for b in range(B):
        for i in range(t):
            o = int(offs[b, i])
            img[o:o + L] = cw[b, i] if i < k else POISON
            want[o:o + L] = cw[b, i]
    rs = shmr_amd.ReedSolomon(k, p)
    g0, inv = _grids(), _inventory()
    if form == "mapped":
        buf = shmr_amd.PinnedBuffer(size)
        buf.array[:] = img
        z0, _ = shmr_amd.path_stats()
        rs.encode_blocks_host([[buf.array[int(o):int(o) + L] for o in row] for row in offs])
        assert shmr_amd.path_stats()[0] == z0 + B
        got = np.array(buf.array)
        buf = None
    else:
        arena = torch.from_numpy(img).to(gpu)
        torch.cuda.synchronize()
        rs.encode_ptrs_dev([[arena[int(o):int(o) + L] for o in row] for row in offs])
        torch.cuda.synchronize()
        got = arena.cpu().numpy()
    assert _grids() == g0
    gained = _gained(inv)
    _assert_groups(gained, p, L, need=K_PTRS, forbid=K_SEGS | (K_NT_LOAD if form == "mapped" else 0))
    _no_flag(gained, K_SEGS)
    _same(got, want, "arena")


@pytest.mark.parametrize("k,p", [(4, 7), (10, 6)])
def test_e6_without_the_unaligned_access_mode(gpu, k, p):
    """The packed layout (shard i at i * L, L odd) under uvec=0: the realigning
    kernel (mode 3) for the full 4 KiB tiles and the byte-granular one (mode 2)
    for the rest, both with row0 = 4."""
    import torch
    B, t, L = 6, k + p, 3 * 4096 + 5
    cw = _codewords(k, p, B, L, [6, k, p])
    img = np.full(64 + B * t * L + 64, SENT, np.uint8)
    start = cw.copy()
    start[:, k:] = POISON
    img[64:64 + B * t * L] = start.reshape(-1)
    flat = torch.from_numpy(img).to(gpu)
    packed = flat[64:64 + B * t * L].view(B, t, L)
    torch.cuda.synchronize()
    inv = _inventory()
    shmr_amd.set_tuning(uvec=0)
    try:
        shmr_amd.ReedSolomon(k, p).encode_batch_dev(packed[:, :k], packed[:, k:], shard_len=L, data_shard_pitch=L,
                                                     parity_shard_pitch=L)
        torch.cuda.synchronize()
    finally:
        shmr_amd.set_tuning(uvec=-2)
    gained = _gained(inv)
    for rows in set(_row_groups(p)):
        n = _row_groups(p).count(rows)
        assert gained.get((rows, 1, 3, MODE3_FLAGS), 0) >= n and gained.get((rows, 1, 2, 0), 0) >= n, (rows, gained)
    assert not [key for key in gained if key[2] in (0, 1)], gained
    img[64:64 + B * t * L] = cw.reshape(-1)
    _same(flat.cpu().numpy(), img, "packed buffer")


# =================================== rebuild ===================================
def _run_pitch_in_place(gpu, k, p, L, present, data_only, seed):
    """reconstruct_batch_dev over a [B, t, pitch] batch in place -> the kernels
    that gained launches; bytes and sentinels checked."""
    import torch
    B, t, pitch = present.shape[0], k + p, _pitch(L)
    cw = _codewords(k, p, B, L, seed)
    work, written = _rebuilt(k, p, cw, present, data_only)
    start, want = _in_place(cw, present, work, written)
    img = np.full((B, t, pitch), SENT, np.uint8)
    img[:, :, :L] = start
    dev = torch.from_numpy(img).to(gpu)
    torch.cuda.synchronize()
    inv = _inventory()
    shmr_amd.ReedSolomon(k, p).reconstruct_batch_dev(dev, present, shard_len=L, data_only=data_only)
    torch.cuda.synchronize()
    gained = _gained(inv)
    img[:, :, :L] = want
    _same(dev.cpu().numpy(), img, "batch")
    return gained


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6), (6, 8), (3, 9)])
def test_d1_one_pattern(gpu, k, p, L, data_only):
    lost = LOST[(k, p)]
    present = _present(6, k + p, lambda b: lost)
    (m, (patterns, runs)), = _pattern_runs(present, range(6), k, data_only).items()
    assert m == (sum(1 for i in lost if i < k) if data_only else len(lost)) and (patterns, runs) == (1, 1)
    gained = _run_pitch_in_place(gpu, k, p, L, present, data_only, [11, k, p, L])
    _assert_groups(gained, m, L, forbid=K_SEGS | K_PTRS)
    _no_flag(gained, K_SEGS | K_PTRS)


def _two_patterns_40(t, a, b):
    """The layout of test_reconstruct_segments_irregular_runs: 40 blocks, the
    odd ones lose `a`, the even ones `b`, blocks b % 7 == 3 lose nothing."""
    return _present(40, t, lambda blk: [] if blk % 7 == 3 else (a if blk % 2 else b))


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", LENGTHS)
def test_d2_two_patterns_in_irregular_runs(gpu, L, data_only):
    """Two 5-erasure patterns of RS(10,6) in 7 irregular runs: one segment
    launch per row group, at rows == 4 and at rows == 1."""
    k, p = 10, 6
    present = _two_patterns_40(k + p, *FIVE[(k, p)])
    assert _pattern_runs(present, range(40), k, data_only) == {5: (2, 7)}
    gained = _run_pitch_in_place(gpu, k, p, L, present, data_only, [12, L])
    _assert_groups(gained, 5, L, need=K_SEGS, forbid=K_PTRS)
    _no_flag(gained, K_PTRS)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_d3_more_than_32_runs(gpu, k, p, data_only):
    """105 blocks: 3j and 3j + 1 lose pattern A (35 pair-runs), 3j + 2 loses
    pattern B (one strided run).  More runs than the kernel arguments hold:
    the uploaded plan table and block list, no segment kernel.  RS(10,6): A and
    B rebuild 6 rows (5 under data_only).  RS(5,5) has a single pattern with
    five data shards lost, so under data_only its B rebuilds four rows in a
    launch of its own and A's 35 runs alone overflow the segment table."""
    L = 8192 + 48
    a, b = {(5, 5): FIVE[(5, 5)], (10, 6): ([0, 2, 3, 6, 9, 11], [1, 2, 4, 7, 8, 13])}[(k, p)]
    present = _present(105, k + p, lambda blk: b if blk % 3 == 2 else a)
    groups = _pattern_runs(present, range(105), k, data_only)
    if (k, p) == (5, 5):
        assert groups == ({5: (1, 35), 4: (1, 1)} if data_only else {5: (2, 36)})
    else:
        assert groups == ({5: (2, 36)} if data_only else {6: (2, 36)})
    gained = _run_pitch_in_place(gpu, k, p, L, present, data_only, [13, k, p])
    for m in groups:
        _assert_groups(gained, m, L, forbid=K_SEGS | K_PTRS)
    _no_flag(gained, K_SEGS | K_PTRS)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("off", [0, 1])
@pytest.mark.parametrize("mixed", [False, True])
@pytest.mark.parametrize("L", SPLIT)
def test_d4_compact_output(gpu, L, mixed, off, data_only):
    """reconstruct_batch_dev_out of RS(10,6): the second row group writes
    compact rows 4 and up.  Two 5-erasure patterns (a multi-plan segment
    launch), or 5-erasure and 6-erasure blocks mixed (a 6-row output pitch;
    the 5-row blocks leave row 5 alone); output aligned (sc1 stores) or its
    base 1 byte off."""
    import torch
    k, p, B = 10, 6, 40
    t, pitch = k + p, _pitch(L)
    a, b = ([0, 2, 3, 6, 9], [1, 2, 4, 5, 7, 8]) if mixed else FIVE[(k, p)]
    present = _two_patterns_40(t, a, b)
    groups = _pattern_runs(present, range(B), k, data_only)
    assert groups == ({5: (1, 4), 6: (1, 3)} if mixed else {5: (2, 7)})
    nout = max(groups)
    cw = _codewords(k, p, B, L, [14, L, mixed])
    work, written = _rebuilt(k, p, cw, present, data_only)
    simg = np.full((B, t, pitch), SENT, np.uint8)
    simg[:, :, :L] = cw
    simg[present == 0] = POISON                 # absent slots: never read, never written
    oimg = np.full(off + B * nout * pitch + 64, SENT, np.uint8)
    dev, flat = torch.from_numpy(simg).to(gpu), torch.from_numpy(oimg).to(gpu)
    out = flat[off:off + B * nout * pitch].view(B, nout, pitch)
    torch.cuda.synchronize()
    inv = _inventory()
    shmr_amd.ReedSolomon(k, p).reconstruct_batch_dev_out(dev, present, out, shard_len=L, data_only=data_only)
    torch.cuda.synchronize()
    gained = _gained(inv)
    for m in groups:
        _assert_groups(gained, m, L, need=K_SEGS | (0 if off else K_SC1), forbid=K_PTRS | (K_SC1 if off else 0))
    _no_flag(gained, K_PTRS)
    owant = oimg[off:off + B * nout * pitch].reshape(B, nout, pitch)   # (a view: fills oimg)
    for blk in range(B):
        for j, i in enumerate(np.flatnonzero(written[blk])):            # ascending shard index
            owant[blk, j, :L] = work[blk, i]
    _same(flat.cpu().numpy(), oimg, "compact output")
    _same(dev.cpu().numpy(), simg, "input shards")


def _run_fresh_scattered(gpu, k, p, L, lost, data_only, seed):
    import torch
    B, t = 6, k + p
    present = _present(B, t, lambda b: lost)
    m = sum(1 for i in lost if i < k) if data_only else len(lost)
    cw = _codewords(k, p, B, L, seed)
    work, written = _rebuilt(k, p, cw, present, data_only)
    offs, size = _scatter(B, t, L, [k, L, 5])
    img = np.full(size, SENT, np.uint8)
    for b in range(B):
        for i in range(t):
            o = int(offs[b, i])
            img[o:o + L] = cw[b, i] if present[b, i] else POISON
    arena = torch.from_numpy(img).to(gpu)
    blocks = [[(arena[int(offs[b, i]):int(offs[b, i]) + L] if present[b, i] else None) for i in range(t)]
              for b in range(B)]
    torch.cuda.synchronize()
    g0, inv = _grids(), _inventory()
    shmr_amd.ReedSolomon(k, p).reconstruct_ptrs_dev(blocks, data_only=data_only)
    torch.cuda.synchronize()
    assert _grids() == g0
    gained = _gained(inv)
    _assert_groups(gained, m, L, need=K_PTRS, forbid=K_SEGS)
    _no_flag(gained, K_SEGS)
    for b in range(B):
        for i in range(t):
            if written[b, i]:
                assert blocks[b][i].numel() == L
                _same(blocks[b][i].cpu().numpy(), work[b, i], f"block {b} shard {i}")
            elif not present[b, i]:
                assert blocks[b][i] is None
    _same(arena.cpu().numpy(), img, "arena")


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", SPLIT)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_d5_fresh_buffers_scattered(gpu, k, p, L, data_only):
    """reconstruct_ptrs_dev with None for the lost shards of scattered blocks:
    fresh buffers, the pointer-table kernels; lost parity stays None under
    data_only."""
    _run_fresh_scattered(gpu, k, p, L, LOST[(k, p)], data_only, [15, k, p, L])


@pytest.mark.parametrize("L", BIG)
def test_wide_code_stages_its_plan_in_two_passes(gpu, L):
    """RS(33,8): a 4-row group's tables (k * 4 * 2 = 264 16-byte entries) are
    more than the 256 lanes stage in one pass, so the early-prologue kernels
    take the second staging pass (gf_tile.hpp stage_commit) -- here with
    row0 = 4 too: the encode of a pitch batch, and a rebuild of eight data
    shards into fresh buffers over pointer tables."""
    k, p = 33, 8
    _run_encode_pitch(gpu, k, p, L, [19, L])
    _run_fresh_scattered(gpu, k, p, L, [0, 3, 5, 8, 13, 21, 30, 32], False, [20, L])


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", SPLIT)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_d5_fresh_buffers_on_a_slab(gpu, k, p, L, data_only):
    """Present shards in one ShardSlab, every rebuilt shard a buffer of a
    second slab: the compact lattice (one strided run, sc1 stores); lost
    parity NULL under data_only."""
    import torch
    B, t, lost = 6, k + p, LOST[(k, p)]
    present = _present(B, t, lambda b: lost)
    m = sum(1 for i in lost if i < k) if data_only else len(lost)
    cw = _codewords(k, p, B, L, [16, k, p, L])
    work, written = _rebuilt(k, p, cw, present, data_only)
    shards, outs = shmr_amd.ShardSlab(B, t, L), shmr_amd.ShardSlab(B, m, L)
    sview, oview = shards.tensor(), outs.tensor()
    simg = np.full(tuple(sview.shape), SENT, np.uint8)
    simg[:, :, :L] = cw
    simg[present == 0] = POISON
    oimg = np.full(tuple(oview.shape), SENT, np.uint8)
    sview.copy_(torch.from_numpy(simg).to(gpu))
    oview.copy_(torch.from_numpy(oimg).to(gpu))
    addrs = shards.ptrs.reshape(B, t).copy()
    for b in range(B):
        j = 0
        for i in np.flatnonzero(present[b] == 0):
            addrs[b, i] = outs.ptrs[b * m + j] if written[b, i] else 0
            if written[b, i]:
                oimg[b, j, :L] = work[b, i]
                j += 1
    torch.cuda.synchronize()
    rs = shmr_amd.ReedSolomon(k, p)
    keep, tab = _tab(addrs)
    g0, inv = _grids(), _inventory()
    rc = rs._L.shmr_ec_reconstruct_ptrs_dev(rs._h, tab, _ptr(present), B, L, int(data_only), 0, _stream())
    assert rc == 0, shmr_amd.Error(rc).name
    torch.cuda.synchronize()
    assert _grids() == g0 + 1
    gained = _gained(inv)
    _assert_groups(gained, m, L, need=K_SC1, forbid=K_SEGS | K_PTRS)
    _no_flag(gained, K_SEGS | K_PTRS)
    _same(oview.cpu().numpy(), oimg, "output slab")
    _same(sview.cpu().numpy(), simg, "shard slab")


def _five_failed(pool_live, t, a, b=None):
    """Every live block lost `a`; with b, the blocks in odd slots lost b."""
    return _present(len(pool_live), t, lambda j: b if b is not None and pool_live[j] % 2 else a)


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", SPLIT)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_d6_pool_five_failed_disks(gpu, k, p, L, data_only):
    """Every live block of the pool with holes lost the same five shards,
    rebuilt in place on the lattice (5 segment runs); then the blocks in odd
    slots lost a second 5-erasure pattern (strided runs, two plans in one
    segment launch where both rebuild five rows)."""
    import torch
    t = k + p
    a, b = FIVE[(k, p)]
    rs = shmr_amd.ReedSolomon(k, p)
    pool = None
    for phase, second in enumerate((None, b)):
        live = [s for s in range(24) if s not in HOLES]
        present = _five_failed(live, t, a, second)
        groups = _pattern_runs(present, live, k, data_only)
        if second is None:
            assert groups == {5: (1, 5)}
        elif (k, p) == (5, 5) and data_only:       # (b loses four data shards and one parity)
            assert groups == {5: (1, 3), 4: (1, 4)}
        else:
            assert groups == {5: (2, 7)}
        pool, want = _decode_pool(gpu, k, p, L, present, data_only, [17, k, p, L, phase], pool)
        assert pool.live == live
        order = np.random.default_rng(L + phase).permutation(len(live))
        keep, tab = _tab(pool.table(order))
        pr = np.ascontiguousarray(present[order])
        g0, inv = _grids(), _inventory()
        rc = rs._L.shmr_ec_reconstruct_ptrs_dev(rs._h, tab, _ptr(pr), len(order), L, int(data_only), 0, _stream())
        assert rc == 0, shmr_amd.Error(rc).name
        torch.cuda.synchronize()
        assert _grids() == g0 + 1
        gained = _gained(inv)
        for m in groups:
            _assert_groups(gained, m, L, need=K_SEGS, forbid=K_PTRS)
        _no_flag(gained, K_PTRS)
        _same(pool.view.cpu().numpy(), pool.image(want), f"slab, phase {phase}")


@pytest.mark.parametrize("data_only", [False, True])
@pytest.mark.parametrize("L", BIG)
@pytest.mark.parametrize("k,p", [(5, 5), (10, 6)])
def test_d7_rebuild_through_the_queue(gpu, k, p, L, data_only):
    """One started shmr_ec_reconstruct_dev per live block of the pool with
    holes (five failed disks; the odd slots a second pattern), in shuffled
    order under a coalescing window: merged batches over the slots, exact."""
    t = k + p
    a, b = FIVE[(k, p)]
    live = [s for s in range(24) if s not in HOLES]
    present = _five_failed(live, t, a, b)
    pool, want = _decode_pool(gpu, k, p, L, present, data_only, [18, k, p, L])
    rs = shmr_amd.ReedSolomon(k, p)
    order = np.random.default_rng(L + 7).permutation(len(live))
    q0, g0, inv = shmr_amd.queue_stats(0), _grids(), _inventory()
    shmr_amd.set_tuning(coalesce_us=3000)
    try:
        ops = [rs.reconstruct_dev([(int(x), L) for x in pool.blocks[live[int(j)]]], present[int(j)],
                                  data_only=data_only, start=True) for j in order]
        for op in ops:
            op.wait()
    finally:
        shmr_amd.set_tuning(coalesce_us=-2)
    _queue_merged(q0, shmr_amd.queue_stats(0), len(order))
    assert _grids() > g0
    gained = _gained(inv)
    assert sum(v for (r, c, mode, f), v in gained.items() if r == 4) >= 1 and \
        sum(v for (r, c, mode, f), v in gained.items() if r == 1) >= 1, gained
    _same(pool.view.cpu().numpy(), pool.image(want), "slab")
