"""Batches that cross the table-upload chunk and ring boundaries, vs the CPU
oracle, bit-exact.

Every launch form that needs a table in device memory splits its batch on the
host, one 256 KiB slot of a 32-slot UploadRing per part (ec_core.hpp
UploadRing).  Three splitters, each with offsets, counts and slot lifetimes of
its own:

* the multi-plan rebuild tables (ec_core.cpp reconstruct_on_device: the block
  list, u32, and the plan index, u16, behind the group's plan-pointer table);
* the device shard-pointer tables (ptrs.cpp ptrs_launch: rows of t pointers,
  through the 8-entry table cache or the pointer ring);
* the same rows for mapped host slabs (host_engine.cpp run_mapped).

The rest of the suite stays below 1,100 blocks per call, so each of them runs
with one part (two at t = 255).  Here only the block count is large: shards
are tiny, the block counts are computed from the mirrored constants below, and
every case

(1) compares the whole buffer image with the oracle's (c_oracle.encode_batch
    for the codewords; a rebuild restores the codeword): shard bytes, the
    sentinel-filled pitch padding and the bytes outside the shards;
(2) proves that it crossed the boundary: the exact delta of
    device_stats(0)["launches"] (one per row group per launch set, so the sum
    over parts of their row groups -- `_rebuild_sets` mirrors the grouping and
    the split) and the launches gained by the kernel_inventory() rows of the
    kernels that serve the call, with no launch of any other kernel.

A change of the slot size, the ring or the chunk arithmetic changes the
launches count, and the case fails instead of quietly covering nothing."""
import ctypes

import numpy as np
import pytest

import shmr_amd
from shmr_amd.reed_solomon import _ptr, _u8p
from oracle import c_oracle

pytestmark = pytest.mark.gpu

# ---- the product constants under test, mirrored once ----------------------------
SLOT_BYTES = 256 * 1024     # ec_core.hpp:297  UploadRing::kSlotBytes
RING_SLOTS = 32             # ec_core.hpp:296  UploadRing::kSlots
CACHE_ENTRIES = 8           # ec_core.hpp:367  PtrTableCache::kEntries
MAX_SEGS = 32               # gf_apply.hpp:21  kern::kMaxSegs (runs that travel in the kernel arguments)
MAX_ROWS = 4                # gf_apply.hpp     kern::kMaxRowsPerLaunch


def plan_cap(patterns):
    """Blocks per part of a multi-plan rebuild (ec_core.cpp:1379-1381): the slot
    minus the 16-byte-aligned plan-pointer table and 32 bytes of alignment
    slack, over a u32 block and a u16 plan index per block."""
    table = (8 * patterns + 15) // 16 * 16
    return (SLOT_BYTES - table - 32) // (4 + 2)


def ptr_cap(t):
    """Blocks per part of a shard-pointer table (ptrs.cpp:250,
    host_engine.cpp:313): rows of t 8-byte pointers per slot."""
    return SLOT_BYTES // (8 * t)


SENT, POISON = 0xC3, 0xEE     # bytes no call may touch; the content of lost shards

# kernel template flags (gf_apply.hpp: never renumbered)
K_NT_LOAD, K_FUSE, K_PTRS, K_SEGS = 1, 1 << 18, 1 << 19, 1 << 20


# ---- oracle ---------------------------------------------------------------------
def _codewords(k, p, B, L, seed):
    """[B, k + p, L] codewords of random data, one vectorised draw."""
    rng = np.random.default_rng(seed)
    data = np.frombuffer(rng.bytes(B * k * L), np.uint8).reshape(B, k, L)
    par = np.zeros((B, p, L), np.uint8)
    c_oracle.encode_batch(k, p, data, par, B, L, 8)
    cw = np.empty((B, k + p, L), np.uint8)
    cw[:, :k] = data
    cw[:, k:] = par
    return cw


def _erasures(rng, B, t, lo, hi, weights=None):
    """present [B, t]: every block loses between lo and hi shards (weights: the
    probability of each count), count and places drawn per block (no Python
    loop over blocks)."""
    n = rng.choice(np.arange(lo, hi + 1), size=B, p=weights)
    rank = rng.random((B, t)).argsort(axis=1).argsort(axis=1)
    return np.ascontiguousarray((rank >= n[:, None]).astype(np.uint8))


def _written(present, k, data_only):
    """The shards a rebuild must write."""
    w = present == 0
    if data_only:
        w = w.copy()
        w[:, k:] = False
    return w


def _in_place(cw, present, k, data_only):
    """(start, want) shard bytes of an in-place rebuild: lost shards hold
    POISON, the written ones end as the codeword's."""
    start = cw.copy()
    start[present == 0] = POISON
    want = start.copy()
    w = _written(present, k, data_only)
    want[w] = cw[w]
    return start, want


def _same(got, want, what):
    if np.array_equal(got, want):
        return
    bad = np.argwhere(got != want)
    at = tuple(int(x) for x in bad[0])
    raise AssertionError(f"{what}: {len(bad)} bytes differ, first at {at}: {int(got[at]):#04x}, "
                         f"expected {int(want[at]):#04x}")


# ---- mirrors of the split -------------------------------------------------------
def _runs(blocks):
    """Maximal arithmetic runs of ascending block numbers, greedily from the
    left (ec_core.cpp:1296-1314)."""
    s = [int(x) for x in blocks]
    runs, i = 0, 0
    while i < len(s):
        e = i + 1
        st = s[e] - s[i] if e < len(s) else 1
        while e < len(s) and s[e] - s[e - 1] == st:
            e += 1
        runs += 1
        i = e
    return runs


def _row_groups(m):
    return [min(MAX_ROWS, m - row0) for row0 in range(0, m, MAX_ROWS)]


def _parts(B, cap):
    return [min(cap, B - b0) for b0 in range(0, B, cap)]


def _rebuild_sets(present, k, data_only, part_cap=None):
    """Mirror of reconstruct_on_device, called once per part of part_cap blocks
    (pointer tables; None: the whole batch in one call): blocks grouped by
    erasure pattern, patterns by the number of rows they rebuild; a group of P
    patterns whose blocks form more than MAX_SEGS runs goes up in parts of
    plan_cap(P) blocks, any other group is one launch set; a launch set is one
    launch per row group.  -> ({rows: launches}, [parts of every split group])."""
    present = np.asarray(present)
    B, t = present.shape
    want, split = {}, []
    for b0 in range(0, B, part_cap or B):
        pr = present[b0:b0 + (part_cap or B)]
        lost = pr == 0
        m_of = (lost[:, :k] if data_only else lost).sum(axis=1)
        m_of[lost.sum(axis=1) == 0] = 0
        for m in (int(x) for x in np.unique(m_of) if x):
            rows = np.flatnonzero(m_of == m)
            patterns, which = np.unique(pr[rows], axis=0, return_inverse=True)
            which = np.asarray(which).reshape(-1)
            P, sets = len(patterns), 1
            if len(rows) > plan_cap(P):
                runs = sum(_runs(rows[which == j]) for j in range(P))
                assert runs > MAX_SEGS, "the segment path would take this group: nothing is split"
                parts = _parts(len(rows), plan_cap(P))
                split.append(parts)
                sets = len(parts)
            for r in _row_groups(m):
                want[r] = want.get(r, 0) + sets
    return want, split


def _encode_sets(p, parts):
    return {r: _row_groups(p).count(r) * parts for r in set(_row_groups(p))}


# ---- path checks ----------------------------------------------------------------
def _launches():
    return shmr_amd.device_stats(0)["launches"]


def _inventory():
    return {(e["rows"], e["chunks"], e["mode"], e["flags"]): e["launches"] for e in shmr_amd.kernel_inventory()}


class _Path:
    """Counters before a call; check(): what the call added to them."""

    def __init__(self):
        self.launches, self.inv = _launches(), _inventory()

    def check(self, want, L, need=0, forbid=0):
        """want {rows: launches}: the launches counter rose by their sum, and
        each row count's launches went to the kernel its form and length call
        for -- the partial-tile kernel (mode 1, no flags) where the shard is
        shorter than the group's tile, else a full-tile kernel (mode 0) with
        the flags `need`, none of `forbid` and a fused tail exactly when the
        length leaves a partial tile -- and to no other kernel."""
        after = _inventory()
        gained = {key: after[key] - self.inv[key] for key in after if after[key] != self.inv[key]}
        print("launches", _launches() - self.launches, "kernels (rows, U, mode, flags):",
              {(r, c, mode, hex(f)): v for (r, c, mode, f), v in gained.items()})
        assert _launches() - self.launches == sum(want.values()), (_launches() - self.launches, want)
        served = 0
        for rows, n in want.items():
            u = 2 if rows == 4 else 1
            tile = 4096 * u
            if L < tile:
                got = gained.get((rows, 1, 1, 0), 0)
            else:
                got = sum(v for (r, c, mode, f), v in gained.items()
                          if r == rows and c == u and mode == 0 and f & need == need and not f & forbid
                          and bool(f & K_FUSE) == (L % tile != 0))
            assert got == n, (f"rows={rows}, len={L}: {got} launches of the expected kernel (need {need:#x}, "
                              f"forbid {forbid:#x}), wanted {n}; gained {gained}")
            served += got
        assert sum(gained.values()) == served, ("another kernel ran", gained, want)


def _stream():
    import torch
    return ctypes.c_void_p(torch.cuda.current_stream(0).cuda_stream)


def _pitch_image(shards, pitch):
    B, t, L = shards.shape
    img = np.full((B, t, pitch), SENT, np.uint8)
    img[:, :, :L] = shards
    return img


# ====================== A. multi-plan rebuild tables ======================
def _run_in_place(gpu, k, p, L, pitch, present, data_only, seed):
    import torch
    B = present.shape[0]
    cw = _codewords(k, p, B, L, seed)
    start, want = _in_place(cw, present, k, data_only)
    del cw
    dev = torch.from_numpy(_pitch_image(start, pitch)).to(gpu)
    del start
    torch.cuda.synchronize()
    path = _Path()
    shmr_amd.ReedSolomon(k, p).reconstruct_batch_dev(dev, present, shard_len=L, data_only=data_only)
    torch.cuda.synchronize()
    sets, split = _rebuild_sets(present, k, data_only)
    path.check(sets, L, forbid=K_SEGS | K_PTRS)
    _same(dev.cpu().numpy(), _pitch_image(want, pitch), "batch")
    return sets, split


def test_a1_block_list_in_three_parts(gpu):
    """RS(2,1), 48-byte shards at pitch 64, one random erasure per block, in
    place: three patterns of one row each share one multi-plan group, whose
    block list and plan index go up in parts of cap, cap and 1 blocks: a last
    part of one block (an odd count in front of its plan index), and two parts
    whose lists start cap and 2 * cap blocks into the group.  The partial-tile
    kernel serves all three."""
    k, p, L = 2, 1, 48
    cap = plan_cap(3)
    B = 2 * cap + 1
    present = _erasures(np.random.default_rng(0xA1), B, k + p, 1, 1)
    sets, split = _run_in_place(gpu, k, p, L, 64, present, False, [0xA1, 1])
    assert split == [[cap, cap, 1]] and sets == {1: 3}


def test_a2_block_list_under_the_full_tile_kernel(gpu):
    """The same code at 4096 + 48 bytes (pitch 4160), cap + 1 blocks: the
    full-tile table kernel with a fused tail reads a block list that came up in
    two parts."""
    k, p, L = 2, 1, 4096 + 48
    cap = plan_cap(3)
    B = cap + 1
    present = _erasures(np.random.default_rng(0xA2), B, k + p, 1, 1)
    sets, split = _run_in_place(gpu, k, p, L, 4160, present, False, [0xA2, 1])
    assert split == [[cap, 1]] and sets == {1: 2}


def test_a3_compact_output_across_the_part_boundary(gpu):
    """reconstruct_batch_dev_out, RS(2,1), cap + 1 blocks: block b's rebuilt
    shard lands in output row b on both sides of the part boundary, no other
    output byte changes, and the input (absent slots poisoned) is not
    written."""
    import torch
    k, p, L, pitch = 2, 1, 48, 64
    cap = plan_cap(3)
    B = cap + 1
    present = _erasures(np.random.default_rng(0xA3), B, k + p, 1, 1)
    cw = _codewords(k, p, B, L, [0xA3, 1])
    start = cw.copy()
    start[present == 0] = POISON
    simg = _pitch_image(start, pitch)
    oimg = np.full((B, 1, pitch), SENT, np.uint8)
    dev, out = torch.from_numpy(simg).to(gpu), torch.from_numpy(oimg).to(gpu)
    torch.cuda.synchronize()
    path = _Path()
    shmr_amd.ReedSolomon(k, p).reconstruct_batch_dev_out(dev, present, out, shard_len=L)
    torch.cuda.synchronize()
    sets, split = _rebuild_sets(present, k, False)
    assert split == [[cap, 1]] and sets == {1: 2}
    path.check(sets, L, forbid=K_SEGS | K_PTRS)
    oimg[:, 0, :L] = cw[present == 0]          # one lost shard per block, in block order
    _same(out.cpu().numpy(), oimg, "compact output")
    _same(dev.cpu().numpy(), simg, "input shards")


@pytest.mark.parametrize("data_only", [False, True])
def test_a4_two_row_counts_split_on_their_own(gpu, data_only):
    """RS(4,2), 100,000 blocks that lose 0 (4 %), 1 (48 %) or 2 (48 %) random
    shards, so that either count has more blocks than one part holds: the
    one-row group (6 patterns) and the two-row group (15 patterns) are each
    split by their own part size, and whole blocks are skipped.  Under
    data_only a block that lost only parity contributes nothing and one that
    lost a data and a parity shard moves to the one-row group (12 patterns,
    still split); the two-row group (both data, 6 patterns) then fits one
    part."""
    k, p, L, B = 4, 2, 48, 100000
    present = _erasures(np.random.default_rng(0xA4), B, k + p, 0, 2, [0.04, 0.48, 0.48])
    lost = present == 0
    m_of = (lost[:, :k] if data_only else lost).sum(axis=1)
    n1, n2 = int((m_of == 1).sum()), int((m_of == 2).sum())
    p1 = len(np.unique(present[m_of == 1], axis=0))
    p2 = len(np.unique(present[m_of == 2], axis=0))
    assert (p1, p2) == ((12, 6) if data_only else (6, 15))
    assert n1 > plan_cap(p1) and (data_only or n2 > plan_cap(p2))
    sets, split = _run_in_place(gpu, k, p, L, 64, present, data_only, [0xA4, 1])
    assert sets == {1: -(-n1 // plan_cap(p1)), 2: -(-n2 // plan_cap(p2))}
    assert sorted(split) == sorted(_parts(n, plan_cap(P)) for n, P in ((n1, p1), (n2, p2)) if n > plan_cap(P))


# ====================== B. device shard-pointer tables ======================
def _arena(gpu, shards, slot):
    """[B, t, slot] arena on the device holding `shards`, SENT elsewhere ->
    (tensor, host image, address table [B, t])."""
    import torch
    img = _pitch_image(shards, slot)
    dev = torch.from_numpy(img).to(gpu)
    B, t, _ = img.shape
    addr = np.uint64(dev.data_ptr()) + np.arange(B * t, dtype=np.uint64).reshape(B, t) * np.uint64(slot)
    return dev, img, np.ascontiguousarray(addr)


def _tab(addr):
    return addr.ctypes.data_as(ctypes.POINTER(_u8p))


def _ptrs_pair(gpu, k, p, L, slot, B, present, seed):
    """shmr_ec_encode_ptrs_dev, then shmr_ec_reconstruct_ptrs_dev in place,
    over one arena of B * t slots; each call's image and path checked."""
    import torch
    t = k + p
    cap = ptr_cap(t)
    parts = _parts(B, cap)
    cw = _codewords(k, p, B, L, seed)
    start = cw.copy()
    start[:, k:] = POISON
    dev, img, addr = _arena(gpu, start, slot)
    rs = shmr_amd.ReedSolomon(k, p)
    torch.cuda.synchronize()
    path = _Path()
    rc = rs._L.shmr_ec_encode_ptrs_dev(rs._h, _tab(addr), B, L, 0, _stream())
    assert rc == 0, shmr_amd.Error(rc).name
    torch.cuda.synchronize()
    path.check(_encode_sets(p, len(parts)), L, need=K_PTRS, forbid=K_SEGS)
    img[:, :, :L] = cw
    _same(dev.cpu().numpy(), img, "arena after the encode")
    start, want = _in_place(cw, present, k, False)
    dev.copy_(torch.from_numpy(_pitch_image(start, slot)))
    torch.cuda.synchronize()
    path = _Path()
    rc = rs._L.shmr_ec_reconstruct_ptrs_dev(rs._h, _tab(addr), _ptr(present), B, L, 0, 0, _stream())
    assert rc == 0, shmr_amd.Error(rc).name
    torch.cuda.synchronize()
    sets, split = _rebuild_sets(present, k, False, cap)
    assert not split      # (a part of a pointer table is far below the plan tables' part size)
    path.check(sets, L, need=K_PTRS)
    _same(dev.cpu().numpy(), _pitch_image(want, slot), "arena after the rebuild")
    return parts, sets


def test_b5_pointer_rows_in_two_parts(gpu, table_kernels):
    """RS(8,3), 4096 + 48 bytes in 4160-byte slots of one arena, one block more
    than a slot holds rows of 11 pointers: parts of cap and 1 blocks under the
    full-tile pointer-table kernels; encode, then 1 to 3 random erasures."""
    k, p, L = 8, 3, 4096 + 48
    cap = ptr_cap(k + p)
    B = cap + 1
    present = _erasures(np.random.default_rng(0xB5), B, k + p, 1, 3)
    parts, sets = _ptrs_pair(gpu, k, p, L, 4160, B, present, [0xB5, 1])
    assert parts == [cap, 1]
    m_last = int((present[-1] == 0).sum())
    first = {int(m) for m in np.unique((present[:cap] == 0).sum(axis=1))}
    assert first == {1, 2, 3} and sum(sets.values()) == 3 + 1 and sets[m_last] == 2


def test_b6_two_row_groups_per_part(gpu, table_kernels):
    """RS(6,5), 48-byte shards, cap + 1 blocks: every part walks two row groups
    (4 + 1), in the encode and in a rebuild of five random shards per block:
    2 parts x 2 launches each."""
    k, p, L = 6, 5, 48
    cap = ptr_cap(k + p)
    B = cap + 1
    present = _erasures(np.random.default_rng(0xB6), B, k + p, 5, 5)
    parts, sets = _ptrs_pair(gpu, k, p, L, 64, B, present, [0xB6, 1])
    assert parts == [cap, 1] and sets == {4: 2, 1: 2} and _encode_sets(p, 2) == {4: 2, 1: 2}


WIDE = (251, 4)            # t = 255, the crate's maximum: the fewest rows per slot


def _wide_erasures(rng, B):
    """1 to 4 random erasures per block of RS(251,4), every block's pattern
    drawn from 64 random ones: each distinct pattern costs the host a
    251 x 251 inversion and the process a permanent plan image, neither of
    which is under test here (the two wide cases share the 64)."""
    pool = _erasures(np.random.default_rng(0x251), 64, sum(WIDE), 1, 4)
    return np.ascontiguousarray(pool[rng.integers(0, len(pool), B)])


def test_b7_ring_wrap_and_cache_cycling(gpu, table_kernels):
    """RS(251,4): 128 rows per slot, (RING_SLOTS + 1) * 128 + 1 blocks = 34
    parts, more than the ring's slots and the table cache's entries, in 64-byte
    slots.  Encode and rebuild, twice, with no synchronise between the four
    calls (lost shards are poisoned and the arena is snapshotted by device work
    in stream order): a slot or cache entry reused too early has a reader in
    flight.  Nothing is asserted about blocking_calls or ptr_table_hits:
    whether a slot's event is ready yet depends on timing."""
    import torch
    (k, p), L, slot = WIDE, 48, 64
    t = k + p
    cap = ptr_cap(t)
    B = (RING_SLOTS + 1) * cap + 1
    parts = _parts(B, cap)
    assert len(parts) > RING_SLOTS > CACHE_ENTRIES and parts[-1] == 1
    rng = np.random.default_rng(0xB7)
    cw = _codewords(k, p, B, L, [0xB7, 1])
    start = cw.copy()
    start[:, k:] = POISON
    dev, img, addr = _arena(gpu, start, slot)
    presents = [_wide_erasures(rng, B) for _ in range(2)]
    assert not np.array_equal(*presents)
    masks = [torch.from_numpy(pr == 0).to(gpu)[:, :, None] for pr in presents]
    snaps = [torch.empty_like(dev) for _ in range(4)]
    rs = shmr_amd.ReedSolomon(k, p)
    stream = _stream()
    torch.cuda.synchronize()
    path = _Path()
    for rep in range(2):
        dev[:, k:, :L].fill_(POISON)
        rc = rs._L.shmr_ec_encode_ptrs_dev(rs._h, _tab(addr), B, L, 0, stream)
        assert rc == 0, shmr_amd.Error(rc).name
        snaps[2 * rep].copy_(dev)
        dev[:, :, :L].masked_fill_(masks[rep], POISON)
        rc = rs._L.shmr_ec_reconstruct_ptrs_dev(rs._h, _tab(addr), _ptr(presents[rep]), B, L, 0, 0, stream)
        assert rc == 0, shmr_amd.Error(rc).name
        snaps[2 * rep + 1].copy_(dev)
    torch.cuda.synchronize()
    sets = _encode_sets(p, 2 * len(parts))
    for pr in presents:
        more, split = _rebuild_sets(pr, k, False, cap)
        assert not split
        for rows, n in more.items():
            sets[rows] = sets.get(rows, 0) + n
    assert sum(sets.values()) >= 4 * len(parts)
    path.check(sets, L)
    img[:, :, :L] = cw
    for j, snap in enumerate(snaps):
        _same(snap.cpu().numpy(), img, f"arena after call {j} (encode, rebuild, encode, rebuild)")


# ====================== C. mapped host slabs, zero-copy ======================
GUARD = 64


def _mapped_pair(k, p, L, B, present):
    """encode_blocks_host, then reconstruct_blocks_host, over a PinnedBuffer
    viewed as [B, t, L] between two guards; the whole buffer, the path_stats()
    delta and the launches of each call checked."""
    t = k + p
    cap = ptr_cap(t)
    parts = _parts(B, cap)
    cw = _codewords(k, p, B, L, [k, p, L, B])
    buf = shmr_amd.PinnedBuffer(GUARD + B * t * L + GUARD)
    body = slice(GUARD, GUARD + B * t * L)
    blocks = buf.array[body].reshape(B, t, L)
    img = np.full(buf.nbytes, SENT, np.uint8)
    shards = img[body].reshape(B, t, L)            # (a view: fills img)
    rs = shmr_amd.ReedSolomon(k, p)

    def call(fn, start, want, sets, what):
        shards[:] = start
        buf.array[:] = img
        z0, s0 = shmr_amd.path_stats()
        path = _Path()
        fn()
        z1, s1 = shmr_amd.path_stats()
        assert (z1 - z0, s1 - s0) == (B, 0)
        path.check(sets, L, need=K_PTRS, forbid=K_SEGS | K_NT_LOAD)
        shards[:] = want
        _same(np.array(buf.array), img, what)

    start = cw.copy()
    start[:, k:] = POISON
    call(lambda: rs.encode_blocks_host(blocks, devices=[0]), start, cw, _encode_sets(p, len(parts)),
         "slab after the encode")
    start, want = _in_place(cw, present, k, False)
    sets, split = _rebuild_sets(present, k, False, cap)
    assert not split
    call(lambda: rs.reconstruct_blocks_host(blocks, present, devices=[0]), start, want, sets,
         "slab after the rebuild")
    buf = None
    return parts, sets


@pytest.mark.parametrize("direct", [0, 1 << 20])
@pytest.mark.parametrize("L", [64, 4096 + 16])
def test_c8_mapped_rows_in_two_parts(gpu, L, direct):
    """RS(8,3) over a mapped slab, one block more than a slot holds rows: the
    table read in place from the pinned slot (ptrs_direct large) and uploaded
    first (0) both cross a part boundary; encode, then up to 3 random erasures
    per block (some blocks whole)."""
    k, p = 8, 3
    cap = ptr_cap(k + p)
    B = cap + 1
    present = _erasures(np.random.default_rng([0xC8, L]), B, k + p, 0, 3)
    present[-1] = 1
    present[-1, [1, k]] = 0                       # the one-block part has work
    try:
        shmr_amd.set_tuning(ptrs_direct=direct)
        parts, sets = _mapped_pair(k, p, L, B, present)
    finally:
        shmr_amd.set_tuning(ptrs_direct=-2)
    assert parts == [cap, 1] and sum(sets.values()) == 3 + 1


def test_c9_ring_wrap_on_the_mapped_path(gpu):
    """RS(251,4), 16-byte shards on a mapped slab, 34 parts: the pointer ring
    wraps inside one encode and inside one rebuild."""
    (k, p), L = WIDE, 16
    cap = ptr_cap(k + p)
    B = (RING_SLOTS + 1) * cap + 1
    present = _wide_erasures(np.random.default_rng(0xC9), B)
    parts, sets = _mapped_pair(k, p, L, B, present)
    assert len(parts) > RING_SLOTS and parts[-1] == 1 and sum(sets.values()) >= len(parts)
