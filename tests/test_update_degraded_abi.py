"""CPU tests of the degraded update entry points of the C ABI
(include/shmr_ec.h): shmr_ec_update_degraded_batch_dev and
shmr_ec_update_degraded_plan.  Both are exported by both library flavours and
declared in _native.py; the batch call checks its arguments, the update list
and the presence flags included, before any device work.  No kernel is launched
here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY, TOO_FEW_PRESENT = 0, -100, -101, -11, -10
NAMES = {"shmr_ec_update_degraded_batch_dev", "shmr_ec_update_degraded_plan"}
M64 = (1 << 64) - 1
K, P = 4, 2
T = K + P
TABLE_CHUNK = 256 * 1024 // 48                       # 48-byte entries, one 256 KiB ring slot

ALL = [[1] * T] * 3
DEGRADED = [[1] * T, [0, 1, 1, 0, 1, 1], [1, 1, 0, 1, 1, 0]]
TOO_FEW = [[1] * T, [0, 0, 0, 1, 1, 1], [1] * T]      # block 1: 3 of 4 present


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _updates(rows):
    arr = (_native.Update * max(len(rows), 1))()
    for i, row in enumerate(rows):
        arr[i] = _native.Update(*row)
    return arr


def _present(rows):
    return np.ascontiguousarray(rows, dtype=np.uint8)


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_symbols_exported_and_declared(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (shmr_ec_\w+)", out))
    lib = _native._load(flavour)
    declared = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name) and name in declared
    assert len(declared["shmr_ec_update_degraded_batch_dev"][1]) == 13
    assert len(declared["shmr_ec_update_degraded_plan"][1]) == 12
    header = re.sub(r"\s+", " ", open(_native._HERE + "/../include/shmr_ec.h").read())
    section = header[header.index("parity delta update of degraded device-resident blocks"):
                     header.index("shmr_ec_update_degraded_plan(")]
    assert "MUST NOT overlap" in section                     # the caller's contract on d_src
    assert "NOT capturable" in section
    assert "damaged survivor" in section.lower()
    assert "shmr_ec_reconstruct_checked_batch_dev" in section and "shmr_ec_locate_checked_batch_dev" in section


def test_kernel_is_outside_the_inventory():
    """gf_update_degraded_kernel is its own __global__ function in the product
    library, beside gf_update_kernel; the inventory stays what encode and
    reconstruct dispatch, and no counter or status was added."""
    data = open(_native._PATHS["product"], "rb").read()
    assert b"gf_update_degraded_kernel" in data and b"gf_update_kernel" in data
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv
    assert len(shmr_amd.device_stats(0)) == 12


def _update(L, h, rows=((0, 0, 0, 8, 0),), d=0x100000, present=ALL, nblocks=3, shard_len=64, src=0x300000,
            src_bytes=4096, device=0, updates="rows", nupdates=None):
    v = ctypes.c_void_p
    arr = _updates(rows) if updates == "rows" else updates
    n = len(rows) if nupdates is None else nupdates
    pr = _present(present) if present is not None else None
    return L.shmr_ec_update_degraded_batch_dev(
        h, v(d), 64, 512, pr.ctypes.data_as(_native._u8p) if pr is not None else None, nblocks, shard_len,
        ctypes.cast(arr, v) if arr is not None else None, n, v(src), src_bytes, device, None)


def _plan(L, h, rows=((0, 0, 0, 8, 0),), present=ALL, nblocks=3, shard_len=64, src_bytes=4096, updates="rows",
          nupdates=None, outs=True):
    arr = _updates(rows) if updates == "rows" else updates
    n = len(rows) if nupdates is None else nupdates
    pr = _present(present) if present is not None else None
    round_of = (ctypes.c_uint32 * max(n, 1))(*([0xdead] * max(n, 1)))
    rebuilt = (ctypes.c_uint8 * max(n, 1))(*([0xee] * max(n, 1)))
    nrounds, npieces, nchunks = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xdead), ctypes.c_uint32(0xdead)
    rc = L.shmr_ec_update_degraded_plan(
        h, pr.ctypes.data_as(_native._u8p) if pr is not None else None, nblocks, shard_len,
        ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, n, src_bytes,
        round_of if outs else None, ctypes.byref(nrounds) if outs else None, rebuilt if outs else None,
        ctypes.byref(npieces) if outs else None, ctypes.byref(nchunks) if outs else None)
    return rc, list(round_of)[:n], nrounds.value, list(rebuilt)[:n], npieces.value, nchunks.value


BAD_ROWS = [(3, 0, 0, 8, 0),                # block >= nblocks
            (0, K, 0, 8, 0),                # shard >= data (a parity shard cannot be written)
            (0, T - 1, 0, 8, 0),
            (0, 0, 0, 0, 0),                # len == 0
            (0, 0, 57, 8, 0),               # offset + len > shard_len
            (0, 0, M64, 2, 0),              # ... past 2^64
            (0, 0, 2, M64, 0),
            (0, 0, 0, 8, 4089),             # src_offset + len > src_bytes
            (0, 0, 0, 8, M64 - 3)]          # ... past 2^64
# two writes to one byte of a shard (the second list: only after a sort by shard)
INTERSECTING = [((0, 0, 0, 8, 0), (0, 0, 7, 8, 8)),
                ((0, 0, 0, 64, 0), (0, 1, 0, 64, 0), (0, 0, 63, 1, 0))]
FINE = ((0, 0, 0, 8, 0), (0, 0, 8, 8, 8), (0, 1, 0, 64, 100), (2, 3, 63, 1, 4095))


def test_update_degraded_batch_dev_argument_order():
    """NULL rs -> InvalidArgument; no updates or no blocks -> Ok; shard_len == 0
    -> EmptyShard; a NULL pointer (present included), a bad update, two
    intersecting updates of one (block, shard) -> InvalidArgument; a block with
    fewer than k present, updated or not -> TooFewShardsPresent; the device ID
    last.  Every failure is combined with every later one.  The fake device
    addresses are never dereferenced."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    bad_row, cross = (BAD_ROWS[0],), INTERSECTING[0]
    # 1. NULL rs, with every later failure
    assert _update(L, None) == INVALID
    assert _update(L, None, nupdates=0) == INVALID
    assert _update(L, None, nblocks=0) == INVALID
    assert _update(L, None, shard_len=0, d=None, present=TOO_FEW, rows=bad_row, device=-5) == INVALID
    # 2. nothing to do: Ok whatever else is wrong
    assert _update(L, h, nupdates=0, updates=None, d=None, src=None, present=None, shard_len=0, device=-5) == OK
    assert _update(L, h, nblocks=0, d=None, src=None, present=None, shard_len=0, device=-5) == OK
    assert _update(L, h, rows=((7, 9, 0, 0, 0),), nblocks=0) == OK
    assert _update(L, h, nupdates=0, present=TOO_FEW, device=-5) == OK
    # 3. shard_len == 0, with every later failure
    assert _update(L, h, shard_len=0) == EMPTY
    for later in (dict(d=None), dict(present=None), dict(updates=None, nupdates=1), dict(rows=bad_row),
                  dict(rows=cross), dict(present=TOO_FEW), dict(device=-5)):
        assert _update(L, h, shard_len=0, **later) == EMPTY, later
    assert _update(L, h, shard_len=0, d=None, present=TOO_FEW, rows=bad_row, device=-5) == EMPTY
    # 4. a NULL pointer, with every later failure
    nulls = [dict(d=None), dict(src=None), dict(present=None), dict(updates=None, nupdates=1)]
    for null in nulls:
        assert _update(L, h, device=-5, **null) == INVALID, null
        for later in (dict(rows=bad_row), dict(rows=cross), dict(device=-5)):
            if "updates" in null and "rows" in later:
                continue
            assert _update(L, h, **{**later, **null}) == INVALID, (null, later)
        if "present" not in null:
            assert _update(L, h, present=TOO_FEW, device=-5, **null) == INVALID, null
    # 5. a bad update and intersecting updates come before the flags and the device
    for row in BAD_ROWS:
        assert _update(L, h, rows=(row,), device=-5) == INVALID, row
        assert _update(L, h, rows=((1, 1, 0, 8, 0), row), device=-5) == INVALID, row
        assert _update(L, h, rows=(row,), present=TOO_FEW, device=-5) == INVALID, row
    for rows in INTERSECTING:
        assert _update(L, h, rows=rows, device=-5) == INVALID
        assert _update(L, h, rows=rows, present=DEGRADED, device=-5) == INVALID
        assert _update(L, h, rows=rows, present=TOO_FEW, device=-5) == INVALID
    # 6. every block's flags are checked, updated or not, before the device
    assert _update(L, h, rows=FINE, present=TOO_FEW, device=-5) == TOO_FEW_PRESENT       # block 1: no update
    assert _update(L, h, rows=((0, 0, 0, 8, 0),), present=TOO_FEW, device=-5) == TOO_FEW_PRESENT
    assert _update(L, h, rows=((1, 0, 0, 8, 0),), present=TOO_FEW, device=9999) == TOO_FEW_PRESENT
    # 7. the device ID comes last; well formed lists reach it
    for present in (ALL, DEGRADED):
        for device in (-1, 9999):
            assert _update(L, h, rows=FINE, present=present, device=device) == (NO_DEVICE if _no_gpu() else INVALID)


def test_well_formed_call_without_a_gpu_is_no_device():
    """No CPU fallback, and a refused call counts nothing.  (With a GPU the
    well-formed call would run on the fake addresses: only the refusal is made.)"""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    before = shmr_amd.device_stats(0)
    if _no_gpu():
        assert _update(L, rs._h, rows=((0, 0, 0, 8, 0), (1, 0, 13, 40, 8)), present=DEGRADED) == NO_DEVICE
    assert _update(L, rs._h, rows=((0, 0, 0, 8, 0), (0, 0, 0, 8, 0))) == INVALID
    assert shmr_amd.device_stats(0) == before


def test_plan_refusals_in_order():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    bad_row, cross = (BAD_ROWS[0],), INTERSECTING[0]
    assert _plan(L, None)[0] == INVALID
    assert _plan(L, None, nblocks=0, shard_len=0, present=None)[0] == INVALID
    assert _plan(L, h, rows=()) == (OK, [], 0, [], 0, 0)
    assert _plan(L, h, nblocks=0, present=None, shard_len=0)[::2] == (OK, 0, 0)
    assert _plan(L, h, shard_len=0, present=TOO_FEW)[0] == EMPTY
    assert _plan(L, h, shard_len=0, present=None, rows=bad_row)[0] == EMPTY
    assert _plan(L, h, present=None)[0] == INVALID
    assert _plan(L, h, updates=None, nupdates=1)[0] == INVALID
    assert _plan(L, h, updates=None, nupdates=1, present=TOO_FEW)[0] == INVALID
    for row in BAD_ROWS:
        assert _plan(L, h, rows=(row,))[0] == INVALID, row
        assert _plan(L, h, rows=(row,), present=TOO_FEW)[0] == INVALID, row
    assert _plan(L, h, rows=cross, present=TOO_FEW)[0] == INVALID
    assert _plan(L, h, rows=FINE, present=TOO_FEW)[0] == TOO_FEW_PRESENT
    assert _plan(L, h, rows=FINE)[0] == OK
    # any out pointer may be NULL: the checks are the same
    assert _plan(L, h, rows=FINE, outs=False)[0] == OK
    assert _plan(L, h, rows=cross, outs=False)[0] == INVALID
    assert _plan(L, h, rows=FINE, present=TOO_FEW, outs=False)[0] == TOO_FEW_PRESENT
    n = ctypes.c_uint32(7)
    pr = _present(DEGRADED)
    arr = _updates(FINE)
    assert L.shmr_ec_update_degraded_plan(h, pr.ctypes.data_as(_native._u8p), 3, 64, ctypes.cast(arr, ctypes.c_void_p),
                                          len(FINE), 4096, None, None, None, None, ctypes.byref(n)) == OK
    assert n.value == 1


def test_plan_rounds_rebuilt_pieces_and_chunks():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    # rounds: what update_rounds says of the same list
    lists = [
        [(b, s, 0, 16, 16 * (b * K + s)) for b in range(3) for s in range(K)],                 # K rounds in every block
        [(0, 0, 0, 40, 0), (0, 1, 40, 24, 40), (1, 0, 5, 4, 64), (1, 3, 9, 14, 68)],          # disjoint: one round
        [(1, 0, 0, 30, 0), (1, 1, 20, 30, 30), (1, 3, 40, 24, 60), (2, 2, 0, 64, 100)],       # a chain: 2 rounds
    ]
    for rows in lists:
        rc, round_of, nrounds, rebuilt, npieces, nchunks = _plan(L, h, rows=rows, present=DEGRADED)
        want_rounds, want_n = rs.update_rounds(rows, 3, 64, 4096)
        assert rc == OK and round_of == want_rounds.tolist() and nrounds == want_n
        # DEGRADED: block 0 whole; block 1 lost data 0 and 3; block 2 lost data 2 and parity 5
        assert rebuilt == [0 if DEGRADED[b][s] else 1 for b, s, *_ in rows]
        assert nchunks == 1
    assert _plan(L, h, rows=lists[0], present=DEGRADED)[2:5:2] == (K, 12)
    assert sum(_plan(L, h, rows=lists[0], present=DEGRADED)[3]) == 3
    # any non-zero flag is "present", as for the reconstruct
    odd = [[1] * T, [0, 7, 255, 0, 1, 2], [1] * T]
    assert _plan(L, h, rows=lists[0], present=odd)[3][4:8] == [1, 0, 0, 1]
    # pieces: head, whole chunks, tail
    assert _plan(L, h, rows=[(1, 0, 0, 64, 0)], present=DEGRADED)[4] == 1
    assert _plan(L, h, rows=[(1, 0, 1, 63, 0)], present=DEGRADED)[4] == 2
    assert _plan(L, h, rows=[(1, 0, 1, 62, 0)], present=DEGRADED)[4] == 3
    assert _plan(L, h, rows=[(0, 0, 3, 9, 0)], present=DEGRADED)[4] == 1
    assert _plan(L, h, rows=[(0, 0, 10, 9, 0)], present=DEGRADED)[4] == 2
    # a head + vector + tail request beside a whole-chunk one
    assert _plan(L, h, rows=[(1, 0, 1, 62, 0), (1, 1, 0, 64, 64)], present=DEGRADED)[2:5:2] == (2, 4)
    # chunks: one ring slot (256 KiB) of 48-byte entries each
    many = [(i % 3, (i // 3) % K, i // (3 * K), 1, i) for i in range(TABLE_CHUNK + 1)]
    rc, _, nrounds, _, npieces, nchunks = _plan(L, h, rows=many[:TABLE_CHUNK], present=DEGRADED, shard_len=5000,
                                                src_bytes=1 << 30)
    assert (rc, nrounds, npieces, nchunks) == (OK, K, TABLE_CHUNK, 1)
    rc, _, nrounds, _, npieces, nchunks = _plan(L, h, rows=many, present=DEGRADED, shard_len=5000, src_bytes=1 << 30)
    assert (rc, nrounds, npieces, nchunks) == (OK, K, TABLE_CHUNK + 1, 2)


def _brute_split(block, pos, length, shard_len, src_offset):
    """Byte by byte: runs of consecutive payload bytes within one shard."""
    out = []
    for i in range(length):
        shard, off = (pos + i) // shard_len, (pos + i) % shard_len
        if out and out[-1][1] == shard and out[-1][2] + out[-1][3] == off:
            out[-1][3] += 1
        else:
            out.append([block, shard, off, 1, src_offset + i])
    return [tuple(r) for r in out]


def test_block_range_writes():
    f = shmr_amd.ReedSolomon.block_range_writes
    S = 37
    assert f(5, 0, 0, S) == []
    assert f(5, 10, 20, S) == [(5, 0, 10, 20, 0)]
    assert f(5, 10, 20, S, src_offset=7) == [(5, 0, 10, 20, 7)]
    rng = np.random.default_rng(4)
    cases = [(0, 0, K * S, 0), (1, S - 1, 2, 3), (2, S, S, 0), (3, 2 * S - 5, S + 10, 11), (0, K * S - 1, 1, 0)]
    cases += [(int(rng.integers(0, 9)), int(pos), int(rng.integers(1, K * S - pos + 1)), int(rng.integers(0, 50)))
              for pos in rng.integers(0, K * S, 40)]
    for block, pos, length, so in cases:
        rows = f(block, pos, length, S, so)
        assert rows == _brute_split(block, pos, length, S, so), (block, pos, length, so)
        assert sum(r[3] for r in rows) == length and all(a[4] + a[3] == b[4] for a, b in zip(rows, rows[1:]))
    # the read-side twin splits the same way
    assert f(9, 12345, 54321, 4117, 5) == shmr_amd.ReedSolomon.block_range_reads(9, 12345, 54321, 4117, 5)
    # past the payload the shard index says so: the update calls refuse shard >= data
    rs = shmr_amd.ReedSolomon(K, P)
    over = f(0, K * S - 1, 2, S)
    assert over[-1] == (0, K, 0, 1, 1)
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_degraded_plan(np.ones((1, T), np.uint8), over, S, 16)
    assert e.value.name == "InvalidArgument"
    assert rs.update_degraded_plan(np.ones((1, T), np.uint8), f(0, 0, K * S, S), S, K * S)[3] >= K
    for bad in [(-1, 0, 1, S), (0, -1, 1, S), (0, 0, -1, S), (0, 0, 1, 0), (0, 0, 1, S, -1)]:
        with pytest.raises(ValueError):
            f(*bad)


def test_python_plan_and_list_conversion():
    rs = shmr_amd.ReedSolomon(K, P)
    present = np.array(DEGRADED, dtype=bool)
    rows = [(1, 0, 0, 64, 0), (1, 1, 0, 64, 64), (2, 2, 5, 20, 128)]
    round_of, nrounds, rebuilt, npieces, nchunks = rs.update_degraded_plan(present, rows, 64, 256)
    assert round_of.dtype == np.uint32 and sorted(round_of[:2].tolist()) == [0, 1] and round_of[2] == 0 and nrounds == 2
    assert rebuilt.dtype == np.uint8 and rebuilt.tolist() == [1, 0, 1] and (npieces, nchunks) == (1 + 1 + 2, 1)
    # an (n, 5) integer array is the same list
    assert rs.update_degraded_plan(present, np.array(rows, dtype=np.int64), 64, 256)[3] == 4
    assert rs.update_degraded_plan(present, [], 64, 256)[1::2] == (0, 0)
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_degraded_plan(present, [(0, 0, 0, 65, 0)], 64, 256)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_degraded_plan(np.array(TOO_FEW), rows, 64, 256)
    assert e.value.name == "TooFewShardsPresent"
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_degraded_plan(present, [(0, 0, -1, 8, 0)], 64, 256)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(TypeError):
        rs.update_degraded_plan(present, [(0, 0, 0, 8)], 64, 256)
    with pytest.raises(TypeError):
        rs.update_degraded_plan(present, np.zeros((2, 5), dtype=np.float32), 64, 256)
    with pytest.raises(ValueError):
        rs.update_degraded_plan(np.ones(T + 1, np.uint8), rows, 64, 256)


def test_python_checks_precede_device_use():
    """update_degraded_batch_dev applies read_batch_dev's tensor checks in its
    order, then requires src to be a 1-D uint8 tensor on the same device."""
    import torch
    rs = shmr_amd.ReedSolomon(K, P)
    shards = torch.zeros((3, T, 1024), dtype=torch.uint8)
    present = np.ones((3, T), dtype=np.uint8)
    src = torch.zeros(64, dtype=torch.uint8)
    ups = [(0, 0, 0, 8, 0)]
    fn = rs.update_degraded_batch_dev
    with pytest.raises(TypeError):
        fn(shards.float(), present, ups, src)
    with pytest.raises(TypeError):
        fn(shards.reshape(3, -1), present, ups, src)
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards[:, :5], present, ups, src)
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards, present, ups, src, shard_len=1025)
    assert e.value.name == "IncorrectShardSize"
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards, present, ups, src, shard_len=0)
    assert e.value.name == "EmptyShard"
    with pytest.raises(ValueError):
        fn(shards, present[:2], ups, src)
    with pytest.raises(TypeError):                               # well formed, but pageable host memory
        fn(shards, present, ups, src, shard_len=1000)
