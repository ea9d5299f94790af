"""CPU tests of the ranged read entry points of the C ABI (include/shmr_ec.h):
shmr_ec_read_batch_dev and shmr_ec_read_plan.  Both are exported by both
library flavours and declared in _native.py; the batch call checks its
arguments, the read list and the presence flags included, before any device
work.  No kernel is launched here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY, TOO_FEW_PRESENT = 0, -100, -101, -11, -10
NAMES = {"shmr_ec_read_batch_dev", "shmr_ec_read_plan"}
M64 = (1 << 64) - 1
K, P = 4, 2
T = K + P


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _reads(rows):
    arr = (_native.Read * max(len(rows), 1))()
    for i, row in enumerate(rows):
        arr[i] = _native.Read(*row)
    return arr


def _present(rows):
    return np.ascontiguousarray(rows, dtype=np.uint8)


ALL = [[1] * T] * 3
DEGRADED = [[1] * T, [0, 1, 1, 0, 1, 1], [1, 1, 0, 1, 1, 0]]


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_symbols_exported_and_declared(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (shmr_ec_\w+)", out))
    lib = _native._load(flavour)
    declared = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name) and name in declared
    assert len(declared["shmr_ec_read_batch_dev"][1]) == 13 and len(declared["shmr_ec_read_plan"][1]) == 10
    assert ctypes.sizeof(_native.Read) == 32
    assert [_native.Read.block.offset, _native.Read.shard.offset, _native.Read.offset.offset,
            _native.Read.len.offset, _native.Read.dst_offset.offset] == [0, 4, 8, 16, 24]
    assert shmr_amd.ReedSolomon._READ_DTYPE.itemsize == 32
    header = re.sub(r"\s+", " ", open(_native._HERE + "/../include/shmr_ec.h").read())
    section = header[header.index("ranged reads from device-resident blocks"):header.index("shmr_ec_read_plan(")]
    assert "MUST NOT overlap" in section                     # the caller's contract on d_dst
    assert "NOT capturable" in section
    assert "damaged survivor" in section.lower() and "shmr_ec_reconstruct_checked_batch_dev" in section


def test_read_kernel_is_outside_the_inventory():
    """gf_read_kernel is its own __global__ function in the product library; the
    inventory stays what encode and reconstruct dispatch, and no counter or
    status was added."""
    data = open(_native._PATHS["product"], "rb").read()
    assert b"gf_read_kernel" in data
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv
    assert len(shmr_amd.device_stats(0)) == 12


def _read(L, h, rows=((0, 0, 0, 8, 0),), d=0x100000, present=ALL, nblocks=3, shard_len=64, dst=0x300000,
          dst_bytes=4096, device=0, reads="rows", nreads=None):
    v = ctypes.c_void_p
    arr = _reads(rows) if reads == "rows" else reads
    n = len(rows) if nreads is None else nreads
    pr = _present(present) if present is not None else None
    return L.shmr_ec_read_batch_dev(h, v(d), 64, 512, pr.ctypes.data_as(_native._u8p) if pr is not None else None,
                                    nblocks, shard_len, ctypes.cast(arr, v) if arr is not None else None, n, v(dst),
                                    dst_bytes, device, None)


def _plan(L, h, rows=((0, 0, 0, 8, 0),), present=ALL, nblocks=3, shard_len=64, dst_bytes=4096, reads="rows",
          nreads=None, want_rebuilt=True):
    arr = _reads(rows) if reads == "rows" else reads
    n = len(rows) if nreads is None else nreads
    pr = _present(present) if present is not None else None
    rebuilt = (ctypes.c_uint8 * max(n, 1))(*([0xee] * max(n, 1)))
    npieces, nchunks = ctypes.c_uint32(0xdead), ctypes.c_uint32(0xdead)
    rc = L.shmr_ec_read_plan(h, pr.ctypes.data_as(_native._u8p) if pr is not None else None, nblocks, shard_len,
                             ctypes.cast(arr, ctypes.c_void_p) if arr is not None else None, n, dst_bytes,
                             rebuilt if want_rebuilt else None, ctypes.byref(npieces), ctypes.byref(nchunks))
    return rc, list(rebuilt)[:n], npieces.value, nchunks.value


BAD_ROWS = [(3, 0, 0, 8, 0),                # block >= nblocks
            (0, K, 0, 8, 0),                # shard >= data (a parity shard cannot be requested)
            (0, T - 1, 0, 8, 0),
            (0, 0, 0, 0, 0),                # len == 0
            (0, 0, 57, 8, 0),               # offset + len > shard_len
            (0, 0, M64, 2, 0),              # ... past 2^64
            (0, 0, 2, M64, 0),
            (0, 0, 0, 8, 4089),             # dst_offset + len > dst_bytes
            (0, 0, 0, 8, M64 - 3)]          # ... past 2^64
TOO_FEW = [[1] * T, [0, 0, 0, 1, 1, 1], [1] * T]      # block 1: 3 of 4 present


def test_read_batch_dev_argument_order():
    """NULL rs -> InvalidArgument; no requests or no blocks -> Ok; shard_len == 0
    -> EmptyShard; a NULL pointer, a bad request, two intersecting destinations
    -> InvalidArgument; a block with fewer than k present -> TooFewShardsPresent;
    the device ID last.  The fake device addresses are never dereferenced."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    assert _read(L, None) == INVALID
    assert _read(L, None, nreads=0) == INVALID
    # nothing to do: Ok whatever else is wrong
    assert _read(L, h, nreads=0, reads=None, d=None, dst=None, present=None, shard_len=0, device=-5) == OK
    assert _read(L, h, nblocks=0, d=None, dst=None, present=None, shard_len=0, device=-5) == OK
    assert _read(L, h, rows=((7, 9, 0, 0, 0),), nblocks=0) == OK
    assert _read(L, h, shard_len=0) == EMPTY
    assert _read(L, h, shard_len=0, d=None, present=TOO_FEW, device=-5) == EMPTY
    for null in ("d", "dst", "present"):
        assert _read(L, h, device=-5, **{null: None}) == INVALID, null
    assert _read(L, h, reads=None, nreads=1, device=-5) == INVALID
    # a NULL pointer comes before the flags, a bad request too
    assert _read(L, h, d=None, present=TOO_FEW, device=-5) == INVALID
    for row in BAD_ROWS:
        assert _read(L, h, rows=(row,), device=-5) == INVALID, row
        assert _read(L, h, rows=((1, 1, 0, 8, 100), row), device=-5) == INVALID, row
        assert _read(L, h, rows=(row,), present=TOO_FEW, device=-5) == INVALID, row
    # two writes to one destination byte, in either order; the same source twice is fine
    assert _read(L, h, rows=((0, 0, 0, 8, 0), (1, 1, 0, 8, 7)), device=-5) == INVALID
    assert _read(L, h, rows=((1, 1, 0, 8, 7), (0, 0, 0, 8, 0)), device=-5) == INVALID
    assert _read(L, h, rows=((0, 0, 0, 8, 0), (1, 1, 0, 8, 7)), present=TOO_FEW, device=-5) == INVALID
    # every block's flags are checked, requested or not, before the device
    fine = ((0, 0, 0, 8, 0), (0, 0, 0, 8, 8), (0, 1, 0, 64, 100), (2, 3, 63, 1, 4095))
    assert _read(L, h, rows=fine, present=TOO_FEW, device=-5) == TOO_FEW_PRESENT
    assert _read(L, h, rows=((0, 0, 0, 8, 0),), present=TOO_FEW, device=-5) == TOO_FEW_PRESENT
    # the device ID comes last; well formed lists reach it
    for present in (ALL, DEGRADED):
        for device in (-1, 9999):
            assert _read(L, h, rows=fine, present=present, device=device) == (NO_DEVICE if _no_gpu() else INVALID)


def test_well_formed_call_without_a_gpu_is_no_device():
    """No CPU fallback, and a refused call counts nothing.  (With a GPU the
    well-formed call would run on the fake addresses: only the refusal is made.)"""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    before = shmr_amd.device_stats(0)
    if _no_gpu():
        assert _read(L, rs._h, rows=((0, 0, 0, 8, 0), (1, 0, 13, 40, 8)), present=DEGRADED) == NO_DEVICE
    assert _read(L, rs._h, rows=((0, 0, 0, 8, 0), (0, 1, 0, 8, 0))) == INVALID
    assert shmr_amd.device_stats(0) == before


def test_read_plan_refusals_in_order():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    n = ctypes.c_uint32()
    assert L.shmr_ec_read_plan(None, None, 0, 1, None, 0, 1, None, ctypes.byref(n), ctypes.byref(n)) == INVALID
    assert L.shmr_ec_read_plan(h, None, 0, 1, None, 0, 1, None, None, ctypes.byref(n)) == INVALID
    assert L.shmr_ec_read_plan(h, None, 0, 1, None, 0, 1, None, ctypes.byref(n), None) == INVALID
    assert _plan(L, h, rows=()) == (OK, [], 0, 0)
    assert _plan(L, h, nblocks=0, present=None, shard_len=0)[::2] == (OK, 0)
    assert _plan(L, h, shard_len=0, present=TOO_FEW)[0] == EMPTY
    assert _plan(L, h, present=None)[0] == INVALID
    assert _plan(L, h, reads=None, nreads=1)[0] == INVALID
    for row in BAD_ROWS:
        assert _plan(L, h, rows=(row,))[0] == INVALID, row
        assert _plan(L, h, rows=(row,), present=TOO_FEW)[0] == INVALID, row
    assert _plan(L, h, rows=((0, 0, 0, 8, 0), (1, 1, 0, 8, 7)), present=TOO_FEW)[0] == INVALID
    assert _plan(L, h, rows=((0, 0, 0, 8, 0), (1, 1, 0, 8, 8)), present=TOO_FEW)[0] == TOO_FEW_PRESENT
    assert _plan(L, h, rows=((0, 0, 0, 8, 0), (1, 1, 0, 8, 8)))[0] == OK


def test_read_plan_rebuilt_pieces_and_chunks():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(K, P)
    h = rs._h
    # DEGRADED: block 0 whole; block 1 lost data 0 and 3; block 2 lost data 2 and parity 5
    rows = [(b, s, 0, 16, 16 * (b * K + s)) for b in range(3) for s in range(K)]
    rc, rebuilt, npieces, nchunks = _plan(L, h, rows=rows, present=DEGRADED)
    assert (rc, npieces, nchunks) == (OK, 12, 1)
    assert rebuilt == [0 if DEGRADED[b][s] else 1 for b in range(3) for s in range(K)]
    assert sum(rebuilt) == 3
    # any non-zero flag is "present", as for the reconstruct
    odd = [[1] * T, [0, 7, 255, 0, 1, 2], [1] * T]
    assert _plan(L, h, rows=rows, present=odd)[1][4:8] == [1, 0, 0, 1]
    assert _plan(L, h, rows=rows, present=DEGRADED, want_rebuilt=False)[2:] == (12, 1)
    # pieces: head, whole chunks, tail
    assert _plan(L, h, rows=[(0, 0, 0, 64, 0)])[2] == 1
    assert _plan(L, h, rows=[(0, 0, 1, 63, 0)])[2] == 2
    assert _plan(L, h, rows=[(0, 0, 1, 62, 0)])[2] == 3
    assert _plan(L, h, rows=[(0, 0, 3, 9, 0)])[2] == 1
    assert _plan(L, h, rows=[(0, 0, 10, 9, 0)])[2] == 2
    # chunks: one ring slot (256 KiB) of 40-byte entries each
    per = 256 * 1024 // 40
    many = [(i % 3, i % K, 16 * (i % 4), 16, 16 * i) for i in range(per + 1)]
    assert _plan(L, h, rows=many[:per], dst_bytes=1 << 30)[2:] == (per, 1)
    assert _plan(L, h, rows=many, dst_bytes=1 << 30)[2:] == (per + 1, 2)


def test_block_range_reads():
    f = shmr_amd.ReedSolomon.block_range_reads
    S = 1000
    assert f(5, 0, 0, S) == []
    assert f(5, 10, 20, S) == [(5, 0, 10, 20, 0)]
    assert f(5, 10, 20, S, dst_offset=7) == [(5, 0, 10, 20, 7)]
    # exactly one shard, and up to a boundary without crossing it
    assert f(0, 2000, 1000, S) == [(0, 2, 0, 1000, 0)]
    assert f(0, 1990, 10, S) == [(0, 1, 990, 10, 0)]
    # across one boundary
    assert f(1, 990, 20, S, 100) == [(1, 0, 990, 10, 100), (1, 1, 0, 10, 110)]
    # across several
    assert f(2, 999, 2003, S) == [(2, 0, 999, 1, 0), (2, 1, 0, 1000, 1), (2, 2, 0, 1000, 1001), (2, 3, 0, 2, 2001)]
    # the payload's end: the last byte of the last data shard of RS(4, 2)
    assert f(0, 4 * S - 1, 1, S) == [(0, 3, 999, 1, 0)]
    assert f(0, 3 * S - 5, S + 5, S) == [(0, 2, 995, 5, 0), (0, 3, 0, 1000, 5)]
    whole = f(3, 0, 4 * S, S, 64)
    assert whole == [(3, s, 0, S, 64 + s * S) for s in range(4)]
    # lengths add up and destinations follow one another
    rows = f(9, 12345, 54321, 4117)
    assert sum(r[3] for r in rows) == 54321 and all(a[4] + a[3] == b[4] for a, b in zip(rows, rows[1:]))
    assert all(r[1] * 4117 + r[2] == 12345 + r[4] for r in rows)
    # past the payload the shard index says so: the read call refuses shard >= data
    rs = shmr_amd.ReedSolomon(K, P)
    over = f(0, 4 * S - 1, 2, S)
    assert over[-1] == (0, 4, 0, 1, 1)
    with pytest.raises(shmr_amd.Error) as e:
        rs.read_plan(np.ones((1, T), np.uint8), over, S, 16)
    assert e.value.name == "InvalidArgument"
    assert rs.read_plan(np.ones((1, T), np.uint8), f(0, 0, 4 * S, S), S, 4 * S)[1] >= 4
    for bad in [(-1, 0, 1, S), (0, -1, 1, S), (0, 0, -1, S), (0, 0, 1, 0)]:
        with pytest.raises(ValueError):
            f(*bad)


def test_python_read_plan_and_list_conversion():
    rs = shmr_amd.ReedSolomon(K, P)
    present = np.array(DEGRADED, dtype=bool)
    rows = [(1, 0, 0, 64, 0), (1, 1, 0, 64, 64), (2, 2, 5, 20, 128)]
    rebuilt, npieces, nchunks = rs.read_plan(present, rows, 64, 256)
    assert rebuilt.dtype == np.uint8 and rebuilt.tolist() == [1, 0, 1] and (npieces, nchunks) == (1 + 1 + 2, 1)
    # an (n, 5) integer array is the same list
    assert rs.read_plan(present, np.array(rows, dtype=np.int64), 64, 256)[1] == 4
    assert rs.read_plan(present, [], 64, 256)[1:] == (0, 0)
    with pytest.raises(shmr_amd.Error) as e:
        rs.read_plan(present, [(0, 0, 0, 65, 0)], 64, 256)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(shmr_amd.Error) as e:
        rs.read_plan(np.array(TOO_FEW), rows, 64, 256)
    assert e.value.name == "TooFewShardsPresent"
    with pytest.raises(shmr_amd.Error) as e:
        rs.read_plan(present, [(0, 0, -1, 8, 0)], 64, 256)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(shmr_amd.Error):
        rs.read_plan(present, [(1 << 32, 0, 0, 8, 0)], 64, 256)
    with pytest.raises(shmr_amd.Error):
        rs.read_plan(present, np.array([[0, 0, 0, 8, -1]]), 64, 256)
    with pytest.raises(TypeError):
        rs.read_plan(present, [(0, 0, 0, 8)], 64, 256)
    with pytest.raises(TypeError):
        rs.read_plan(present, [(0, 0, 0.5, 8, 0)], 64, 256)
    with pytest.raises(TypeError):
        rs.read_plan(present, [(0, 0, True, 8, 0)], 64, 256)
    with pytest.raises(TypeError):
        rs.read_plan(present, np.zeros((2, 4), dtype=np.int64), 64, 256)
    with pytest.raises(TypeError):
        rs.read_plan(present, np.zeros((2, 5), dtype=np.float32), 64, 256)
    with pytest.raises(ValueError):
        rs.read_plan(np.ones(T + 1, np.uint8), rows, 64, 256)


def test_python_checks_precede_device_use():
    """read_batch_dev applies reconstruct_batch_dev's tensor checks in its order,
    then requires dst to be a 1-D uint8 tensor on the same device."""
    import torch
    rs = shmr_amd.ReedSolomon(K, P)
    shards = torch.zeros((3, T, 1024), dtype=torch.uint8)
    present = np.ones((3, T), dtype=np.uint8)
    dst = torch.zeros(64, dtype=torch.uint8)
    reads = [(0, 0, 0, 8, 0)]
    fn = rs.read_batch_dev
    with pytest.raises(TypeError):
        fn(shards.float(), present, reads, dst)
    with pytest.raises(TypeError):
        fn(shards.reshape(3, -1), present, reads, dst)
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards[:, :5], present, reads, dst)
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards, present, reads, dst, shard_len=1025)
    assert e.value.name == "IncorrectShardSize"
    with pytest.raises(shmr_amd.Error) as e:
        fn(shards, present, reads, dst, shard_len=0)
    assert e.value.name == "EmptyShard"
    with pytest.raises(ValueError):
        fn(shards, present[:2], reads, dst)
    with pytest.raises(TypeError):                               # well formed, but pageable host memory
        fn(shards, present, reads, dst, shard_len=1000)
