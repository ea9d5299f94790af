"""CPU tests of the parity delta update entry points of the C ABI
(include/shmr_ec.h): shmr_ec_update_batch_dev and shmr_ec_update_rounds.  Both
are exported by both library flavours and declared in _native.py; the batch
call checks its arguments, the update list included, before any device work.
No kernel is launched here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY = 0, -100, -101, -11
NAMES = {"shmr_ec_update_batch_dev", "shmr_ec_update_rounds"}
M64 = (1 << 64) - 1


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _updates(rows):
    arr = (_native.Update * max(len(rows), 1))()
    for i, row in enumerate(rows):
        arr[i] = _native.Update(*row)
    return arr


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_symbols_exported_and_declared(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (shmr_ec_\w+)", out))
    lib = _native._load(flavour)
    declared = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name) and name in declared
    assert len(declared["shmr_ec_update_batch_dev"][1]) == 15 and len(declared["shmr_ec_update_rounds"][1]) == 8
    assert ctypes.sizeof(_native.Update) == 32
    assert [(_native.Update.block.offset), _native.Update.shard.offset, _native.Update.offset.offset,
            _native.Update.len.offset, _native.Update.src_offset.offset] == [0, 4, 8, 16, 24]
    assert shmr_amd.ReedSolomon._UPDATE_DTYPE.itemsize == 32
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    assert "must not overlap" in re.sub(r"\s+", " ", header).lower()        # the caller's contract on d_src


def test_update_kernel_is_outside_the_inventory():
    """gf_update_kernel is its own __global__ function in the product library;
    the inventory stays what encode and reconstruct dispatch, the gf_apply kernels."""
    data = open(_native._PATHS["product"], "rb").read()
    assert b"gf_update_kernel" in data
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv
    assert len(shmr_amd.device_stats(0)) == 12                              # no device counter was added


def _update(L, h, rows=((0, 0, 0, 8, 0),), d=0x100000, p=0x200000, nblocks=3, shard_len=64, src=0x300000,
            src_bytes=4096, device=0, updates="rows", nupdates=None):
    v = ctypes.c_void_p
    arr = _updates(rows) if updates == "rows" else updates
    n = len(rows) if nupdates is None else nupdates
    return L.shmr_ec_update_batch_dev(h, v(d), 64, 256, v(p), 64, 128, nblocks, shard_len,
                                      ctypes.cast(arr, v) if arr is not None else None, n, v(src), src_bytes,
                                      device, None)


def test_update_batch_dev_argument_order():
    """NULL rs -> InvalidArgument; no updates or no blocks -> Ok; shard_len == 0
    -> EmptyShard; a NULL pointer, a bad update, two intersecting updates of one
    (block, shard) -> InvalidArgument; the device ID last.  The fake device
    addresses are never dereferenced on the host."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(4, 2)
    h = rs._h
    assert _update(L, None) == INVALID
    assert _update(L, None, nupdates=0) == INVALID
    # nothing to do: Ok whatever else is wrong
    assert _update(L, h, nupdates=0, updates=None, d=None, p=None, src=None, shard_len=0, device=-5) == OK
    assert _update(L, h, nblocks=0, d=None, p=None, src=None, shard_len=0, device=-5) == OK
    assert _update(L, h, rows=((7, 9, 0, 0, 0),), nblocks=0) == OK
    assert _update(L, h, shard_len=0) == EMPTY
    assert _update(L, h, shard_len=0, d=None, device=-5) == EMPTY
    for null in ("d", "p", "src"):
        assert _update(L, h, device=-5, **{null: None}) == INVALID, null
    assert _update(L, h, updates=None, nupdates=1, device=-5) == INVALID
    bad = [(3, 0, 0, 8, 0),                # block >= nblocks
           (0, 4, 0, 8, 0),                # shard >= data
           (0, 0, 0, 0, 0),                # len == 0
           (0, 0, 57, 8, 0),               # offset + len > shard_len
           (0, 0, M64, 2, 0),              # ... past 2^64
           (0, 0, 2, M64, 0),
           (0, 0, 0, 8, 4089),             # src_offset + len > src_bytes
           (0, 0, 0, 8, M64 - 3)]          # ... past 2^64
    for row in bad:
        assert _update(L, h, rows=(row,), device=-5) == INVALID, row
        assert _update(L, h, rows=((1, 1, 0, 8, 0), row), device=-5) == INVALID, row
    # two writes to one byte of a shard
    assert _update(L, h, rows=((0, 0, 0, 8, 0), (0, 0, 7, 8, 8)), device=-5) == INVALID
    assert _update(L, h, rows=((0, 0, 0, 64, 0), (0, 1, 0, 64, 0), (0, 0, 63, 1, 0)), device=-5) == INVALID
    # the device ID comes last; well formed lists reach it
    fine = ((0, 0, 0, 8, 0), (0, 0, 8, 8, 8), (0, 1, 0, 64, 100), (2, 3, 63, 1, 4095))
    for device in (-1, 9999):
        assert _update(L, h, rows=fine, device=device) == (NO_DEVICE if _no_gpu() else INVALID)


def test_well_formed_call_without_a_gpu_is_no_device():
    """No CPU fallback, and a refused call counts nothing.  (With a GPU the
    well-formed call would run on the fake addresses: only the refusal is made.)"""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(8, 3)
    before = shmr_amd.device_stats(0)
    if _no_gpu():
        assert _update(L, rs._h, rows=((0, 0, 0, 8, 0), (1, 7, 13, 40, 8))) == NO_DEVICE
    assert _update(L, rs._h, rows=((0, 0, 0, 8, 0), (0, 0, 0, 8, 0))) == INVALID
    assert shmr_amd.device_stats(0) == before


def _rounds(L, h, rows, nblocks=3, shard_len=5000, src_bytes=1 << 30, want_rounds=True):
    n = len(rows)
    arr = _updates(rows)
    round_of = (ctypes.c_uint32 * max(n, 1))(*([0xdead] * max(n, 1)))
    nrounds = ctypes.c_uint32(0xdead)
    rc = L.shmr_ec_update_rounds(h, ctypes.cast(arr, ctypes.c_void_p), n, nblocks, shard_len, src_bytes,
                                 round_of if want_rounds else None, ctypes.byref(nrounds))
    return rc, list(round_of)[:n], nrounds.value


def test_update_rounds_through_ctypes():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(8, 3)
    h = rs._h
    S = 5000
    assert L.shmr_ec_update_rounds(None, None, 0, 1, 1, 1, None, ctypes.byref(ctypes.c_uint32())) == INVALID
    assert L.shmr_ec_update_rounds(h, None, 0, 1, 1, 1, None, None) == INVALID
    assert _rounds(L, h, []) == (OK, [], 0)
    assert _rounds(L, h, [(0, 0, 0, 8, 0)], nblocks=0)[::2] == (OK, 0)
    assert _rounds(L, h, [(0, 0, 0, 8, 0)], shard_len=0)[0] == EMPTY
    assert L.shmr_ec_update_rounds(h, None, 1, 1, 64, 64, None, ctypes.byref(ctypes.c_uint32())) == INVALID
    # disjoint: one round; neighbours inside a 16-byte chunk share it (byte-exact edge stores)
    assert _rounds(L, h, [(0, 0, 0, 100, 0), (0, 1, 100, 100, 0), (1, 0, 0, 100, 0)]) == (OK, [0, 0, 0], 1)
    assert _rounds(L, h, [(0, 0, 0, 8, 0), (0, 0, 8, 8, 8)]) == (OK, [0, 0], 1)
    assert _rounds(L, h, [(0, 0, 5, 4, 0), (0, 1, 9, 14, 4)]) == (OK, [0, 0], 1)
    # the same columns of m shards: m rounds
    rc, rounds, n = _rounds(L, h, [(0, 0, 0, S, 0), (0, 1, 0, S, S)])
    assert (rc, sorted(rounds), n) == (OK, [0, 1], 2)
    rc, rounds, n = _rounds(L, h, [(2, s, 0, S, s * S) for s in range(8)])
    assert (rc, sorted(rounds), n) == (OK, list(range(8)), 8)
    rc, _, n = _rounds(L, h, [(2, s, 0, S, s * S) for s in range(8)], want_rounds=False)
    assert (rc, n) == (OK, 8)
    # refusals: as the batch call's
    for row in [(3, 0, 0, 8, 0), (0, 8, 0, 8, 0), (0, 0, 0, 0, 0), (0, 0, S - 7, 8, 0), (0, 0, M64, 2, 0),
                (0, 0, 0, 8, (1 << 30) - 7)]:
        assert _rounds(L, h, [row])[0] == INVALID, row
    assert _rounds(L, h, [(0, 0, 0, 8, 0), (0, 0, 7, 1, 0)])[0] == INVALID


def test_python_update_rounds():
    rs = shmr_amd.ReedSolomon(4, 2)
    round_of, n = rs.update_rounds([(0, 0, 0, 64, 0), (0, 1, 0, 64, 64), (1, 1, 0, 64, 0)], 2, 64, 128)
    assert n == 2 and round_of.dtype == np.uint32 and sorted(round_of[:2].tolist()) == [0, 1] and round_of[2] == 0
    # an (n, 5) integer array is the same list
    arr = np.array([(0, 0, 0, 64, 0), (0, 1, 0, 64, 64), (1, 1, 0, 64, 0)], dtype=np.int64)
    assert rs.update_rounds(arr, 2, 64, 128)[1] == 2
    assert rs.update_rounds([], 2, 64, 128)[1] == 0
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_rounds([(0, 0, 0, 65, 0)], 2, 64, 128)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_rounds([(0, 0, -1, 8, 0)], 2, 64, 128)
    assert e.value.name == "InvalidArgument"
    with pytest.raises(shmr_amd.Error):
        rs.update_rounds([(1 << 32, 0, 0, 8, 0)], 2, 64, 128)
    with pytest.raises(TypeError):
        rs.update_rounds([(0, 0, 0, 8)], 2, 64, 128)
    with pytest.raises(TypeError):
        rs.update_rounds([(0, 0, 0.5, 8, 0)], 2, 64, 128)
    with pytest.raises(TypeError):
        rs.update_rounds(np.zeros((2, 4), dtype=np.int64), 2, 64, 128)
    with pytest.raises(TypeError):
        rs.update_rounds(np.zeros((2, 5), dtype=np.float32), 2, 64, 128)


def test_python_checks_precede_device_use():
    """update_batch_dev applies encode_batch_dev's tensor checks in its order,
    then requires src to be a 1-D uint8 tensor on the same device."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 2)
    data = torch.zeros((3, 4, 1024), dtype=torch.uint8)
    parity = torch.zeros((3, 2, 1024), dtype=torch.uint8)
    src = torch.zeros(64, dtype=torch.uint8)
    ups = [(0, 0, 0, 8, 0)]
    fn = rs.update_batch_dev
    with pytest.raises(TypeError):
        fn(data.float(), parity, ups, src)
    with pytest.raises(shmr_amd.Error) as e:
        fn(data[:, :3], parity, ups, src)
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        fn(data, parity, ups, src, shard_len=1025)
    assert e.value.name == "IncorrectShardSize"
    with pytest.raises(shmr_amd.Error) as e:
        fn(data, parity, ups, src, shard_len=0)
    assert e.value.name == "EmptyShard"
    with pytest.raises(ValueError):
        fn(data, parity[:2], ups, src)
    with pytest.raises(TypeError):                               # well formed, but pageable host memory
        fn(data, parity, ups, src, shard_len=1000)
    with pytest.raises(shmr_amd.Error) as e:
        rs.update_shards_dev(torch.zeros((3, 5, 1024), dtype=torch.uint8), ups, src)
    assert e.value.name == "TooFewShards"
    with pytest.raises(TypeError):
        rs.update_shards_dev(torch.zeros((3, 6 * 1024), dtype=torch.uint8), ups, src)
