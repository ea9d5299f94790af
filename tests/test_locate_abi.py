"""CPU tests of the scrub entry points of the C ABI (include/shmr_ec.h):
shmr_ec_locate_work_size, shmr_ec_locate_batch_dev and shmr_ec_scrub_batch_dev.
All three are exported by both library flavours and declared in _native.py;
the batch calls check their arguments before any device work.  No kernel is
launched here.
"""
import ctypes
import re
import subprocess

import pytest

import shmr_amd
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY = 0, -100, -101, -11
NAMES = {"shmr_ec_locate_work_size", "shmr_ec_locate_batch_dev", "shmr_ec_scrub_batch_dev"}


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_symbols_exported_and_declared(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    assert NAMES <= set(re.findall(r"\bT (shmr_ec_\w+)", out))
    lib = _native._load(flavour)
    declared = {name: (res, args) for name, res, args in _native.SIGNATURES}
    for name in NAMES:
        assert hasattr(lib, name) and name in declared
    assert declared["shmr_ec_locate_work_size"][0] is ctypes.c_size_t
    assert len(declared["shmr_ec_locate_batch_dev"][1]) == 15 and len(declared["shmr_ec_scrub_batch_dev"][1]) == 13
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    assert re.search(r"#define SHMR_EC_LOCATE_CLEAN \(-1\)", header) and re.search(r"#define SHMR_EC_LOCATE_NONE \(-2\)", header)


def test_locate_kernels_are_outside_the_inventory():
    """The locate kernels are their own __global__ templates (R = 2..4 rows of
    the first row group, modes 0-2) plus the resolve kernel; the inventory
    stays what encode and reconstruct dispatch, the gf_apply kernels."""
    data = open(_native._PATHS["product"], "rb").read()
    locate = set(re.findall(rb"gf_locate_kernelILi(\d+)ELi(\d+)E", data))
    assert {(int(r), int(m)) for r, m in locate} == {(r, m) for r in (2, 3, 4) for m in (0, 1, 2)}
    assert b"gf_locate_resolve_kernel" in data
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv


@pytest.mark.parametrize("k,p", [(4, 2), (8, 3), (40, 4), (200, 32)])
def test_work_size_is_positive_and_monotonic(k, p):
    rs = shmr_amd.ReedSolomon(k, p)
    sizes = [rs.locate_work_size(n) for n in (0, 1, 2, 5, 64, 65, 1000, 1 << 20)]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes)
    words = (k + 31) // 32
    for n, s in zip((1, 2, 5, 64, 65, 1000, 1 << 20), sizes[1:]):
        assert s >= n * words * 4, "a candidate bitmap of ceil(k / 32) words per block"
    assert sizes[-1] > sizes[1]
    assert _native.lib().shmr_ec_locate_work_size(None, 5) == 0
    assert shmr_amd.ReedSolomon(k, 1).locate_work_size(5) == 0      # a codec the call refuses


def _locate(L, h, d=0x100000, p=0x200000, nblocks=3, shard_len=64, m=0x300000, loc=0x400000, w=0x500000,
            work_bytes=1 << 16, device=0):
    v = ctypes.c_void_p
    return L.shmr_ec_locate_batch_dev(h, v(d), 64, 256, v(p), 64, 128, nblocks, shard_len, v(m), v(loc), v(w),
                                      work_bytes, device, None)


def test_locate_batch_dev_argument_order():
    """NULL rs or a codec that cannot locate -> InvalidArgument; nblocks == 0 ->
    Ok; shard_len == 0 -> EmptyShard; NULL or misaligned pointers and a short
    work buffer -> InvalidArgument; the device ID last.  The fake device
    addresses are never dereferenced on the host."""
    L = _native.lib()
    rs, one, many = shmr_amd.ReedSolomon(4, 2), shmr_amd.ReedSolomon(4, 1), shmr_amd.ReedSolomon(4, 33)
    h = rs._h
    assert _locate(L, None) == INVALID
    assert _locate(L, one._h) == INVALID                                    # p < 2: nothing to locate with
    assert _locate(L, one._h, nblocks=0) == INVALID
    assert _locate(L, many._h) == INVALID                                   # p > 32: rows share bit 31
    assert _locate(L, h, nblocks=0) == OK
    assert _locate(L, h, nblocks=0, d=None, loc=None, w=None, work_bytes=0, device=-5) == OK
    assert _locate(L, h, shard_len=0) == EMPTY
    assert _locate(L, h, shard_len=0, d=None, device=-5) == EMPTY
    for null in ("d", "p", "m", "loc", "w"):
        assert _locate(L, h, **{null: None}) == INVALID, null
    assert _locate(L, h, m=0x300002) == INVALID
    assert _locate(L, h, loc=0x400001) == INVALID
    assert _locate(L, h, w=0x500002) == INVALID
    need = rs.locate_work_size(3)
    assert _locate(L, h, work_bytes=need - 1, device=-5) == INVALID
    assert _locate(L, h, work_bytes=0) == INVALID
    for device in (-1, 9999):
        assert _locate(L, h, device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        assert _locate(L, h, work_bytes=need) == NO_DEVICE                  # well formed: no CPU fallback


def test_scrub_batch_dev_argument_order():
    L = _native.lib()
    rs, one = shmr_amd.ReedSolomon(4, 2), shmr_amd.ReedSolomon(4, 1)
    v = ctypes.c_void_p
    located = (ctypes.c_int32 * 3)(7, 7, 7)
    counts = (ctypes.c_uint64 * 3)(9, 9, 9)

    def call(h=rs._h, d=0x100000, p=0x200000, nblocks=3, shard_len=64, loc=located, cnt=counts, device=0):
        return L.shmr_ec_scrub_batch_dev(h, v(d), 64, 256, v(p), 64, 128, nblocks, shard_len, loc, cnt, device, None)

    assert call(h=None) == INVALID
    assert call(cnt=None) == INVALID
    assert call(h=one._h) == INVALID
    assert list(counts) == [9, 9, 9], "a refused call wrote the counts"
    assert call(nblocks=0, loc=None) == OK and list(counts) == [0, 0, 0]
    # every other refusal leaves the counts alone as well
    counts[:] = [9, 9, 9]
    assert call(shard_len=0) == EMPTY
    assert call(d=None) == INVALID and call(p=None) == INVALID
    for device in (-1, 9999):
        assert call(device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        assert call() == NO_DEVICE
    assert list(counts) == [9, 9, 9], "a refused call wrote the counts"
    assert list(located) == [7, 7, 7]


def test_python_checks_precede_device_use():
    """The locate and scrub methods apply verify_batch_dev's tensor checks."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 2)
    data = torch.zeros((3, 4, 1024), dtype=torch.uint8)
    parity = torch.zeros((3, 2, 1024), dtype=torch.uint8)
    for fn in (rs.locate_batch_dev, rs.scrub_batch_dev):
        with pytest.raises(TypeError):
            fn(data.float(), parity)
        with pytest.raises(shmr_amd.Error) as e:
            fn(data[:, :3], parity)
        assert e.value.name == "TooFewShards"
        with pytest.raises(shmr_amd.Error) as e:
            fn(data, parity, shard_len=1025)
        assert e.value.name == "IncorrectShardSize"
        with pytest.raises(shmr_amd.Error) as e:
            fn(data, parity, shard_len=0)
        assert e.value.name == "EmptyShard"
        with pytest.raises(ValueError):
            fn(data, parity[:2])
        with pytest.raises(TypeError):                           # well formed, but pageable host memory
            fn(data, parity, shard_len=1000)
    for fn in (rs.locate_shards_dev, rs.scrub_shards_dev):
        with pytest.raises(shmr_amd.Error) as e:
            fn(torch.zeros((3, 5, 1024), dtype=torch.uint8))
        assert e.value.name == "TooFewShards"
        with pytest.raises(TypeError):
            fn(torch.zeros((3, 6 * 1024), dtype=torch.uint8))
