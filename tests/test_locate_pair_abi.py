"""CPU tests of the two-shard scrub entry points of the C ABI (include/shmr_ec.h):
shmr_ec_locate_pair_work_size, shmr_ec_locate_pair_batch_dev,
shmr_ec_scrub_pair_batch_dev and shmr_ec_locate_pair_plan.  All are exported by
both library flavours and declared in _native.py; the batch calls check their
arguments before any device work.  No kernel is launched here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from locate_pair_ref import pair_coeffs_ref
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY = 0, -100, -101, -11
NAMES = {"shmr_ec_locate_pair_work_size", "shmr_ec_locate_pair_batch_dev", "shmr_ec_scrub_pair_batch_dev",
         "shmr_ec_locate_pair_plan"}
MAX_DATA = 29                              # locate_plan.hpp pair_max_data


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
    assert declared["shmr_ec_locate_pair_work_size"][0] is ctypes.c_size_t
    assert len(declared["shmr_ec_locate_pair_batch_dev"][1]) == 15
    assert len(declared["shmr_ec_scrub_pair_batch_dev"][1]) == 13
    assert len(declared["shmr_ec_locate_pair_plan"][1]) == 4


def test_pair_kernels_are_outside_the_inventory():
    """The pair kernel is its own __global__ template (modes 0-2) next to the
    preset, select and resolve kernels; the inventory stays the gf_apply kernels."""
    data = open(_native._PATHS["product"], "rb").read()
    assert {int(m) for m in re.findall(rb"gf_locate_pair_kernelILi(\d+)EE", data)} == {0, 1, 2}
    for name in (b"gf_locate_pair_preset_kernel", b"gf_locate_pair_select_kernel", b"gf_locate_pair_resolve_kernel"):
        assert name in data
    assert all("locate" not in str(e) for e in shmr_amd.kernel_inventory())


@pytest.mark.parametrize("k,p", [(4, 4), (10, 4), (5, 5), (MAX_DATA, 4), (8, 32)])
def test_work_size_is_positive_and_monotonic(k, p):
    rs = shmr_amd.ReedSolomon(k, p)
    counts = (0, 1, 2, 5, 64, 65, 1000, 1 << 20)
    sizes = [rs.locate_pair_work_size(n) for n in counts]
    assert all(s > 0 for s in sizes)
    assert sizes == sorted(sizes) and sizes[-1] > sizes[1]
    words = (k * (k - 1) // 2 + 4 * k + 31) // 32
    for n, s in zip(counts, sizes):
        # locate's scratch, the single answers, the pair bitmaps, the worklist and its counter
        assert s >= rs.locate_work_size(n) + n * 4 + n * words * 4 + n * 4 + 4, n


def test_refused_codecs_have_no_work_size_and_no_plan():
    assert _native.lib().shmr_ec_locate_pair_work_size(None, 5) == 0
    for k, p in [(4, 3), (4, 2), (4, 33), (MAX_DATA + 1, 4), (40, 8)]:
        rs = shmr_amd.ReedSolomon(k, p)
        assert rs.locate_pair_work_size(5) == 0, (k, p)
        with pytest.raises(shmr_amd.Error) as e:
            rs.locate_pair_plan()
        assert e.value.name == "InvalidArgument"


@pytest.mark.parametrize("k,p", [(10, 4), (4, 4), (5, 5), (8, 6), (MAX_DATA, 4)])
def test_plan_through_the_abi(k, p):
    rs = shmr_amd.ReedSolomon(k, p)
    npairs, dd, dp = rs.locate_pair_plan()
    want_dd, want_dp = pair_coeffs_ref(k, p)
    assert npairs == k * (k - 1) // 2 + 4 * k
    assert np.array_equal(dd, want_dd) and np.array_equal(dp, want_dp)
    # a short buffer and NULL pointers are refused
    L = _native.lib()
    buf = np.zeros(dd.size + dp.size, np.uint8)
    n = ctypes.c_uint32(7)
    p8 = buf.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8))
    assert L.shmr_ec_locate_pair_plan(rs._h, p8, buf.size - 1, ctypes.byref(n)) == INVALID
    assert L.shmr_ec_locate_pair_plan(rs._h, None, buf.size, ctypes.byref(n)) == INVALID
    assert L.shmr_ec_locate_pair_plan(rs._h, p8, buf.size, None) == INVALID
    assert L.shmr_ec_locate_pair_plan(None, p8, buf.size, ctypes.byref(n)) == INVALID
    assert n.value == 7 and not buf.any()
    assert L.shmr_ec_locate_pair_plan(rs._h, p8, buf.size, ctypes.byref(n)) == OK and n.value == npairs


def _locate(L, h, d=0x100000, p=0x200000, nblocks=3, shard_len=64, m=0x300000, loc=0x400000, w=0x500000,
            work_bytes=1 << 20, device=0):
    v = ctypes.c_void_p
    return L.shmr_ec_locate_pair_batch_dev(h, v(d), 64, 256, v(p), 64, 256, nblocks, shard_len, v(m), v(loc), v(w),
                                           work_bytes, device, None)


def test_locate_pair_batch_dev_argument_order():
    """NULL rs or a codec the call refuses -> InvalidArgument; nblocks == 0 ->
    Ok; shard_len == 0 -> EmptyShard; NULL or misaligned pointers and a short
    work buffer -> InvalidArgument; the device ID last.  The fake device
    addresses are never dereferenced on the host."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(4, 4)
    h = rs._h
    assert _locate(L, None) == INVALID
    for k, p in [(4, 3), (4, 33), (MAX_DATA + 1, 4)]:
        refused = shmr_amd.ReedSolomon(k, p)
        assert _locate(L, refused._h) == INVALID, (k, p)
        assert _locate(L, refused._h, nblocks=0) == INVALID, (k, p)
    assert _locate(L, h, nblocks=0) == OK
    assert _locate(L, h, nblocks=0, d=None, loc=None, w=None, work_bytes=0, device=-5) == OK
    assert _locate(L, h, shard_len=0) == EMPTY
    assert _locate(L, h, shard_len=0, d=None, device=-5) == EMPTY
    for null in ("d", "p", "m", "loc", "w"):
        assert _locate(L, h, **{null: None}) == INVALID, null
    assert _locate(L, h, m=0x300002) == INVALID
    assert _locate(L, h, loc=0x400001) == INVALID
    assert _locate(L, h, w=0x500002) == INVALID
    need = rs.locate_pair_work_size(3)
    assert _locate(L, h, work_bytes=need - 1, device=-5) == INVALID
    assert _locate(L, h, work_bytes=rs.locate_work_size(3), device=-5) == INVALID     # locate's scratch is not enough
    assert _locate(L, h, work_bytes=0) == INVALID
    for device in (-1, 9999):
        assert _locate(L, h, device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        assert _locate(L, h, work_bytes=need) == NO_DEVICE                  # well formed: no CPU fallback


def test_scrub_pair_batch_dev_argument_order():
    L = _native.lib()
    rs, three = shmr_amd.ReedSolomon(4, 4), shmr_amd.ReedSolomon(4, 3)
    v = ctypes.c_void_p
    located = (ctypes.c_int32 * 6)(*[7] * 6)
    counts = (ctypes.c_uint64 * 5)(*[9] * 5)

    def call(h=rs._h, d=0x100000, p=0x200000, nblocks=3, shard_len=64, loc=located, cnt=counts, device=0):
        return L.shmr_ec_scrub_pair_batch_dev(h, v(d), 64, 256, v(p), 64, 256, nblocks, shard_len, loc, cnt, device,
                                              None)

    assert call(h=None) == INVALID
    assert call(cnt=None) == INVALID
    assert call(h=three._h) == INVALID
    assert list(counts) == [9] * 5, "a refused call wrote the counts"
    assert call(nblocks=0, loc=None) == OK and list(counts) == [0, 0, 0, 0, 9], "four counts"
    # every other refusal leaves the counts alone as well
    counts[:] = [9] * 5
    assert call(shard_len=0) == EMPTY
    assert call(d=None) == INVALID and call(p=None) == INVALID
    for device in (-1, 9999):
        assert call(device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        assert call() == NO_DEVICE
    assert list(counts) == [9] * 5, "a refused call wrote the counts"
    assert list(located) == [7] * 6


def test_python_checks_precede_device_use():
    """The pair methods apply verify_batch_dev's tensor checks."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 4)
    data = torch.zeros((3, 4, 1024), dtype=torch.uint8)
    parity = torch.zeros((3, 4, 1024), dtype=torch.uint8)
    for fn in (rs.locate_pair_batch_dev, rs.scrub_pair_batch_dev):
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
    for fn in (rs.locate_pair_shards_dev, rs.scrub_pair_shards_dev):
        with pytest.raises(shmr_amd.Error) as e:
            fn(torch.zeros((3, 7, 1024), dtype=torch.uint8))
        assert e.value.name == "TooFewShards"
        with pytest.raises(TypeError):
            fn(torch.zeros((3, 8 * 1024), dtype=torch.uint8))
