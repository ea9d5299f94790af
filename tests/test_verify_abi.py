"""CPU tests of the verify entry points of the C ABI (include/shmr_ec.h):
shmr_ec_verify (ReedSolomon::verify on host shards) and
shmr_ec_verify_batch_dev (device-resident batches).  Both are exported by
both library flavours and check their arguments -- the crate's checks in the
crate's order -- before any device work.  No kernel is launched here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from shmr_amd import _native

OK, INVALID, NO_DEVICE = 0, -100, -101
TOO_FEW, TOO_MANY, BAD_SIZE, EMPTY = -1, -2, -9, -11
u8p = _native._u8p


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _host_args(arrs):
    n = len(arrs)
    ptrs = (u8p * max(n, 1))(*[a.ctypes.data_as(u8p) if a.size else ctypes.cast(ctypes.c_void_p(1), u8p)
                               for a in arrs])
    lens = (ctypes.c_size_t * max(n, 1))(*[a.size for a in arrs])
    return ptrs, lens, n


def _device_untouched():
    """No per-device object was created and nothing was counted on device 0."""
    st = shmr_amd.device_stats(0)
    return all(st[key] == 0 for key in ("blocks_verified", "launches", "plan_images", "staging_streams",
                                        "blocking_calls"))


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_both_symbols_exported(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    exported = set(re.findall(r"\bT (shmr_ec_\w+)", out))
    assert {"shmr_ec_verify", "shmr_ec_verify_batch_dev"} <= exported
    lib = _native._load(flavour)
    assert hasattr(lib, "shmr_ec_verify") and hasattr(lib, "shmr_ec_verify_batch_dev")


def test_verify_kernels_are_outside_the_inventory():
    """The parity check kernels are their own __global__ template: no
    gf_apply_kernel instantiation was added for them, and the inventory (what
    encode and reconstruct dispatch) does not list them."""
    data = open(_native._PATHS["product"], "rb").read()
    assert b"gf_verify_kernel" in data
    verify = set(re.findall(rb"gf_verify_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    # R = 1..4 for each of the modes 0 (full tiles), 1 (tail) and 2 (byte-granular)
    assert {(int(r), int(m)) for r, u, m, f in verify} == {(r, m) for r in (1, 2, 3, 4) for m in (0, 1, 2)}
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv


def test_verify_checks_in_the_crates_order():
    """count (TooFew, TooMany), then EmptyShard, then IncorrectShardSize -- each
    while the later faults are present too -- before any device work."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(3, 2)
    ok = ctypes.c_int(7)

    def call(arrs):
        ptrs, lens, n = _host_args(arrs)
        return L.shmr_ec_verify(rs._h, ptrs, lens, n, ctypes.byref(ok))

    empty = [np.zeros(0, np.uint8) for _ in range(8)]
    uneven = [np.zeros(4, np.uint8) for _ in range(4)] + [np.zeros(5, np.uint8)]
    assert call(empty[:4]) == TOO_FEW                  # ... although every shard is empty too
    assert call(empty[:6]) == TOO_MANY
    assert call(uneven[:4]) == TOO_FEW
    assert call(uneven + uneven[:1]) == TOO_MANY
    assert call(empty[:5]) == EMPTY
    assert call([np.zeros(0, np.uint8)] + uneven[1:]) == EMPTY    # ... although the lengths differ too
    assert call(uneven) == BAD_SIZE
    assert call([np.zeros(4, np.uint8), np.zeros(3, np.uint8)] + uneven[:3]) == BAD_SIZE
    assert ok.value == 7, "an error wrote *consistent"
    # NULL arguments
    ptrs, lens, n = _host_args([np.zeros(4, np.uint8) for _ in range(5)])
    assert L.shmr_ec_verify(None, ptrs, lens, n, ctypes.byref(ok)) == INVALID
    assert L.shmr_ec_verify(rs._h, None, lens, n, ctypes.byref(ok)) == INVALID
    assert L.shmr_ec_verify(rs._h, ptrs, None, n, ctypes.byref(ok)) == INVALID
    assert L.shmr_ec_verify(rs._h, ptrs, lens, n, None) == INVALID
    nulls = (u8p * 5)(*([ptrs[i] for i in range(4)] + [u8p()]))
    assert L.shmr_ec_verify(rs._h, nulls, lens, n, ctypes.byref(ok)) == INVALID
    if _no_gpu():
        assert _device_untouched()
        assert L.shmr_ec_verify(rs._h, ptrs, lens, n, ctypes.byref(ok)) == NO_DEVICE    # well formed: no CPU fallback
        assert ok.value == 7


def test_python_verify_raises_the_crates_errors():
    """ReedSolomon.verify raises what it raised when it ran a scratch encode:
    the checks of ReedSolomon.encode, in its order; bytes shards are accepted."""
    rs = shmr_amd.ReedSolomon(3, 2)
    cases = [([np.zeros(4, np.uint8)] * 4, "TooFewShards"),
             ([np.zeros(4, np.uint8)] * 6, "TooManyShards"),
             ([], "TooFewShards"),
             ([np.zeros(0, np.uint8) for _ in range(5)], "EmptyShard"),
             ([np.zeros(4, np.uint8) for _ in range(4)] + [np.zeros(5, np.uint8)], "IncorrectShardSize"),
             ([bytes(4)] * 4 + [bytes(3)], "IncorrectShardSize")]
    for shards, name in cases:
        with pytest.raises(shmr_amd.Error) as e:
            rs.verify(shards)
        assert e.value.name == name, shards
    if _no_gpu():
        with pytest.raises(shmr_amd.Error) as e:
            rs.verify([bytes(4)] * 5)
        assert e.value.name == "NoDevice"


def test_verify_batch_dev_argument_order():
    """NULL rs -> InvalidArgument; nblocks == 0 -> Ok; shard_len == 0 ->
    EmptyShard; any NULL pointer -> InvalidArgument; the device ID last.  The
    fake device addresses are never dereferenced on the host."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(4, 2)
    h = rs._h
    d, p, m = (ctypes.c_void_p(0x100000), ctypes.c_void_p(0x200000), ctypes.c_void_p(0x300000))

    def call(h=h, d=d, p=p, nblocks=3, shard_len=64, m=m, device=0):
        return L.shmr_ec_verify_batch_dev(h, d, 64, 256, p, 64, 128, nblocks, shard_len, m, device, None)

    assert call(h=None) == INVALID
    assert call(h=None, nblocks=0) == INVALID          # rs is checked first
    assert call(nblocks=0) == OK
    assert call(nblocks=0, shard_len=0, d=None, p=None, m=None, device=-5) == OK     # nothing to do
    assert call(shard_len=0) == EMPTY
    assert call(shard_len=0, d=None, device=-5) == EMPTY                             # before the pointers
    assert call(d=None) == INVALID
    assert call(p=None) == INVALID
    assert call(m=None) == INVALID
    assert call(m=None, device=-5) == INVALID
    assert call(m=ctypes.c_void_p(0x300002)) == INVALID                              # words are 4-byte aligned
    # the device ID, as shmr_ec_encode_batch_dev reports it
    # (both refuse these IDs before any device work)
    for device in (-1, 9999):
        want = L.shmr_ec_encode_batch_dev(h, d, 64, 256, p, 64, 128, 3, 64, device, None)
        assert want == (NO_DEVICE if _no_gpu() else INVALID)
        assert call(device=device) == want, device
    if _no_gpu():
        assert call() == NO_DEVICE == L.shmr_ec_encode_batch_dev(h, d, 64, 256, p, 64, 128, 3, 64, 0, None)
        assert _device_untouched()


def test_device_stats_carry_blocks_verified():
    assert shmr_amd.reed_solomon.DEVICE_COUNTERS[11] == "blocks_verified"
    assert len(shmr_amd.reed_solomon.DEVICE_COUNTERS) == 12
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    assert re.search(r"SHMR_EC_DEV_BLOCKS_VERIFIED\s*=\s*11\b", header)
    assert re.search(r"SHMR_EC_DEV_COUNTERS\s*=\s*12\b", header)
    st = shmr_amd.device_stats(3)
    assert st["blocks_verified"] == 0 and list(st) == list(shmr_amd.reed_solomon.DEVICE_COUNTERS)
    # the native counter exists: entry 11 is written (here: zero, nothing ran on device 5)
    out = (ctypes.c_uint64 * 12)(*([7] * 12))
    assert _native.lib().shmr_ec_device_stats(5, out, 12) == 0 and list(out) == [0] * 12


def test_python_batch_checks_precede_device_use():
    """verify_batch_dev applies encode_batch_dev's tensor checks, in its order."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 2)
    data = torch.zeros((3, 4, 1024), dtype=torch.uint8)
    parity = torch.zeros((3, 2, 1024), dtype=torch.uint8)
    with pytest.raises(TypeError):
        rs.verify_batch_dev(data.float(), parity)
    with pytest.raises(shmr_amd.Error) as e:
        rs.verify_batch_dev(data[:, :3], parity)
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        rs.verify_batch_dev(data, torch.zeros((3, 3, 1024), dtype=torch.uint8))
    assert e.value.name == "TooManyShards"
    with pytest.raises(shmr_amd.Error) as e:
        rs.verify_batch_dev(data, parity, shard_len=1025)
    assert e.value.name == "IncorrectShardSize"
    with pytest.raises(shmr_amd.Error) as e:
        rs.verify_batch_dev(data, parity, shard_len=0)
    assert e.value.name == "EmptyShard"
    with pytest.raises(ValueError):
        rs.verify_batch_dev(data, parity[:2])
    with pytest.raises(TypeError):                               # well formed, but pageable host memory
        rs.verify_batch_dev(data, parity, shard_len=1000)
    with pytest.raises(shmr_amd.Error) as e:
        rs.verify_shards_dev(torch.zeros((3, 5, 1024), dtype=torch.uint8))
    assert e.value.name == "TooFewShards"
