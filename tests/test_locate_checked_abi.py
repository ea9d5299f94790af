"""CPU tests of the degraded-block entry points of the C ABI (include/shmr_ec.h):
shmr_ec_locate_checked_plan (host only), shmr_ec_locate_checked_batch_dev and
shmr_ec_reconstruct_repair_batch_dev.  All three are exported by both library
flavours and declared in _native.py; the batch calls check their arguments
before any device work.  No kernel is launched here.
"""
import ctypes
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from oracle import rs_oracle as O
from shmr_amd import _native

OK, INVALID, NO_DEVICE, EMPTY, TOO_FEW_PRESENT, TOO_FEW, TOO_MANY = 0, -100, -101, -11, -10, -1, -2
NAMES = {"shmr_ec_locate_checked_plan", "shmr_ec_locate_checked_batch_dev", "shmr_ec_reconstruct_repair_batch_dev"}


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
    assert len(declared["shmr_ec_locate_checked_batch_dev"][1]) == 14
    assert len(declared["shmr_ec_reconstruct_repair_batch_dev"][1]) == 11
    assert len(declared["shmr_ec_locate_checked_plan"][1]) == 9
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    for name in NAMES:
        assert re.search(r"\bint " + name + r"\(", header), name


def test_degraded_kernels_are_outside_the_inventory():
    """The degraded locate kernels are instantiations of their own (R = 2..4,
    modes 0-2) beside the complete-block ones, which keep their names; the
    inventory stays what encode and reconstruct dispatch, the gf_apply kernels."""
    data = open(_native._PATHS["product"], "rb").read()
    want = {(r, m) for r in (2, 3, 4) for m in (0, 1, 2)}
    for name in (rb"gf_locate_kernel", rb"gf_locate_checked_kernel"):
        got = set(re.findall(name + rb"ILi(\d+)ELi(\d+)EEEv", data))
        assert {(int(r), int(m)) for r, m in got} == want, name
    assert b"gf_locate_checked_resolve_kernel" in data
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = [(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()]
    assert len(inv) == len(set(inv)) and set(inv) == {tuple(int(x) for x in key) for key in apply_keys}


def test_plan_contents_and_errors():
    rs = shmr_amd.ReedSolomon(8, 3)
    M = O.ReedSolomon(8, 3).matrix
    # one lost: s = 2, one ratio row
    present = [1] * 11
    present[2] = 0
    in_idx, out_idx, q, mask = rs.locate_checked_plan(present)
    assert in_idx == [0, 1, 3, 4, 5, 6, 7, 8] and out_idx == [9, 10] and mask == 6 == rs.checked_rows(present)
    D = O.mat_mul(M[out_idx], O.mat_invert(M[in_idx]))
    assert q.tolist() == [[O.gal_div(int(D[1][t]), int(D[0][t])) for t in range(8)]]
    # the checked plan's compare rows are the D the ratios come from
    _, c_out, c_rows, n_store = rs.checked_plan(present, rebuild=False)
    assert n_store == 0 and c_out == out_idx and c_rows.tolist() == D.tolist()
    # complete: the codec's own locate ratios (s = 3: two rows)
    in_idx, out_idx, q, mask = rs.locate_checked_plan([1] * 11)
    C = M[8:]
    assert in_idx == list(range(8)) and out_idx == [8, 9, 10] and mask == 7
    assert q.tolist() == [[O.gal_div(int(C[r][t]), int(C[0][t])) for t in range(8)] for r in (1, 2)]
    # s = 1 and s = 0: no ratio plan, nothing can be located
    in_idx, out_idx, q, mask = rs.locate_checked_plan([0, 0] + [1] * 9)
    assert out_idx == [10] and q.shape == (0, 8) and mask == 4
    in_idx, out_idx, q, mask = rs.locate_checked_plan([1, 0, 1, 0, 1, 0] + [1] * 5)
    assert in_idx == [0, 2, 4, 6, 7, 8, 9, 10] and out_idx == [] and q.shape == (0, 8) and mask == 0
    # s = 5: the first row group only (three ratio rows)
    wide = shmr_amd.ReedSolomon(6, 6)
    _, out_idx, q, mask = wide.locate_checked_plan([0] + [1] * 11)
    assert out_idx == [7, 8, 9, 10, 11] and q.shape == (3, 6) and mask == 62

    # errors: counts and presence as shmr_ec_reconstruct_plan
    for bad, name in (([1] * 10, "TooFewShards"), ([1] * 12, "TooManyShards"),
                      ([0, 0, 0, 0] + [1] * 7, "TooFewShardsPresent")):
        with pytest.raises(shmr_amd.Error) as e:
            rs.locate_checked_plan(bad)
        assert e.value.name == name
    L = _native.lib()
    pr = np.ones(11, dtype=np.uint8)
    pr[2] = 0
    u8 = ctypes.POINTER(ctypes.c_uint8)
    ii, oi = (ctypes.c_uint16 * 8)(), (ctypes.c_uint16 * 11)()
    rows = np.zeros(24, dtype=np.uint8)
    n, mask = ctypes.c_uint32(77), ctypes.c_uint32(77)

    def call(h=rs._h, present=pr, nshards=11, in_idx=ii, out_idx=oi, out=rows, out_len=24, n_rows=n, row_mask=mask):
        return L.shmr_ec_locate_checked_plan(h, present.ctypes.data_as(u8) if present is not None else None, nshards,
                                             in_idx, out_idx, out.ctypes.data_as(u8) if out is not None else None,
                                             out_len, ctypes.byref(n_rows) if n_rows is not None else None,
                                             ctypes.byref(row_mask) if row_mask is not None else None)

    for null in ("h", "present", "in_idx", "out_idx", "out", "n_rows", "row_mask"):
        assert call(**{null: None}) == INVALID, null
    assert call(nshards=10) == TOO_FEW and call(nshards=12) == TOO_MANY
    assert call(out_len=7) == INVALID                              # one ratio row of 8 does not fit
    assert (n.value, mask.value) == (77, 77), "a refused call wrote its outputs"
    assert call(out_len=8) == OK and (n.value, mask.value) == (1, 6)


def _locate(L, h, d=0x100000, present=None, nblocks=3, shard_len=64, flags=0, m=0x300000, loc=0x400000, w=0x500000,
            work_bytes=1 << 16, device=0, total=6):
    v = ctypes.c_void_p
    pr = np.ones(nblocks * total, dtype=np.uint8) if present is None else np.asarray(present, dtype=np.uint8)
    ptr = pr.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if present is not False else None
    return L.shmr_ec_locate_checked_batch_dev(h, v(d), 64, 512, ptr, nblocks, shard_len, flags, v(m), v(loc), v(w),
                                              work_bytes, device, None)


def test_locate_checked_batch_dev_argument_order():
    """NULL rs or a codec outside 2 <= parity <= 32 -> InvalidArgument; nblocks
    == 0 -> Ok; shard_len == 0 -> EmptyShard; NULL or misaligned pointers,
    unknown flags and a short work buffer -> InvalidArgument; a block with
    fewer than `data` present -> TooFewShardsPresent; the device ID last.  The
    fake device addresses are never dereferenced on the host."""
    L = _native.lib()
    rs, one, many = shmr_amd.ReedSolomon(4, 2), shmr_amd.ReedSolomon(4, 1), shmr_amd.ReedSolomon(4, 33)
    h = rs._h
    assert _locate(L, None) == INVALID
    assert _locate(L, one._h, total=5) == INVALID                   # p < 2: nothing to locate with
    assert _locate(L, one._h, total=5, nblocks=0) == INVALID
    assert _locate(L, many._h, total=37) == INVALID                 # p > 32: rows share bit 31
    assert _locate(L, h, nblocks=0) == OK
    assert _locate(L, h, nblocks=0, d=None, present=False, loc=None, w=None, work_bytes=0, flags=8, device=-5) == OK
    assert _locate(L, h, shard_len=0) == EMPTY
    assert _locate(L, h, shard_len=0, d=None, flags=8, device=-5) == EMPTY
    for null in ("d", "m", "loc", "w"):
        assert _locate(L, h, **{null: None}) == INVALID, null
    assert _locate(L, h, present=False) == INVALID
    assert _locate(L, h, m=0x300002) == INVALID
    assert _locate(L, h, loc=0x400001) == INVALID
    assert _locate(L, h, w=0x500002) == INVALID
    for flags in (4, 8, -1):
        assert _locate(L, h, flags=flags) == INVALID
    need = rs.locate_work_size(3)
    assert _locate(L, h, work_bytes=need - 1, device=-5) == INVALID
    assert _locate(L, h, work_bytes=0) == INVALID
    few = np.ones((3, 6), dtype=np.uint8)
    few[2, :3] = 0
    assert _locate(L, h, present=few.ravel(), device=-5) == TOO_FEW_PRESENT
    assert _locate(L, h, present=few.ravel(), flags=8) == INVALID    # the arguments before the batch's contents
    for device in (-1, 9999):
        assert _locate(L, h, device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        for flags in (0, 1, 2, 3):
            assert _locate(L, h, work_bytes=need, flags=flags) == NO_DEVICE   # well formed: no CPU fallback


def test_repair_batch_dev_argument_order():
    L = _native.lib()
    rs, one = shmr_amd.ReedSolomon(4, 2), shmr_amd.ReedSolomon(4, 1)
    v = ctypes.c_void_p
    located = (ctypes.c_int32 * 3)(7, 7, 7)
    counts = (ctypes.c_uint64 * 3)(9, 9, 9)
    ones = np.ones((3, 6), dtype=np.uint8)
    few = ones.copy()
    few[1, 1:4] = 0

    def call(h=rs._h, d=0x100000, present=ones, nblocks=3, shard_len=64, loc=located, cnt=counts, device=0):
        ptr = present.ctypes.data_as(ctypes.POINTER(ctypes.c_uint8)) if present is not None else None
        return L.shmr_ec_reconstruct_repair_batch_dev(h, v(d), 64, 512, ptr, nblocks, shard_len, loc, cnt, device, None)

    assert call(h=None) == INVALID
    assert call(cnt=None) == INVALID
    assert call(h=one._h) == INVALID
    assert list(counts) == [9, 9, 9], "a refused call wrote the counts"
    assert call(nblocks=0, loc=None, present=None, d=None) == OK and list(counts) == [0, 0, 0]
    # every other refusal leaves the counts alone as well
    counts[:] = [9, 9, 9]
    assert call(shard_len=0) == EMPTY
    assert call(shard_len=0, d=None, device=-5) == EMPTY
    assert call(d=None) == INVALID and call(present=None) == INVALID
    assert call(present=few, device=-5) == TOO_FEW_PRESENT
    for device in (-1, 9999):
        assert call(device=device) == (NO_DEVICE if _no_gpu() else INVALID)
    if _no_gpu():
        assert call() == NO_DEVICE
        assert call(loc=None) == NO_DEVICE
    assert list(counts) == [9, 9, 9], "a refused call wrote the counts"
    assert list(located) == [7, 7, 7]


def test_python_checks_precede_device_use():
    """The degraded-batch methods apply reconstruct_checked_batch_dev's tensor checks."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 2)
    shards = torch.zeros((3, 6, 1024), dtype=torch.uint8)
    present = np.ones((3, 6), dtype=np.uint8)
    for fn in (rs.locate_checked_batch_dev, rs.reconstruct_repair_batch_dev):
        with pytest.raises(TypeError):
            fn(shards.float(), present)
        with pytest.raises(TypeError):
            fn(shards.reshape(3, 6 * 1024), present)
        with pytest.raises(shmr_amd.Error) as e:
            fn(shards[:, :5], present)
        assert e.value.name == "TooFewShards"
        with pytest.raises(shmr_amd.Error) as e:
            fn(shards, present, shard_len=1025)
        assert e.value.name == "IncorrectShardSize"
        with pytest.raises(shmr_amd.Error) as e:
            fn(shards, present, shard_len=0)
        assert e.value.name == "EmptyShard"
        with pytest.raises(ValueError):
            fn(shards, present[:2])
        with pytest.raises(TypeError):                           # well formed, but pageable host memory
            fn(shards, present, shard_len=1000)
