"""CPU tests of the checked reconstruct's C ABI (include/shmr_ec.h):
shmr_ec_reconstruct_checked_batch_dev, shmr_ec_checked_rows and the host-only
shmr_ec_checked_plan.  Both library flavours export them; the batch call checks
its arguments in the documented order before any device work; the plan the GPU
runs is, per presence pattern, the reconstruct plan's rows verbatim followed by
the check rows M[surplus] * inv(M[first k present]), computed here in numpy
from oracle/rs_oracle.py.  No kernel is launched here.
"""
import ctypes
import itertools
import re
import subprocess

import numpy as np
import pytest

import shmr_amd
from shmr_amd import _native
from oracle import rs_oracle as O

OK, INVALID, NO_DEVICE = 0, -100, -101
TOO_FEW_SHARDS, TOO_MANY_SHARDS, TOO_FEW_PRESENT, EMPTY = -1, -2, -10, -11
DATA_ONLY, NO_REBUILD = 1, 2
u8p = _native._u8p
SYMBOLS = {"shmr_ec_reconstruct_checked_batch_dev", "shmr_ec_checked_rows", "shmr_ec_checked_plan"}


def _no_gpu():
    import torch
    return not torch.cuda.is_available()


def _device_untouched():
    """No per-device object was created and nothing was counted on device 0."""
    st = shmr_amd.device_stats(0)
    return all(st[key] == 0 for key in ("blocks_verified", "blocks_reconstructed", "launches", "plan_images",
                                        "staging_streams", "blocking_calls"))


def _bit(r):
    return 1 << min(r, 31)


def _split(present, k):
    """(first k present, surplus, absent) shard indices of a pattern."""
    idx = [i for i, x in enumerate(present) if x]
    return idx[:k], idx[k:], [i for i, x in enumerate(present) if not x]


def _mask(present, k):
    return sum({_bit(i - k) for i in _split(present, k)[1]})


def _sample(k, p, n, seed):
    """Seeded patterns of RS(k, p): exactly k present, all present, too few, and
    n random ones with at least k present."""
    rng = np.random.default_rng(seed)
    t = k + p
    out = [[1] * t, [1] * k + [0] * p, [0] * p + [1] * k, [1] * (k - 1) + [0] * (p + 1)]
    for _ in range(n):
        lost = rng.choice(t, size=int(rng.integers(1, p + 1)), replace=False)
        out.append([0 if i in lost else 1 for i in range(t)])
    return out


@pytest.mark.parametrize("flavour", ["product", "tools"])
def test_symbols_exported(flavour):
    out = subprocess.run(["nm", "-D", "--defined-only", _native._PATHS[flavour]], capture_output=True, text=True).stdout
    assert SYMBOLS <= set(re.findall(r"\bT (shmr_ec_\w+)", out))
    lib = _native._load(flavour)
    assert all(hasattr(lib, s) for s in SYMBOLS)
    assert SYMBOLS <= {name for name, _, _ in _native.SIGNATURES}
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    assert re.search(r"#define SHMR_EC_CHECK_DATA_ONLY 1\b", header)
    assert re.search(r"#define SHMR_EC_CHECK_NO_REBUILD 2\b", header)


def test_check_kernels_are_their_own_template():
    """gf_check_kernel<R, 1, MODE, F>, R = 1..4 for the modes 0 (full tiles), 1
    (tail) and 2 (byte-granular), 4 KiB tiles; outside the inventory, which
    still lists exactly the gf_apply_kernel instantiations."""
    data = open(_native._PATHS["product"], "rb").read()
    check = set(re.findall(rb"gf_check_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    assert {(int(r), int(u), int(m)) for r, u, m, f in check} == {(r, 1, m) for r in (1, 2, 3, 4) for m in (0, 1, 2)}
    apply_keys = set(re.findall(rb"gf_apply_kernelILi(\d+)ELi(\d+)ELi(\d+)ELi(\d+)E", data))
    inv = {(e["rows"], e["chunks"], e["mode"], e["flags"]) for e in shmr_amd.kernel_inventory()}
    assert {tuple(int(x) for x in key) for key in apply_keys} == inv


@pytest.mark.parametrize("k,p,patterns", [
    (4, 2, list(itertools.product((0, 1), repeat=6))),
    (8, 3, list(itertools.product((0, 1), repeat=11))),
    (10, 4, _sample(10, 4, 200, 104)),
    (5, 6, _sample(5, 6, 200, 56)),
    (2, 34, _sample(2, 34, 200, 234)),
], ids=lambda v: None if isinstance(v, list) else str(v))
def test_checked_rows_is_the_surplus_mask(k, p, patterns):
    rs = shmr_amd.ReedSolomon(k, p)
    seen = set()
    for pr in patterns:
        npres = sum(pr)
        if npres < k:
            with pytest.raises(shmr_amd.Error) as e:
                rs.checked_rows(pr)
            assert e.value.name == "TooFewShardsPresent"
            seen.add("few")
            continue
        want = _mask(pr, k)
        if npres == k:
            assert want == 0
            seen.add("k")
        if npres == k + p:
            assert want == sum({_bit(r) for r in range(p)})
            seen.add("all")
        assert rs.checked_rows(pr) == want, pr
    assert seen == {"few", "k", "all"}
    if p > 32:
        assert rs.checked_rows([1] * (k + p)) == 0xFFFFFFFF
        assert rs.checked_rows([1] * k + [0] * 31 + [1] * (p - 31)) == 1 << 31        # rows >= 31 share bit 31


def test_checked_rows_argument_checks():
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(4, 2)
    pr = np.ones(6, np.uint8)
    rows = ctypes.c_uint32(77)
    assert L.shmr_ec_checked_rows(None, pr.ctypes.data_as(u8p), 6, ctypes.byref(rows)) == INVALID
    assert L.shmr_ec_checked_rows(rs._h, None, 6, ctypes.byref(rows)) == INVALID
    assert L.shmr_ec_checked_rows(rs._h, pr.ctypes.data_as(u8p), 6, None) == INVALID
    assert L.shmr_ec_checked_rows(rs._h, pr.ctypes.data_as(u8p), 5, ctypes.byref(rows)) == TOO_FEW_SHARDS
    assert L.shmr_ec_checked_rows(rs._h, pr.ctypes.data_as(u8p), 7, ctypes.byref(rows)) == TOO_MANY_SHARDS
    assert rows.value == 77, "an error wrote *rows"
    assert L.shmr_ec_checked_rows(rs._h, pr.ctypes.data_as(u8p), 6, ctypes.byref(rows)) == OK and rows.value == 3


def test_batch_call_argument_order():
    """NULL rs -> InvalidArgument; nblocks == 0 -> Ok; shard_len == 0 ->
    EmptyShard; a NULL pointer or unknown flag bits -> InvalidArgument; a block
    with fewer than k present -> TooFewShardsPresent; the device ID last -- each
    with the later faults present too.  The fake device addresses are never
    dereferenced on the host."""
    L = _native.lib()
    rs = shmr_amd.ReedSolomon(4, 2)
    h = rs._h
    d, m = ctypes.c_void_p(0x100000), ctypes.c_void_p(0x300000)
    good = np.array([[1, 1, 1, 1, 1, 1], [1, 0, 1, 1, 1, 1], [0, 1, 1, 1, 0, 1]], np.uint8)
    few = good.copy()
    few[2] = [1, 0, 1, 0, 0, 1]                                  # the LAST block: every block is looked at

    def call(h=h, d=d, present=good, nblocks=3, shard_len=64, flags=0, m=m, device=0):
        pr = None if present is None else present.ctypes.data_as(u8p)
        return L.shmr_ec_reconstruct_checked_batch_dev(h, d, 64, 512, pr, nblocks, shard_len, flags, m, device, None)

    assert call(h=None) == INVALID
    assert call(h=None, nblocks=0) == INVALID                    # rs is checked first
    assert call(nblocks=0) == OK
    assert call(nblocks=0, shard_len=0, d=None, present=None, m=None, flags=64, device=-5) == OK    # nothing to do
    assert call(shard_len=0) == EMPTY
    assert call(shard_len=0, d=None, present=few, flags=64, device=-5) == EMPTY                     # before the rest
    assert call(d=None) == INVALID
    assert call(present=None) == INVALID
    assert call(m=None) == INVALID
    assert call(m=ctypes.c_void_p(0x300002)) == INVALID                                          # 4-byte aligned words
    for flags in (4, 8, -1, DATA_ONLY | NO_REBUILD | 16):
        assert call(flags=flags) == INVALID, flags
    assert call(flags=4, present=few, device=-5) == INVALID      # ... before the presence flags and the device
    assert call(m=None, present=few, device=-5) == INVALID
    assert call(present=few) == TOO_FEW_PRESENT
    assert call(present=few, device=-5) == TOO_FEW_PRESENT       # ... before the device
    assert call(present=few, flags=DATA_ONLY | NO_REBUILD, device=9999) == TOO_FEW_PRESENT
    # the device ID, as shmr_ec_reconstruct_batch_dev reports it (both refuse these before any device work)
    for device in (-1, 9999):
        want = L.shmr_ec_reconstruct_batch_dev(h, d, 64, 512, good.ctypes.data_as(u8p), 3, 64, 0, device, None)
        assert want == (NO_DEVICE if _no_gpu() else INVALID)
        for flags in (0, DATA_ONLY, NO_REBUILD, DATA_ONLY | NO_REBUILD):
            assert call(device=device, flags=flags) == want, (device, flags)
    if _no_gpu():
        assert call() == NO_DEVICE                               # well formed: no CPU fallback
        assert call(flags=NO_REBUILD) == NO_DEVICE
        assert _device_untouched()


def test_device_stats_gain_no_slot():
    assert len(shmr_amd.reed_solomon.DEVICE_COUNTERS) == 12
    header = open(_native._HERE + "/../include/shmr_ec.h").read()
    assert re.search(r"SHMR_EC_DEV_COUNTERS\s*=\s*12\b", header)
    out = (ctypes.c_uint64 * 13)(*([7] * 13))
    assert _native.lib().shmr_ec_device_stats(5, out, 13) == 0 and list(out) == [0] * 12 + [7]


def _check_plan(rs, m, k, p, pr):
    """The checked plan of pattern pr under every flag combination."""
    valid, surplus, absent = _split(pr, k)
    dec = O.mat_invert(m[valid])
    want_check = O.mat_mul(m[surplus], dec) if surplus else np.zeros((0, k), np.uint8)
    for data_only, rebuild in itertools.product((False, True), (True, False)):
        in_idx, out_idx, rows, n_store = rs.checked_plan(pr, data_only=data_only, rebuild=rebuild)
        assert in_idx == valid
        # stored rows: the reconstruct plan's, verbatim
        if rebuild and absent:
            r_in, r_out, r_rows = rs.reconstruct_plan(pr, data_only)
            assert r_in == valid
        else:                                                     # (all present: the reconstruct is a no-op)
            r_out, r_rows = [], np.zeros((0, k), np.uint8)
        assert n_store == len(r_out) and out_idx[:n_store] == r_out
        assert np.array_equal(rows[:n_store], r_rows), (pr, data_only, rebuild)
        if rebuild:
            assert r_out == [i for i in absent if i < k] + ([] if data_only else [i for i in absent if i >= k])
        # check rows: the surplus shards in ascending index, M[k + r] * Dec
        assert out_idx[n_store:] == surplus and all(i >= k for i in surplus)
        assert np.array_equal(rows[n_store:], want_check), (pr, data_only, rebuild)
        assert want_check.all(), "MDS: every coefficient of a check row is non-zero"
        if not absent:
            assert n_store == 0 and np.array_equal(rows, m[k:])      # Dec = I: the encode rows


@pytest.mark.parametrize("k,p,patterns", [
    (4, 2, [pr for pr in itertools.product((0, 1), repeat=6) if sum(pr) >= 4]),
    (8, 3, [pr for pr in _sample(8, 3, 60, 83) if sum(pr) >= 8]),
    (5, 6, [pr for pr in _sample(5, 6, 40, 56) if sum(pr) >= 5]),
    (4, 6, [pr for pr in _sample(4, 6, 40, 46) if sum(pr) >= 4]),
    (2, 34, [pr for pr in _sample(2, 34, 10, 234) if sum(pr) >= 2]),
], ids=lambda v: None if isinstance(v, list) else str(v))
def test_checked_plan_rows(k, p, patterns):
    rs = shmr_amd.ReedSolomon(k, p)
    m = O.build_matrix(k, k + p)
    assert np.array_equal(rs.matrix(), m)
    for pr in patterns:
        _check_plan(rs, m, k, p, list(pr))


def test_checked_plan_argument_checks():
    rs = shmr_amd.ReedSolomon(4, 2)
    with pytest.raises(shmr_amd.Error) as e:
        rs.checked_plan([1, 1, 1, 0, 0, 0])
    assert e.value.name == "TooFewShardsPresent"
    with pytest.raises(shmr_amd.Error) as e:
        rs.checked_plan([1] * 5)
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        rs.checked_plan([1] * 7)
    assert e.value.name == "TooManyShards"
    # exactly k present, nothing rebuilt: an empty plan
    in_idx, out_idx, rows, n_store = rs.checked_plan([1, 1, 0, 1, 0, 1], rebuild=False)
    assert (in_idx, out_idx, rows.shape, n_store) == ([0, 1, 3, 5], [], (0, 4), 0)


def test_python_batch_checks_precede_device_use():
    """reconstruct_checked_batch_dev applies reconstruct_batch_dev's tensor checks."""
    import torch
    rs = shmr_amd.ReedSolomon(4, 2)
    shards = torch.zeros((3, 6, 1024), dtype=torch.uint8)
    present = np.ones((3, 6), np.uint8)
    with pytest.raises(TypeError):
        rs.reconstruct_checked_batch_dev(shards.view(3, -1), present)
    with pytest.raises(shmr_amd.Error) as e:
        rs.reconstruct_checked_batch_dev(shards[:, :5], present[:, :5])
    assert e.value.name == "TooFewShards"
    with pytest.raises(shmr_amd.Error) as e:
        rs.reconstruct_checked_batch_dev(shards, present, shard_len=2048)
    assert e.value.name == "IncorrectShardSize"
    with pytest.raises(shmr_amd.Error) as e:
        rs.reconstruct_checked_batch_dev(shards, present, shard_len=0)
    assert e.value.name == "EmptyShard"
    with pytest.raises(ValueError):
        rs.reconstruct_checked_batch_dev(shards, present[:2])
    with pytest.raises(TypeError):                               # well formed, but pageable host memory
        rs.reconstruct_checked_batch_dev(shards, present)
