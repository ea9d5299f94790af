"""The numpy reference of single-shard location (tests/locate_ref.py) on
oracle codewords: the GPU tests (test_gpu_locate.py, test_gpu_scrub.py) compare
the kernels against it, so it is checked here against what was damaged.
"""
import numpy as np
import pytest

from locate_ref import CLEAN, NONE, locate_ref, syndromes
from oracle import rs_oracle as O

CODES = [(2, 2), (4, 2), (8, 3), (10, 4), (5, 5), (3, 9)]
L = 48


def _codeword(k, p, seed):
    rng = np.random.default_rng(seed)
    shards = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(p)]
    O.ReedSolomon(k, p).encode(shards)
    return np.stack(shards), rng


def _damage(cw, shard, cols, rng):
    """XOR non-zero bytes into the columns of one shard."""
    out = cw.copy()
    out[shard, cols] ^= rng.integers(1, 256, len(cols), dtype=np.uint8)
    return out


@pytest.mark.parametrize("k,p", CODES)
def test_clean_codeword(k, p):
    cw, _ = _codeword(k, p, 1)
    assert not syndromes(k, p, cw[:k], cw[k:]).any()
    assert locate_ref(k, p, cw[:k], cw[k:]) == CLEAN


@pytest.mark.parametrize("k,p", CODES)
def test_every_shard_is_found(k, p):
    """One byte, several bytes, every byte of each of the k + p shards."""
    cw, rng = _codeword(k, p, 2)
    for shard in range(k + p):
        for cols in ([0], [L - 1], [3, 17, 18, L - 1], list(range(L))):
            bad = _damage(cw, shard, cols, rng)
            assert locate_ref(k, p, bad[:k], bad[k:]) == shard, (shard, cols)


@pytest.mark.parametrize("k,p", [c for c in CODES if c[1] >= 3])
def test_two_damaged_shards_are_not_locatable(k, p):
    """p >= 3: three columns of H are independent, so damage in two shards never
    passes for damage in one -- same column or different columns."""
    cw, rng = _codeword(k, p, 3)
    t = k + p
    pairs = [(0, 1), (0, k), (k - 1, t - 1), (k, k + 1), (k, t - 1)]
    for a, b in pairs:
        for ca, cb in (([5], [5]), ([5], [6]), (list(range(L)), [0])):
            bad = _damage(_damage(cw, a, ca, rng), b, cb, rng)
            assert locate_ref(k, p, bad[:k], bad[k:]) == NONE, (a, b, ca, cb)


def test_syndrome_of_one_data_byte():
    """A data byte err in shard j leaves s_r = C[r][j] (x) err in its column and
    nothing elsewhere: what the kernel's ratio test rests on."""
    k, p = 8, 3
    cw, _ = _codeword(k, p, 4)
    C = O.ReedSolomon(k, p).parity_rows()
    bad = cw.copy()
    bad[5, 7] ^= 0x5B
    s = syndromes(k, p, bad[:k], bad[k:])
    assert [int(s[r, 7]) for r in range(p)] == [O.gal_mul(int(C[r][5]), 0x5B) for r in range(p)]
    s[:, 7] = 0
    assert not s.any()
