"""The four legs of the single-block host calls (shmr_ec_encode,
shmr_ec_reconstruct with and without data_only), each driven on purpose and
checked byte for byte against the CPU oracle:

  coalesced  mapped shards, knob coalesce=1: through the submission queue
  mapped     mapped shards: coded in place by one zero-copy launch
  bounced    pageable shards within bounce_kib: one bounce, one launch
  staged     pageable shards, bounce_kib=0: per-shard DMA into device staging

and shmr_ec_verify, which takes the staged leg alone.  The counters tell the
legs apart: zero-copy blocks and queue requests for the first two; the last two
both count a staged block and no queue request, and which of them runs is what
bounce_kib decides.  Shard length 4096 + 17: one full 4 KiB tile and a partial
one, no multiple of 16.  Lost: the first data shard and the last parity shard.
"""
import ctypes

import numpy as np
import pytest

import shmr_amd
from oracle import c_oracle

pytestmark = pytest.mark.gpu

L = 4096 + 17
U8P = ctypes.POINTER(ctypes.c_uint8)
LEGS = {   # leg -> (mapped shards, knobs, (zero-copy blocks, staged blocks, queue requests) per call)
    "coalesced": (True, {"coalesce": 1}, (1, 0, 1)),
    "mapped": (True, {}, (1, 0, 0)),
    "bounced": (False, {"bounce_kib": 65536}, (0, 1, 0)),
    "staged": (False, {"bounce_kib": 0}, (0, 1, 0)),
}


@pytest.fixture(scope="module")
def codewords():
    """(k, p) -> [k + p, L] codeword of the oracle (read-only)."""
    out = {}
    for k, p in ((3, 2), (5, 5)):
        rng = np.random.default_rng([k, p, L])
        sh = [rng.integers(0, 256, L, dtype=np.uint8) for _ in range(k)] + [np.zeros(L, np.uint8) for _ in range(p)]
        c_oracle.encode(k, p, sh)
        out[k, p] = np.stack(sh)
        out[k, p].flags.writeable = False
    return out


def _moved():
    z, s = shmr_amd.path_stats()
    return np.array([z, s, shmr_amd.queue_stats(0)["requests"]])


def _call(rs, arr, present=None, data_only=0):
    t = arr.shape[0]
    ptrs = (U8P * t)(*[arr[i].ctypes.data_as(U8P) for i in range(t)])
    lens = (ctypes.c_size_t * t)(*([L] * t))
    before = _moved()
    if present is None:
        rc = rs._L.shmr_ec_encode(rs._h, ptrs, lens, t)
    else:
        rc = rs._L.shmr_ec_reconstruct(rs._h, ptrs, lens, present.ctypes.data_as(U8P), t, data_only)
    assert rc == 0
    return tuple(_moved() - before)


@pytest.mark.parametrize("k,p", [(3, 2), (5, 5)])
@pytest.mark.parametrize("leg", list(LEGS))
def test_single_block_leg(gpu, codewords, leg, k, p):
    mapped, knobs, want_moved = LEGS[leg]
    t, full = k + p, codewords[k, p]
    rs = shmr_amd.ReedSolomon(k, p)
    buf = shmr_amd.PinnedBuffer(t * L) if mapped else None
    arr = buf.array.reshape(t, L) if mapped else np.empty((t, L), np.uint8)
    present = np.ones(t, np.uint8)
    present[[0, t - 1]] = 0
    shmr_amd.set_tuning(**knobs)
    try:
        arr[:k], arr[k:] = full[:k], 0xEE
        assert _call(rs, arr) == want_moved
        assert np.array_equal(arr, full)
        arr[[0, t - 1]] = 0xEE
        assert _call(rs, arr, present) == want_moved
        assert np.array_equal(arr, full)
        arr[[0, t - 1]] = 0xEE
        assert _call(rs, arr, present, data_only=1) == want_moved
        assert np.array_equal(arr[:t - 1], full[:t - 1]) and (arr[t - 1] == 0xEE).all()   # absent parity untouched
    finally:
        shmr_amd.set_tuning(**{name: -2 for name in knobs})
        del arr
        buf = None


@pytest.mark.parametrize("k,p", [(3, 2), (5, 5)])
def test_verify_takes_the_staged_leg(gpu, codewords, k, p):
    """A codeword, and a copy with the last byte of the last parity shard
    flipped: one block verified per call, no host path counted, no request."""
    rs = shmr_amd.ReedSolomon(k, p)
    shards = [s.copy() for s in codewords[k, p]]
    for flip, want in ((0, True), (0xFF, False)):
        shards[-1][-1] ^= flip
        before, v0 = _moved(), shmr_amd.device_stats(0)["blocks_verified"]
        assert rs.verify(shards) is want
        assert tuple(_moved() - before) == (0, 0, 0)
        assert shmr_amd.device_stats(0)["blocks_verified"] - v0 == 1
