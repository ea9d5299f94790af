"""The whole scrub on the GPU (shmr_ec_scrub_batch_dev: locate, rebuild the
located shard through the reconstruct kernels, verify again) on the cases of
tests/test_gpu_locate.py, through scrub_batch_dev and scrub_shards_dev:
afterwards every block with one damaged shard equals the pristine codeword
byte for byte, a block that is not locatable is left exactly as it was, and
guards and padding are untouched.
"""
import numpy as np
import pytest

import shmr_amd
from locate_ref import CLEAN, NONE
from test_gpu_locate import B, CODES, LENGTHS, Case, damage_of

pytestmark = pytest.mark.gpu


def _expected_image(c, damaged, located):
    """The pristine image, with the blocks reported NONE as they were damaged."""
    want = c.pristine.copy()
    wd, wq = c.regions(want)
    dd, dq = c.regions(damaged)
    for b in range(B):
        if located[b] == NONE:
            wd[b], wq[b] = dd[b], dq[b]
    return want


def _check_scrubbed(c, damaged, located, counts, want):
    p = c.p
    assert located.dtype == np.int32 and located.tolist() == want
    assert counts == ((1, 3, 1) if p >= 3 else (1, 4, 0))
    got = c.buf.cpu().numpy()
    exp = _expected_image(c, damaged, located)
    bad = np.flatnonzero(got != exp)
    assert bad.size == 0, f"{bad.size} bytes differ from the expected image, first at {int(bad[0])}"
    words = c.rs.verify_batch_dev(c.data, c.parity, shard_len=c.L).cpu().numpy().view(np.uint32)
    assert not words[:4].any() and (words[4] != 0) == (p >= 3), words


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", CODES)
def test_damage_table(gpu, k, p, L):
    c = Case(k, p, L, gpu, seed=(k * 64 + p) * 11 + L)
    damage, want = damage_of(k, p, L)
    damaged = c.damaged(damage)
    c.load(damaged)
    located, counts = c.rs.scrub_batch_dev(c.data, c.parity, shard_len=L)
    _check_scrubbed(c, damaged, located, counts, want)
    # a second scrub finds nothing to repair and writes nothing
    again, counts2 = c.rs.scrub_batch_dev(c.data, c.parity, shard_len=L)
    assert again.tolist() == [CLEAN] * 4 + [want[4] if p >= 3 else CLEAN]
    assert counts2 == ((4, 0, 1) if p >= 3 else (5, 0, 0))
    assert np.array_equal(c.buf.cpu().numpy(), _expected_image(c, damaged, located))


@pytest.mark.parametrize("L", LENGTHS)
@pytest.mark.parametrize("k,p", CODES)
def test_combined_tensor_form(gpu, k, p, L):
    """scrub_shards_dev: one [B, k + p, pitch] tensor, both regions in it."""
    import torch
    c = Case(k, p, L, gpu, seed=31 + k)
    damage, want = damage_of(k, p, L)
    d, q = c.regions(c.damaged(damage))
    host = np.concatenate([d, q], axis=1)                       # [B, k + p, pitch], padding included
    shards = torch.from_numpy(host.copy()).to(gpu)
    located, counts = c.rs.scrub_shards_dev(shards, shard_len=L)
    assert located.tolist() == want and counts == ((1, 3, 1) if p >= 3 else (1, 4, 0))
    pd, pq = c.regions(c.pristine)
    exp = np.concatenate([pd, pq], axis=1)
    if p >= 3:
        exp[4] = host[4]
    assert np.array_equal(shards.cpu().numpy(), exp)


def test_damage_beyond_the_first_row_group_is_demoted(gpu):
    """RS(5,5): one data shard and parity row 4 damaged.  Locate looks at rows
    0-3 and names the data shard; the closing verify still sees row 4, so the
    block is reported not repairable (its data shard has been rebuilt)."""
    k, p, L = 5, 5, 1000
    c = Case(k, p, L, gpu, seed=57)
    damaged = c.damaged([(1, 2, 17, 0x41), (1, k + 4, 900, 0x41), (3, k + 4, 5, 0x22)])
    c.load(damaged)
    _, located = c.rs.locate_batch_dev(c.data, c.parity, shard_len=L)
    assert located.cpu().numpy().tolist() == [CLEAN, 2, CLEAN, k + 4, CLEAN]
    located, counts = c.rs.scrub_batch_dev(c.data, c.parity, shard_len=L)
    assert located.tolist() == [CLEAN, NONE, CLEAN, k + 4, CLEAN] and counts == (3, 1, 1)
    words = c.rs.verify_batch_dev(c.data, c.parity, shard_len=L).cpu().numpy().view(np.uint32)
    assert words.tolist() == [0, 1 << 4, 0, 0, 0]
    # the data shard was rebuilt, the parity row is as it was damaged
    exp = c.damaged([(1, k + 4, 900, 0x41)])
    assert np.array_equal(c.buf.cpu().numpy(), exp)


def test_refused_and_empty(gpu):
    import torch
    one = shmr_amd.ReedSolomon(4, 1)
    data = torch.zeros((B, 4, 64), dtype=torch.uint8, device=gpu)
    parity = torch.zeros((B, 1, 64), dtype=torch.uint8, device=gpu)
    with pytest.raises(shmr_amd.Error) as e:
        one.scrub_batch_dev(data, parity)
    assert e.value.name == "InvalidArgument"
    rs = shmr_amd.ReedSolomon(4, 2)
    located, counts = rs.scrub_batch_dev(data[:0], torch.zeros((0, 2, 64), dtype=torch.uint8, device=gpu))
    assert located.shape == (0,) and counts == (0, 0, 0)
    # all-zero shards are codewords
    located, counts = rs.scrub_batch_dev(data, torch.zeros((B, 2, 64), dtype=torch.uint8, device=gpu))
    assert located.tolist() == [CLEAN] * B and counts == (B, 0, 0)
