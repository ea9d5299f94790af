"""Repair of degraded blocks on the GPU (shmr_ec_reconstruct_repair_batch_dev):
locate the damaged survivor, rebuild the absent shards and the located one
from the good survivors, verify.  Bit-exact against the oracle's codewords;
the batches are laid out as in tests/test_gpu_locate_checked.py.
"""
import numpy as np
import pytest

from locate_checked_ref import CLEAN, NONE
from test_gpu_locate_checked import Batch, lost

pytestmark = pytest.mark.gpu


def _repair(batch):
    """-> (located, counts, the buffer after the call as a numpy image)."""
    import torch
    buf = torch.from_numpy(batch.img).to(batch.gpu)
    located, counts = batch.rs.reconstruct_repair_batch_dev(batch.dev_view(buf), batch.present, shard_len=batch.L)
    torch.cuda.synchronize()
    return located, counts, buf.cpu().numpy()


def _check_image(batch, after, whole, kept):
    """Blocks `whole` hold the oracle's codeword in every shard; blocks `kept`
    keep every present shard byte for byte; every byte outside [0, len) of a
    shard -- the pitch padding, the guards -- is untouched."""
    got, start, code = batch.view(after), batch.view(batch.img), batch.view(batch.codeword)
    L = batch.L
    for b in whole:
        assert np.array_equal(got[b, :, :L], code[b, :, :L]), f"block {b} is not its codeword"
    for b in kept:
        pr = batch.present[b] == 1
        assert np.array_equal(got[b, pr, :L], start[b, pr, :L]), f"a present shard of block {b} was written"
    assert np.array_equal(got[:, :, L:], start[:, :, L:]), "pitch padding was written"
    assert np.array_equal(after[:batch.off], batch.img[:batch.off]), "the front guard was written"
    end = batch.off + batch.B * batch.t * batch.pitch
    assert np.array_equal(after[end:], batch.img[end:]), "the rear guard was written"


@pytest.mark.parametrize("k,p,L", [(8, 3, 2 * 4096 + 83), (10, 4, 4096 + 40)])
def test_mixed_batch(gpu, k, p, L):
    t = k + p
    one = lost(t, 2)                                               # s = p - 1
    present = [one, one, np.ones(t, np.uint8), one, lost(t, k + 1), one, np.ones(t, np.uint8), lost(t, 0, 1),
               lost(t, 0), one]
    batch = Batch(k, p, L, present, gpu)
    batch.damage(1, 5, L - 1)                                      # an input
    batch.damage(3, t - 1, 100)                                    # a surplus shard
    batch.damage(4, 0, 4096)                                       # an input, a parity shard absent
    batch.damage(5, 1, 7)
    batch.damage(5, 6, 4000, x=0x2b)                               # two inputs, different columns
    batch.damage(6, 3, 2222)                                       # complete and damaged
    if p == 3:
        batch.damage(7, 4, 9)                                      # s = 1: seen, not located
    else:
        batch.damage(7, 4, 9)
        batch.damage(7, 9, 10, x=0x1f)                             # s = 2, two inputs
    batch.damage(9, k, 1)                                          # parity row 0: an input here
    located, counts, after = _repair(batch)
    want = [CLEAN, 5, CLEAN, t - 1, 0, NONE, 3, NONE, CLEAN, k]
    assert batch.expected().tolist() == want                       # the definition agrees
    assert located.tolist() == want
    assert counts == {"clean": 3, "repaired": 5, "not_repairable": 2}
    _check_image(batch, after, whole=[0, 1, 2, 3, 4, 6, 8, 9], kept=[5, 7])


def test_damage_beyond_the_first_row_group_is_demoted(gpu):
    """RS(6,6), one absent: an input plus the fifth surplus row.  Locate looks
    at four rows and names the input; the closing verify still differs, the
    block ends NONE and counts as not repairable."""
    k, p, t, L = 6, 6, 12, 4096 + 100
    pr = lost(t, 0)
    batch = Batch(k, p, L, [pr, pr, pr], gpu)
    batch.damage(0, 3, 50)
    batch.damage(0, 11, 4100, x=0x09)
    batch.damage(1, 3, 50)                                         # the input alone: repaired
    _, loc, _ = batch.run()
    assert loc.tolist() == [3, 3, CLEAN]
    located, counts, after = _repair(batch)
    assert located.tolist() == [NONE, 3, CLEAN]
    assert counts == {"clean": 1, "repaired": 1, "not_repairable": 1}
    _check_image(batch, after, whole=[1, 2], kept=[])
    # block 0: its absent shard and the named input were rebuilt from good
    # survivors, the damaged surplus shard is what is left
    got, code = batch.view(after), batch.view(batch.codeword)
    assert np.array_equal(got[0, :11, :L], code[0, :11, :L])
    assert np.flatnonzero(got[0, 11, :L] != code[0, 11, :L]).tolist() == [4100]
