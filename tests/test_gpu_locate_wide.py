"""Locate and scrub on the GPU past 32 shards, one wave, one launch and one
grid: the shapes tests/test_gpu_locate.py and tests/test_gpu_scrub.py (B = 5,
k <= 10, at most two full tiles) never reach.  The damage lists and the answers
their construction fixes are in tests/locate_cases.py;
tests/test_locate_wide_ref.py shows on the CPU that the numpy reference gives
the same.

Every locate test calls shmr_ec_locate_batch_dev through the guarded arrays of
test_gpu_locate.Case (sentinels next to d_mismatch and d_located, guards around
the scratch), compares `located` with the constructed answers for all blocks
and with locate_ref on the damaged blocks (at most 16), compares the words with
verify_batch_dev, and asserts that the shard buffer is unchanged.

 * words: RS(33,2), (40,3), (64,4), (70,5), B = 8 -- two and three bitmap words
   per block.  Block 0 untouched, 1 data shard 0, 2 shard 31, 3 shard 32, 4
   shard k-1, 5 parity shard k+p-1, 6 shards 5 and k-1 in different columns
   (different bitmap words, and with a full tile different launches: NONE),
   7 shard 32 at those two columns.  Blocks 1, 2 and 3 pin the word index and
   the per-block stride of the bitmap.
 * combine: RS(8,3), (40,3), (5,5) at two full tiles and a tail.  Shards a = 1
   and b (k-1; 3 for RS(5,5)) each damaged in its own column: in waves 0 and 3
   of one tile, in two tiles, in the full-tile and the partial-tile launch --
   NONE only if every wave's survivors are ANDed into the bitmap; all those
   columns in shard a alone (a); one byte per wave of tile 1 in four blocks;
   and the pairs again with b the parity shard k+1 (NONE for all three codes,
   RS(5,5) included: row 1 is inside the first row group the kernel tests).
   RS(40,3) once more at an odd byte offset, on the device's path and on the
   byte-granular kernel.
 * grid: RS(4,3), one full tile and a tail, B = grid + 37 blocks, so each of
   the two launches has more tiles than workgroups and workgroup w takes
   blocks w and w + grid: both damaged (plan staged once), only the second
   (first tile skipped, staged late), only the first.
 * preset: RS(3,2), len 16, B = grid * 256 + 3 one-word bitmaps, more than the
   preset grid has threads; the scratch holds zeros before the call, so a word
   the preset missed has no candidate left and gives NONE.
 * scrub on the damaged images of words RS(40,3), combine RS(8,3) and grid:
   answers, counts, the whole image (pristine, but NONE blocks as damaged), and
   a second scrub that repairs and writes nothing.
"""
import numpy as np
import pytest

import locate_cases as W
from locate_ref import CLEAN, NONE
from test_gpu_locate import Case, misaligned_path  # noqa: F401  (the fixture: device path and byte-granular kernel)

pytestmark = pytest.mark.gpu


def _grid():
    """Workgroups of a locate launch and of the preset launch at most."""
    import torch
    return 8 * torch.cuda.get_device_properties(0).multi_processor_count      # kLocateWgsPerCu in gf_locate.hip


def _same(got, want, what):
    bad = np.flatnonzero(np.asarray(got) != np.asarray(want))
    assert bad.size == 0, (f"{what}: {bad.size} blocks differ, first {int(bad[0])}: "
                           f"got {int(got[bad[0]])}, expected {int(want[bad[0]])}")


def _locate(c, damage, want, work_fill=W.SENT):
    c.load(c.damaged(damage))
    rc, words, located = c.locate(work_fill=work_fill)
    assert rc == 0
    blocks = W.damaged_blocks(damage)
    assert len(blocks) <= 16
    assert c.reference_of(c.img, blocks) == {b: int(want[b]) for b in blocks}, "the reference disagrees"
    _same(located, want, "located")
    verify = c.rs.verify_batch_dev(c.data, c.parity, shard_len=c.L).cpu().numpy().view(np.uint32)
    _same(words, verify, "words against verify_batch_dev")
    _same(words != 0, want != CLEAN, "non-zero words")
    c.unchanged()


def _scrub(c, damage, want):
    damaged = c.damaged(damage)
    c.load(damaged)
    located, counts = c.rs.scrub_batch_dev(c.data, c.parity, shard_len=c.L)
    assert located.dtype == np.int32
    _same(located, want, "located")
    clean, repaired, none = W.expected_counts(want)
    assert counts == (clean, repaired, none) and repaired > 0 and none > 0
    # pristine, the blocks reported NONE as they were damaged
    exp = c.pristine.copy()
    for dst, src in zip(c.regions(exp), c.regions(damaged)):
        dst[want == NONE] = src[want == NONE]

    def image_is_expected():
        bad = np.flatnonzero(c.buf.cpu().numpy() != exp)
        assert bad.size == 0, f"{bad.size} bytes differ from the expected image, first at {int(bad[0])}"
    image_is_expected()
    # a second scrub finds nothing to repair and writes nothing
    again, counts2 = c.rs.scrub_batch_dev(c.data, c.parity, shard_len=c.L)
    _same(again, np.where(want == NONE, NONE, CLEAN), "located by the second scrub")
    assert counts2 == (clean + repaired, 0, none)
    image_is_expected()


@pytest.mark.parametrize("L", W.WORDS_LENGTHS)
@pytest.mark.parametrize("k,p", W.WORDS_CODES)
def test_second_and_third_bitmap_word(gpu, k, p, L):
    c = Case(k, p, L, gpu, seed=k * 131 + L, nblk=W.WORDS_B)
    _locate(c, *W.words_case(k, p, L))


@pytest.mark.parametrize("k,p", W.COMBINE_CODES)
def test_survivors_combine_across_waves_tiles_and_launches(gpu, k, p):
    c = Case(k, p, W.COMBINE_L, gpu, seed=k + 17, nblk=W.COMBINE_B)
    _locate(c, *W.combine_case(k, p))


def test_survivors_combine_at_an_odd_byte_offset(gpu, misaligned_path):
    k, p = 40, 3
    c = Case(k, p, W.COMBINE_L, gpu, seed=k + 18, nblk=W.COMBINE_B, odd=True)
    assert c.data.data_ptr() % 2 == 1 and c.parity.data_ptr() % 2 == 1
    _locate(c, *W.combine_case(k, p))


def test_more_tiles_than_the_grid(gpu):
    k, p = W.GRID_CODE
    B, damage, want = W.grid_case(_grid())
    c = Case(k, p, W.GRID_L, gpu, seed=23, nblk=B)
    _locate(c, damage, want)


def test_preset_past_its_grid(gpu):
    k, p = W.PRESET_CODE
    B, damage, want = W.preset_case(_grid())
    c = Case(k, p, W.PRESET_L, gpu, seed=29, nblk=B, pitch=W.PRESET_L)
    _locate(c, damage, want, work_fill=0)


@pytest.mark.parametrize("L", W.WORDS_LENGTHS)
def test_scrub_second_bitmap_word(gpu, L):
    k, p = 40, 3
    c = Case(k, p, L, gpu, seed=k * 137 + L, nblk=W.WORDS_B)
    _scrub(c, *W.words_case(k, p, L))


def test_scrub_combined_survivors(gpu):
    k, p = 8, 3
    c = Case(k, p, W.COMBINE_L, gpu, seed=k + 19, nblk=W.COMBINE_B)
    _scrub(c, *W.combine_case(k, p))


def test_scrub_more_tiles_than_the_grid(gpu):
    """The pointer-table rebuild gets many hit blocks with different erasure
    patterns in one call."""
    k, p = W.GRID_CODE
    B, damage, want = W.grid_case(_grid())
    c = Case(k, p, W.GRID_L, gpu, seed=31, nblk=B)
    _scrub(c, damage, want)
