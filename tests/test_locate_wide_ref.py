"""The constructed answers of the wide locate shapes (tests/locate_cases.py)
against the numpy reference tests/locate_ref.py, on the CPU: the reference
alone passes what tests/test_gpu_locate_wide.py demands of the kernels.

For every case the damaged blocks must come out as constructed and one
untouched block as CLEAN.  The grid-dependent cases are built for a locate grid
of 2048 workgroups (8 per CU of a 256-CU device), as the GPU tests build them
there.
"""
import pytest

import locate_cases as W
from locate_ref import CLEAN, NONE

GRID = 8 * 256


def _agree(hc, damage, want, untouched):
    img = hc.damaged(damage)
    blocks = W.damaged_blocks(damage)
    assert want[untouched] == CLEAN and untouched not in blocks
    assert all(want[b] != CLEAN for b in blocks)
    assert (want != CLEAN).sum() == len(blocks), "an expected answer without damage"
    ref = hc.reference_of(img, blocks + [untouched])
    assert ref == {**{b: int(want[b]) for b in blocks}, untouched: CLEAN}


@pytest.mark.parametrize("L", W.WORDS_LENGTHS)
@pytest.mark.parametrize("k,p", W.WORDS_CODES)
def test_words_case(k, p, L):
    damage, want = W.words_case(k, p, L)
    _agree(W.HostCase(k, p, L, seed=k * 131 + L, nblk=W.WORDS_B), damage, want, 0)


@pytest.mark.parametrize("k,p", W.COMBINE_CODES)
def test_combine_case(k, p):
    """Blocks 9-11 (shard a and the parity shard k + 1 in different columns) are
    NONE for every code, RS(5,5) included: the reference tests all p rows, the
    kernel the first four, and row 1 is among both."""
    damage, want = W.combine_case(k, p)
    assert want[9:12].tolist() == [NONE] * 3
    _agree(W.HostCase(k, p, W.COMBINE_L, seed=k + 17, nblk=W.COMBINE_B), damage, want, 0)


def test_grid_case():
    k, p = W.GRID_CODE
    B, damage, want = W.grid_case(GRID)
    assert B == GRID + 37 and want.shape == (B,)
    _agree(W.HostCase(k, p, W.GRID_L, seed=23, nblk=B), damage, want, GRID + 9)


def test_preset_case():
    k, p = W.PRESET_CODE
    B, damage, want = W.preset_case(GRID)
    assert B == GRID * 256 + 3 and want.shape == (B,)
    _agree(W.HostCase(k, p, W.PRESET_L, seed=29, nblk=B, pitch=W.PRESET_L), damage, want, B - 2)
