"""What the locate and scrub tests share, on the host only (no GPU use): the
guarded host image of a batch of codewords, and the damage lists of the wide
shapes with the answers their construction fixes.

Host image (HostCase), the layout of tests/test_gpu_verify.py: separate data
and parity regions in one buffer, guard bytes (0xC3) in front of, between and
behind them, and by default a shard pitch above len (rounded up to 64) whose
padding holds random bytes that are not a codeword; parity from
c_oracle.encode_batch.

Damage lists are [(block, shard, column, xor)].  The expected answers follow
from the construction, not from any code (tests/test_locate_wide_ref.py checks
that the numpy reference agrees):
 * one damaged shard e gives e;
 * two shards a != b, each damaged alone in its own column, give NONE for
   every p >= 2: any two columns of H = [C | I] are independent, so the column
   that only a damaged eliminates everybody but a, and the other column
   everybody but b.  The same holds when b is a parity shard k + r with r > 0
   inside the first row group: in b's column s_0 is zero and s_r is not, which
   no data shard explains;
 * an untouched block gives CLEAN with word 0.

The wide shapes (tests/test_gpu_locate_wide.py has the tables): `words_case`
more than one bitmap word per block, `combine_case` survivors combined across
waves, tiles and the two launches, `grid_case` more tiles than the locate grid,
`preset_case` more bitmap words than the preset grid has threads.
"""
import numpy as np

from locate_ref import CLEAN, NONE, locate_ref
from oracle import c_oracle

GUARD, SENT = 256, 0xC3
TILE = 4096                               # bytes of a shard one locate workgroup takes (256 lanes x 16)
WAVE = 1024                               # ... and one wave of it (64 lanes x 16)


def pitch_above(L):
    return (L // 64 + 1) * 64            # above len, a multiple of 64


class HostCase:
    """Codewords of one (k, p, L), nblk blocks, in the guarded two-region layout
    (a host image); `odd` puts both regions at an odd byte offset."""

    def __init__(self, k, p, L, seed, nblk=5, odd=False, pitch=None):
        self.k, self.p, self.L, self.B = k, p, L, nblk
        self.pitch = pitch = pitch_above(L) if pitch is None else pitch
        rng = np.random.default_rng(seed)
        B = nblk
        self.data_off = GUARD + (1 if odd else 0)
        self.par_off = self.data_off + B * k * pitch + GUARD
        total = self.par_off + B * p * pitch + GUARD
        img = np.full(total, SENT, np.uint8)
        d = img[self.data_off:self.data_off + B * k * pitch].reshape(B, k, pitch)
        q = img[self.par_off:self.par_off + B * p * pitch].reshape(B, p, pitch)
        d[:] = rng.integers(0, 256, d.shape, dtype=np.uint8)       # padding past len: random, not a codeword
        q[:] = rng.integers(0, 256, q.shape, dtype=np.uint8)
        par = np.zeros((B, p, L), np.uint8)
        c_oracle.encode_batch(k, p, np.ascontiguousarray(d[:, :, :L]), par, B, L, 8)
        q[:, :, :L] = par
        self.pristine = img
        self.rng = rng

    def regions(self, img):
        """(data [B, k, pitch], parity [B, p, pitch]) views of a host image."""
        B, k, p, pitch = self.B, self.k, self.p, self.pitch
        return (img[self.data_off:self.data_off + B * k * pitch].reshape(B, k, pitch),
                img[self.par_off:self.par_off + B * p * pitch].reshape(B, p, pitch))

    def damaged(self, damage):
        img = self.pristine.copy()
        d, q = self.regions(img)
        for b, s, col, x in damage:
            (d if s < self.k else q)[b, s if s < self.k else s - self.k, col] ^= x
        return img

    def reference_of(self, img, blocks):
        """{block: locate_ref of that block of a host image}."""
        d, q = self.regions(img)
        return {int(b): locate_ref(self.k, self.p, d[b, :, :self.L], q[b, :, :self.L]) for b in blocks}


def damaged_blocks(damage):
    return sorted({b for b, _, _, _ in damage})


def expected_counts(want):
    """scrub's (clean, repaired, not repairable) of the constructed answers."""
    want = np.asarray(want)
    return int((want == CLEAN).sum()), int((want >= 0).sum()), int((want == NONE).sum())


# ---- more than one bitmap word -----------------------------------------------------------
WORDS_CODES = [(33, 2), (40, 3), (64, 4), (70, 5)]
WORDS_LENGTHS = [1000, TILE + 48]
WORDS_B = 8


def words_case(k, p, L):
    """-> (damage, want [8]).  The two columns of blocks 6 and 7 are far apart:
    with a full tile, the first is in it and the second in the partial tile
    (the two launches)."""
    c1, c2 = 100, L - 9
    damage = [(1, 0, L // 2, 0x41),
              (2, 31, 3, 0x17),
              (3, 32, L - 1, 0xFF),
              (4, k - 1, 0, 0x5B),
              (5, k + p - 1, L // 3, 0x41),
              (6, 5, c1, 0x41), (6, k - 1, c2, 0x22),               # bits of different bitmap words
              (7, 32, c1, 0x9D), (7, 32, c2, 0x41)]
    return damage, np.array([CLEAN, 0, 31, 32, k - 1, k + p - 1, NONE, 32], np.int32)


# ---- survivors combined across waves, tiles and launches ---------------------------------
COMBINE_CODES = [(8, 3), (40, 3), (5, 5)]
COMBINE_L = 2 * TILE + 48                 # two full tiles and a tail
COMBINE_B = 12
# (column of shard a, column of shard b)
COMBINE_PAIRS = [(7, 3 * WAVE + 9),                       # waves 0 and 3 of tile 0
                 (7, TILE + 2 * WAVE + 5),                # two workgroups
                 (TILE + 100, 2 * TILE + 40)]             # the full-tile launch and the partial-tile launch


def combine_case(k, p):
    """-> (damage, want [12]).  Block 0 untouched; 1-3 the pairs with b a data
    shard; 4 every column of the pairs in shard a alone; 5-8 one byte in wave
    0, 1, 2, 3 of tile 1, each in another shard; 9-11 the pairs with b the
    parity shard k + 1."""
    a, b = 1, (3 if (k, p) == (5, 5) else k - 1)
    damage, want = [], np.full(COMBINE_B, CLEAN, np.int32)
    for i, (ca, cb) in enumerate(COMBINE_PAIRS):
        damage += [(1 + i, a, ca, 0x41), (1 + i, b, cb, 0x17)]
        want[1 + i] = NONE
    for col in sorted({c for pair in COMBINE_PAIRS for c in pair}):
        damage.append((4, a, col, 0x5B))
    want[4] = a
    for w, shard in enumerate([0, 2, k - 2, k - 1]):
        damage.append((5 + w, shard, TILE + w * WAVE + 33 * w + 1, 0x22 + w))
        want[5 + w] = shard
    for i, (ca, cb) in enumerate(COMBINE_PAIRS):
        damage += [(9 + i, a, ca, 0x41), (9 + i, k + 1, cb, 0x17)]
        want[9 + i] = NONE
    return damage, want


# ---- more tiles than the locate grid -----------------------------------------------------
GRID_CODE = (4, 3)
GRID_L = TILE + 16                        # one full tile and a tail: each launch has one tile per block


def grid_case(grid):
    """-> (B, damage, want [B]) for a locate grid of `grid` workgroups: B =
    grid + 37 blocks, so workgroup w takes blocks w and w + grid in each launch.

    The issue's table names block grid + 36 twice (it is B - 1, damaged in data
    shard 2 in the tail columns, and one of the pair "36 and grid + 36" of
    parity damage); the parity pair is at 35 and grid + 35 here, still both
    tiles of one workgroup."""
    k, p = GRID_CODE
    B = grid + 37
    damage = [(0, 1, 50, 0x41), (grid, 2, 1500, 0x17),              # both tiles of a workgroup damaged, staged once
              (grid + 5, 3, 2100, 0x5B),                            # first tile skipped, plan staged on the second
              (9, 0, 3300, 0x22),                                   # staged on the first tile, second tile clean
              (grid - 1, 0, 7, 0x9D),
              (grid + 1, k - 1, TILE - 1, 0xFF),
              (B - 1, 2, TILE + 5, 0x41),                           # in the tail columns
              (35, k + 1, 300, 0x41), (grid + 35, k + 2, TILE + 15, 0x33),
              (grid + 20, 0, 2000, 0x41), (grid + 20, 3, TILE + 2, 0x17)]
    want = np.full(B, CLEAN, np.int32)
    for b, s in [(0, 1), (grid, 2), (grid + 5, 3), (9, 0), (grid - 1, 0), (grid + 1, k - 1), (B - 1, 2),
                 (35, k + 1), (grid + 35, k + 2), (grid + 20, NONE)]:
        want[b] = s
    return B, damage, want


# ---- more bitmap words than the preset grid has threads ----------------------------------
PRESET_CODE = (3, 2)
PRESET_L = 16                             # pitch 16 too: no padding


def preset_case(grid):
    """-> (B, damage, want [B]): B = grid * 256 + 3 blocks of one bitmap word."""
    k, p = PRESET_CODE
    n = grid * 256
    B = n + 3
    damage = [(0, 1, 5, 0x41), (n - 1, 0, 0, 0x17), (n, 2, 15, 0x5B), (B - 1, 1, 9, 0x22), (1, k + 1, 3, 0x41)]
    want = np.full(B, CLEAN, np.int32)
    want[[0, n - 1, n, B - 1, 1]] = [1, 0, 2, 1, k + 1]
    return B, damage, want
