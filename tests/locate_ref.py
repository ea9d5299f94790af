"""numpy reference of single-shard location (shmr_ec_locate_batch_dev), written
from the definition and not from the kernel's shortcut.

With the syndrome s = C (x) data ^ stored parity (p bytes per column) and
H = [C | I_p], shard e alone is damaged exactly when some error row `err`
(one byte per column, not all zero) gives s == H[:, e] (x) err in every row
and column.  locate_ref tries every one of the k + p shards against all p
rows: the error row a shard would need follows from one syndrome row, and the
other rows must then agree.

Outcomes, as include/shmr_ec.h: -1 a codeword, the index of the one shard that
explains the syndromes, -2 none does (or more than one would).
"""
import numpy as np

from oracle import rs_oracle as O

CLEAN, NONE = -1, -2


def _mul(c, row):
    """gal_mul(c, b) for every byte b of row (the table gal_mul reads)."""
    return O.MUL_TABLE[int(c)][row]


def syndromes(k, p, data, parity):
    """s [p, L] of data [k, L] and stored parity [p, L]."""
    C = O.ReedSolomon(k, p).parity_rows()
    s = np.array(parity, dtype=np.uint8, copy=True)
    for r in range(p):
        for j in range(k):
            s[r] ^= _mul(C[r][j], np.asarray(data[j], dtype=np.uint8))
    return s


def locate_ref(k, p, data, parity) -> int:
    C = O.ReedSolomon(k, p).parity_rows()
    H = np.concatenate([C, np.eye(p, dtype=np.uint8)], axis=1)       # [p, k + p]
    s = syndromes(k, p, data, parity)
    if not s.any():
        return CLEAN
    found = []
    for e in range(k + p):
        col = H[:, e]
        r0 = int(np.flatnonzero(col)[0])                              # a row that sees shard e
        inv = O.gal_div(1, int(col[r0]))
        err = _mul(inv, s[r0])                                        # what the damage would have to be
        if all(np.array_equal(s[r], _mul(col[r], err)) for r in range(p)):
            found.append(e)
    return found[0] if len(found) == 1 else NONE
