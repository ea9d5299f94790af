"""numpy reference of two-shard location (shmr_ec_locate_pair_batch_dev).

locate_pair_ref is written from the definition, not from the kernel's
shortcut: with the syndrome s = C (x) data ^ stored parity (p bytes per column)
and H = [C | I_p], shards e and f alone are damaged exactly when two error rows
x, y give s == H[:, e] (x) x ^ H[:, f] (x) y in every row and column.  It tries
every pair of the k + p shards against all p rows: x and y follow from two rows
whose 2x2 minor of (H_e, H_f) is non-singular, and the other rows must agree.

locate_pair_rule is the rule the library documents (include/shmr_ec.h,
locate_plan.hpp resolve_pair): the single answer and the pair candidates come
from the first group of four parity rows only, the other rows enter through the
verify word.

Outcomes, two per block: (-1, -1) a codeword; (e, -1) the one shard that
explains the syndromes; (e, f), e < f, the one pair that does; (-2, -2).
"""
import itertools

import numpy as np

from locate_ref import CLEAN, NONE, _mul, locate_ref, syndromes
from oracle import rs_oracle as O

GROUP = 4                                   # parity rows the pair tests read


def _parity_check(k, p):
    C = O.ReedSolomon(k, p).parity_rows()
    return np.concatenate([C, np.eye(p, dtype=np.uint8)], axis=1)       # [p, k + p]


def _explains(s, he, hf):
    """Whether s lies in span(he, hf) in every column (he, hf: columns of H over
    the rows of s)."""
    n = len(he)
    for r0, r1 in itertools.combinations(range(n), 2):
        det = O.gal_mul(int(he[r0]), int(hf[r1])) ^ O.gal_mul(int(he[r1]), int(hf[r0]))
        if det:
            break
    else:
        return False                        # dependent columns: no code here has them
    inv = O.gal_div(1, det)
    x = _mul(inv, _mul(hf[r1], s[r0]) ^ _mul(hf[r0], s[r1]))
    y = _mul(inv, _mul(he[r1], s[r0]) ^ _mul(he[r0], s[r1]))
    return all(np.array_equal(s[r], _mul(he[r], x) ^ _mul(hf[r], y)) for r in range(n))


def locate_pair_ref(k, p, data, parity):
    """The definition, over all k + p shards and all p rows."""
    single = locate_ref(k, p, data, parity)
    if single != NONE:
        return single, CLEAN
    H = _parity_check(k, p)
    s = syndromes(k, p, data, parity)
    found = [(e, f) for e, f in itertools.combinations(range(k + p), 2) if _explains(s, H[:, e], H[:, f])]
    return found[0] if len(found) == 1 else (NONE, NONE)


def verify_word(s):
    return sum(1 << min(r, 31) for r in range(len(s)) if s[r].any())


def locate_rule(k, p, s):
    """shmr_ec_locate_batch_dev's answer from the syndromes: data shards are told
    apart by the first min(p, 4) rows only."""
    C = O.ReedSolomon(k, p).parity_rows()
    word = verify_word(s)
    if word == 0:
        return CLEAN
    if word & (word - 1) == 0:
        return k + word.bit_length() - 1
    if word != (1 << p) - 1:
        return NONE
    R = min(p, GROUP)
    found = [j for j in range(k)
             if all(np.array_equal(s[r], _mul(O.gal_div(int(C[r][j]), int(C[0][j])), s[0])) for r in range(1, R))]
    return found[0] if len(found) == 1 else NONE


def locate_pair_rule(k, p, data, parity):
    """The first-group rule (needs p >= 4)."""
    s = syndromes(k, p, data, parity)
    word = verify_word(s)
    single = locate_rule(k, p, s)
    if single != NONE:
        return single, CLEAN
    rows = [r for r in range(p) if (word >> r) & 1]
    if len(rows) == 2:
        return k + rows[0], k + rows[1]
    if len(rows) < 3 or any(r not in rows for r in range(GROUP, p)):
        return NONE, NONE
    H = _parity_check(k, p)[:GROUP, :k + GROUP]
    g = s[:GROUP]
    found = [(e, f) for e, f in itertools.combinations(range(k + GROUP), 2)
             if e < k and _explains(g, H[:, e], H[:, f])]
    return found[0] if len(found) == 1 else (NONE, NONE)


def pair_index(k, e, f):
    """The fixed candidate index of the pair e < f (e a data shard, f a data
    shard or one of the parity shards k .. k + 3)."""
    if f < k:
        return e * k - e * (e + 1) // 2 + (f - e - 1)
    return k * (k - 1) // 2 + e * 4 + (f - k)


def pair_coeffs_ref(k, p):
    """(dd [k (k - 1) / 2, 4], dp [k, 4, 2]) from the oracle's matrix: per
    data-data pair the coefficients of s_2 == c0 s_0 ^ c1 s_1 and
    s_3 == c2 s_0 ^ c3 s_1, per (a, r) the ratios of the two rows other than r
    and the base row against the base row (row 0, or row 1 for r == 0)."""
    C = O.ReedSolomon(k, p).parity_rows()
    mul, div = O.gal_mul, O.gal_div
    dd = []
    for a, b in itertools.combinations(range(k), 2):
        ca, cb = [int(C[r][a]) for r in range(4)], [int(C[r][b]) for r in range(4)]
        det = mul(ca[0], cb[1]) ^ mul(ca[1], cb[0])
        assert det != 0
        row = []
        for v in (2, 3):
            # s_v = ca[v] x ^ cb[v] y with (x, y) solved from rows 0, 1
            row += [div(mul(ca[v], cb[1]) ^ mul(cb[v], ca[1]), det), div(mul(ca[v], cb[0]) ^ mul(cb[v], ca[0]), det)]
        dd.append(row)
    dp = np.zeros((k, 4, 2), np.uint8)
    for a in range(k):
        for r in range(4):
            base = 1 if r == 0 else 0
            dp[a, r] = [div(int(C[v][a]), int(C[base][a])) for v in range(4) if v not in (r, base)]
    return np.array(dd, np.uint8).reshape(len(dd), 4), dp
