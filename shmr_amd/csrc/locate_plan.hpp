// Single-shard location (shmr_ec_locate_batch_dev): the ratio rows the locate
// kernel multiplies by, and the rule that turns a block's verify word and
// candidate bitmap into its answer.
// Host logic only, header-only (tests/test_locate_plan.py compiles it on the
// CPU); resolve() is also what the resolve kernel (gf_locate.hip) runs per block.
// Further down: degraded blocks, and two damaged shards per block (p >= 4).
//
// With the syndrome s = C * data ^ stored parity (p bytes per column) and only
// shard e damaged, s = H[:, e] * err in every column, H = [C | I_p]:
//  * parity shard k + r: only row r differs -- the verify word has exactly bit r;
//  * data shard j: every row differs, and s_r == q[r][j] * s_0 for every row r,
//    q[r][j] = C[r][j] / C[0][j].  The kernel tests rows 1 .. R-1 of the first
//    row group, R = min(p, 4).
#pragma once

#include <cstddef>
#include <cstdint>

#if defined(__HIP__)
#define SHMR_LOCATE_HD __attribute__((host)) __attribute__((device))
#else
#define SHMR_LOCATE_HD
#endif

namespace shmr {
namespace locate {

constexpr int32_t kClean = -1;   // SHMR_EC_LOCATE_CLEAN
constexpr int32_t kNone = -2;    // SHMR_EC_LOCATE_NONE
constexpr unsigned kMinParity = 2, kMaxParity = 32;   // one verify-word bit per parity row

// Parity rows the locate kernel tests (the first row group of a verify).
SHMR_LOCATE_HD inline unsigned rows_used(unsigned p) { return p < 4 ? p : 4; }
// Words of a block's candidate bitmap: bit t of word t / 32 is data shard t.
SHMR_LOCATE_HD inline unsigned bitmap_words(unsigned k) { return (k + 31) / 32; }
// The verify word of a block whose every parity row differs.
SHMR_LOCATE_HD inline uint32_t all_rows(unsigned p) { return p >= 32 ? 0xffffffffu : (1u << p) - 1u; }

// q[(r - 1) * k + j] = C[r][j] / C[0][j] for r = 1 .. R-1 (C: the parity rows,
// row-major, k columns; div(a, b), b != 0).  False when some C[0][j] is 0: the
// ratios do not exist (no code of this crate's matrix has one).
template <class Div>
bool ratio_rows(const uint8_t* C, unsigned k, unsigned R, Div div, uint8_t* q) {
    for (unsigned j = 0; j < k; ++j) {
        if (C[j] == 0) return false;
        for (unsigned r = 1; r < R; ++r) q[size_t(r - 1) * k + j] = div(C[size_t(r) * k + j], C[j]);
    }
    return true;
}

// A block's answer from its verify word and candidate bitmap (bitmap_words(k)
// words; bits at and above k are ignored): kClean, the damaged shard's index,
// or kNone.
SHMR_LOCATE_HD inline int32_t resolve(uint32_t word, const uint32_t* bitmap, unsigned k, unsigned p) {
    if (word == 0) return kClean;
    if ((word & (word - 1)) == 0) {   // one parity row: that parity shard
        unsigned r = 0;
        while (!((word >> r) & 1u)) ++r;
        return r < p ? int32_t(k + r) : kNone;
    }
    if (word != all_rows(p)) return kNone;
    int32_t found = kNone;
    for (unsigned t = 0; t < k; ++t) {
        if (!((bitmap[t >> 5] >> (t & 31)) & 1u)) continue;
        if (found != kNone) return kNone;   // a second candidate
        found = int32_t(t);
    }
    return found;
}

// ---- degraded blocks (shmr_ec_locate_checked_batch_dev) --------------------
// A block with absent shards is compared by its checked plan (gf256.hpp
// Codec::checked_plan): inputs in_idx[0 .. k), the first k present shards, and
// one compare row per surplus shard out_idx[0 .. s) in ascending index, rows
// D = M[surplus] * inv(M[inputs]).  The s surplus shards with the k inputs are
// an MDS code of their own, so the rule above carries over with D for C:
//  * surplus shard out_idx[r] damaged: only its row differs -- the word has
//    exactly its bit;
//  * input t damaged: every compared row differs (the word is the pattern's row
//    mask), and s_r == q[r][t] * s_0, q[r][t] = D[r][t] / D[0][t]
//    (ratio_rows over D; the kernel tests rows 1 .. R-1, R = rows_used(s)).
// One row cannot tell its own shard from an input: below s = 2 nothing is located.

// The bit of parity shard `shard` (>= k) in a verify / check word.
SHMR_LOCATE_HD inline unsigned row_bit(unsigned shard, unsigned k) { return shard - k < 31 ? shard - k : 31; }

// The word of a block whose every compared row differs (shmr_ec_checked_rows).
SHMR_LOCATE_HD inline uint32_t row_mask(const uint16_t* out_idx, unsigned s, unsigned k) {
    uint32_t mask = 0;
    for (unsigned r = 0; r < s; ++r) mask |= 1u << row_bit(out_idx[r], k);
    return mask;
}

// A degraded block's answer from its check word and candidate bitmap (bit t:
// plan input t; bits at and above k are ignored): kClean, a shard index in
// [0, total), or kNone.  s == 0 compares nothing: the word is 0 and the answer
// kClean, as the checked reconstruct reports such a block.  With every shard
// present (s = p >= 2, in_idx the identity, out_idx = k .. k+p-1) this is
// resolve() above, answer for answer.
SHMR_LOCATE_HD inline int32_t resolve_checked(uint32_t word, const uint32_t* bitmap, unsigned k, unsigned s,
                                              uint32_t mask, const uint16_t* in_idx, const uint16_t* out_idx) {
    if (word == 0) return kClean;
    if (s < 2) return kNone;
    if ((word & (word - 1)) == 0) {   // one compared row: that surplus shard
        for (unsigned r = 0; r < s; ++r)
            if (word == 1u << row_bit(out_idx[r], k)) return int32_t(out_idx[r]);
        return kNone;
    }
    if (word != mask) return kNone;
    int32_t found = kNone;
    for (unsigned t = 0; t < k; ++t) {
        if (!((bitmap[t >> 5] >> (t & 31)) & 1u)) continue;
        if (found != kNone) return kNone;   // a second candidate
        found = int32_t(in_idx[t]);
    }
    return found;
}

// ---- two damaged shards (shmr_ec_locate_pair_batch_dev) --------------------
// A code with p >= 4 has distance >= 5: it determines two damaged shards.  With
// H' = [C[0:4] | I_4] (the first row group, k + 4 columns, any four of them
// independent) and shards e, f damaged, s_G lies in span(H'_e, H'_f) in every
// column; a column where only e is hit is consistent with exactly the pairs
// that hold e, so the pairs consistent with every column are {e, f} alone once
// each of the two is hit somewhere.  The pair kernel (gf_locate.hip) tests:
//  * data shards a < b: rows 0, 1 fix the two error bytes (the 2x2 minor of C
//    is non-zero), rows 2, 3 must agree --
//      s_2 == al (x) s_0 ^ be (x) s_1,   s_3 == ga (x) s_0 ^ de (x) s_1;
//  * data shard a with parity shard k + r, r < 4: the three rows other than r
//    are proportional to C[.][a] -- for r != 0 the two of s_v == q[v][a] (x) s_0
//    with v != r, for r == 0 s_v == (C[v][a] / C[1][a]) (x) s_1, v = 2, 3;
//  * two parity shards leave a verify word of exactly two bits (a damaged data
//    shard makes at least p - 1 >= 3 rows differ): no kernel.
constexpr unsigned pair_min_parity = 4;   // the group's rows: 4 (rows_used)

// Candidates of a block: the data-data pairs (a, b), a < b, in lexicographic
// order, then the data-parity pairs (a, k + r) at a * 4 + r.
SHMR_LOCATE_HD constexpr unsigned pair_dd_count(unsigned k) { return k * (k - 1) / 2; }
SHMR_LOCATE_HD constexpr unsigned pair_count(unsigned k) { return pair_dd_count(k) + 4 * k; }
// Words of a block's pair bitmap: bit i of word i / 32 is candidate i.
SHMR_LOCATE_HD constexpr unsigned pair_bitmap_words(unsigned k) { return (pair_count(k) + 31) / 32; }
SHMR_LOCATE_HD constexpr unsigned pair_index_dd(unsigned a, unsigned b, unsigned k) {
    return a * k - a * (a + 1) / 2 + (b - a - 1);
}
SHMR_LOCATE_HD constexpr unsigned pair_index_dp(unsigned a, unsigned r, unsigned k) {
    return pair_dd_count(k) + a * 4 + r;
}
// The two shards of candidate i < pair_count(k), ascending.
SHMR_LOCATE_HD inline void pair_shards(unsigned i, unsigned k, int32_t* out) {
    if (i >= pair_dd_count(k)) {
        i -= pair_dd_count(k);
        out[0] = int32_t(i >> 2);
        out[1] = int32_t(k + (i & 3u));
        return;
    }
    unsigned a = 0;
    while (i >= k - 1 - a) i -= k - 1 - a++;
    out[0] = int32_t(a);
    out[1] = int32_t(a + 1 + i);
}

// Coefficients of a codec's candidates in pair-index order: four per data-data
// pair (al, be, ga, de), two per data-parity pair (ascending row v).
SHMR_LOCATE_HD constexpr unsigned pair_coeff_count(unsigned k) { return 4 * pair_dd_count(k) + 8 * k; }
// LDS of the pair kernel: the staged 4-row plan (gf_tile.hpp plan_lds_bytes(k, 4),
// restated here for the host; the launch compares the two), then one 32-byte
// perm table per coefficient.
constexpr unsigned pair_tab_off(unsigned k) { return (k * 4 * 32 + k * 8 + 4 * 8 + 15) & ~15u; }
constexpr unsigned pair_lds_bytes(unsigned k) { return pair_tab_off(k) + pair_coeff_count(k) * 32; }
constexpr unsigned pair_max_data_of(unsigned lds) {
    unsigned k = 1;
    while (pair_lds_bytes(k + 1) <= lds) ++k;
    return k;
}
// The largest k whose plan and tables fit 64 KiB of LDS.
constexpr unsigned pair_max_data = pair_max_data_of(64 * 1024);
static_assert(pair_max_data == 29, "64 k^2 + 192 k table bytes behind a 136 k + 32 byte plan");
SHMR_LOCATE_HD constexpr bool pair_supported(unsigned k, unsigned p) {
    return p >= pair_min_parity && p <= kMaxParity && k >= 1 && k <= pair_max_data;
}

// out[pair_coeff_count(k)] from the parity rows C (row-major, k columns, at
// least 4 rows).  False when a needed pivot is zero (a 2x2 minor of rows 0, 1,
// or an entry of those rows): no code of this crate's matrix has one.
template <class Mul, class Div>
bool pair_coeffs(const uint8_t* C, unsigned k, Mul mul, Div div, uint8_t* out) {
    auto c = [&](unsigned r, unsigned j) { return C[size_t(r) * k + j]; };
    for (unsigned a = 0; a < k; ++a)
        for (unsigned b = a + 1; b < k; ++b) {
            const uint8_t det = uint8_t(mul(c(0, a), c(1, b)) ^ mul(c(1, a), c(0, b)));
            if (det == 0) return false;
            for (unsigned v = 2; v < 4; ++v) {
                *out++ = div(uint8_t(mul(c(v, a), c(1, b)) ^ mul(c(v, b), c(1, a))), det);   // of s_0
                *out++ = div(uint8_t(mul(c(v, a), c(0, b)) ^ mul(c(v, b), c(0, a))), det);   // of s_1
            }
        }
    for (unsigned a = 0; a < k; ++a)
        for (unsigned r = 0; r < 4; ++r) {
            const unsigned base = r == 0 ? 1 : 0;
            if (c(base, a) == 0) return false;
            for (unsigned v = 0; v < 4; ++v)
                if (v != r && v != base) *out++ = div(c(v, a), c(base, a));
        }
    return true;
}

SHMR_LOCATE_HD inline unsigned bits_set(uint32_t w) {
    unsigned n = 0;
    for (; w; w &= w - 1) ++n;
    return n;
}

// Whether a block goes through the pair kernel: no single shard explains it, at
// least three rows differ, and every row beyond the group differs (a data shard
// in the pair makes every row differ).
SHMR_LOCATE_HD inline bool pair_listed(uint32_t word, int32_t single, unsigned p) {
    return single == kNone && bits_set(word) >= 3 && (word >> 4) == (all_rows(p) >> 4);
}

// A block's two answers from its verify word, its single-shard answer
// (resolve) and its pair bitmap (pair_bitmap_words(k) words; bits at and above
// pair_count(k) are ignored):
//  1. a single answer stands: (it, kClean) -- clean blocks and single shards
//     are exactly locate's;
//  2. two rows differ: those two parity shards;
//  3. a block that is not pair_listed: (kNone, kNone);
//  4. exactly one surviving candidate: its shards, ascending; else (kNone, kNone).
SHMR_LOCATE_HD inline void resolve_pair(uint32_t word, int32_t single, const uint32_t* bitmap, unsigned k, unsigned p,
                                        int32_t* out) {
    out[0] = single;
    out[1] = kClean;
    if (single != kNone) return;
    out[1] = kNone;
    if (bits_set(word) == 2) {
        unsigned r1 = 0;
        while (!((word >> r1) & 1u)) ++r1;
        unsigned r2 = r1 + 1;
        while (!((word >> r2) & 1u)) ++r2;
        if (r2 < p) {
            out[0] = int32_t(k + r1);
            out[1] = int32_t(k + r2);
        }
        return;
    }
    if (!pair_listed(word, single, p)) return;
    const unsigned n = pair_count(k);
    unsigned found = n;
    for (unsigned i = 0; i < n; ++i) {
        if (!((bitmap[i >> 5] >> (i & 31)) & 1u)) continue;
        if (found != n) return;   // a second candidate
        found = i;
    }
    if (found != n) pair_shards(found, k, out);
}

}  // namespace locate
}  // namespace shmr
