// Single-shard location (shmr_ec_locate_batch_dev): the ratio rows the locate
// kernel multiplies by, and the rule that turns a block's verify word and
// candidate bitmap into its answer.
// Host logic only, header-only (tests/test_locate_plan.py compiles it on the
// CPU); resolve() is also what the resolve kernel (gf_locate.hip) runs per block.
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

}  // namespace locate
}  // namespace shmr
