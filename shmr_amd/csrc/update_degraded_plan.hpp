// Parity delta update of degraded blocks (shmr_ec_update_degraded_batch_dev):
// what the call adds to update_plan.hpp -- the presence check, the piece table
// entry and the table chunks.  The update list, its range and intersection
// checks, the pieces and the rounds are update::plan's, unchanged.  Host logic
// only, header-only and CPU-compilable; the piece table entry is also what the
// kernel (gf_update_degraded.hip) reads.
//
// The code is linear and column-wise.  Writing `new` over columns [a, b) of
// data shard j changes every parity row r by C[r][j] (x) (old ^ new) there:
//
//  * shard j present: old is its stored bytes, which `new` replaces;
//  * shard j absent: old[col] = sum_t D[j][t] (x) input_t[col], the row of the
//    pattern's data-only reconstruct plan that the ranged read evaluates
//    (read_plan.hpp), its inputs the first k present shards.  Slot j is not
//    touched.
//
// Either way the delta goes into the PRESENT parity rows only: what is XORed
// into the survivors is the punctured codeword of the delta, so they stay the
// punctured codeword of the new data plus whatever damage they carried.
//
//  * Footprint rule: BYTE-EXACT, as update_plan.hpp -- bytes [a, b) of shard j
//    (if present) and of the present parity shards of the block, nothing wider;
//    absent slots are neither read nor written.
//  * Rounds: update::plan's.  A rebuild piece reads columns [a, b) of the k
//    inputs and stores columns [a, b) of the present parity rows: pieces of one
//    block with disjoint columns touch disjoint bytes, whatever their shards and
//    whether those are present, so the column rule holds as it stands.  Every
//    round leaves the survivors a punctured codeword (plus the damage), so the
//    order of the rounds does not matter.
//  * Present parity rows: a list per pattern (a row index each), not a mask --
//    parity may be up to 255 rows.  DevPiece::rows is the device address of the
//    pattern's list image (gf256.hpp Codec::parity_rows_plan).
//  * Chunks: the piece table travels in chunks of at most kTablePieces entries
//    (one slot of the upload ring); behind each chunk one launch per round
//    present in it.
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "piece_plan.hpp"
#include "update_plan.hpp"

namespace shmr {
namespace degraded {

using namespace piece;

constexpr uint32_t kRebuildFlag = 1u << 30;   // DevPiece::shard: the shard is absent
constexpr uint32_t kRowShift = 16;            // DevPiece::shard: the shard's row of the plan image, from this bit
constexpr uint32_t kShardMask = (1u << kRowShift) - 1;
constexpr uint32_t kRowMask = (kRebuildFlag - 1) >> kRowShift;

// One piece as the kernel reads it (48 bytes, scalar dword loads).
struct DevPiece {
    uint64_t col, src;
    uint64_t plan;    // rebuild pieces: device address of the pattern's data-only reconstruct plan image
    uint64_t rows;    // device address of the pattern's present parity rows: [u32 0][u32 n][u16 row[n]]
    uint32_t block, len;
    uint32_t shard;   // the data shard | its plan row << kRowShift (rebuild) | kVecFlag | kRebuildFlag
    uint32_t tile0;   // tiles of the table's pieces in front of this one
};
static_assert(sizeof(DevPiece) == 48, "the kernel indexes the table in 12-dword entries");
constexpr uint32_t kPieceWords = sizeof(DevPiece) / 4;
constexpr size_t kTablePieces = kSlotBytes / sizeof(DevPiece);

inline uint32_t pack_shard(uint32_t shard, uint32_t row, bool rebuild) {
    return shard | (rebuild ? (row << kRowShift) | kRebuildFlag : 0u);
}

// Whether every block, updated or not, has at least k of its t shards present
// (any non-zero flag is "present", as for the reconstruct).
inline bool enough_present(const uint8_t* present, uint64_t nblocks, unsigned k, unsigned t) {
    for (uint64_t b = 0; b < nblocks; ++b) {
        unsigned np = 0;
        for (unsigned i = 0; i < t; ++i) np += present[b * t + i] ? 1 : 0;
        if (np < k) return false;
    }
    return true;
}

// The table chunks of the pieces of an update::Plan (ascending round).
inline uint32_t count_chunks(const std::vector<Piece>& ps) {
    uint32_t n = 0;
    for (size_t c0 = 0; c0 < ps.size(); c0 += chunk_pieces<DevPiece>(ps, c0)) ++n;
    return n;
}

}  // namespace degraded
}  // namespace shmr
