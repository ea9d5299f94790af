// Ranged reads from device-resident blocks (shmr_ec_read_batch_dev): validation
// of a read list, its split into kernel pieces, and the table chunks the pieces
// upload in.  Host logic only, header-only (tests/test_read_plan.py compiles it
// on the CPU through tools/read_plan_check.cpp); the piece table entry and the
// tile search are also what the kernel (gf_read.hip) reads and runs.
//
// The code is column-wise: column c of an absent data shard is
// sum_t D[shard][t] (x) input_t[c], D the data-only reconstruct plan of the
// block's presence pattern, so bytes [offset, offset + len) of the shard need
// those columns of the k inputs and nothing else.  A present shard is copied.
//
//  * Footprint rule: BYTE-EXACT.  A request writes d_dst[dst_offset,
//    dst_offset + len) and nothing wider: interior chunks are whole 16-byte
//    stores inside the range, edge chunks are stored byte by byte.  Nothing of
//    the shards is written, so there are no hazards between requests and no
//    rounds (update_plan.hpp has them): two requests may read the same bytes.
//    Two requests must not write the same destination byte.
//  * Pieces: piece_plan.hpp (head, 16-byte vector run, tail; Piece::flat is the
//    first byte in d_dst: the loads are aligned accesses of the shards, the
//    stores follow dst_offset), as are the range check and the table chunks.
//  * Chunks: the piece table travels in chunks of at most kTablePieces entries
//    (one slot of the upload ring); a chunk is one launch.
//  * Cost: one sort of the read list, O(n log n).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

#include "piece_plan.hpp"
#include "shmr_ec.h"

namespace shmr {
namespace read {

using namespace piece;   // the range check, the split, the chunks and the tile search, shared with update_plan.hpp

constexpr uint32_t kRebuildFlag = 1u << 30;     // DevPiece::shard: the shard is absent; `shard` is its plan row

// One piece as the kernel reads it (40 bytes, scalar dword loads).
struct DevPiece {
    uint64_t col, dst;
    uint64_t plan;    // rebuild pieces: device address of the pattern's data-only reconstruct plan image
    uint32_t block, len;
    uint32_t shard;   // the data shard (copy) or its row of the plan (rebuild) | kVecFlag | kRebuildFlag
    uint32_t tile0;   // tiles of the table's pieces in front of this one
};
static_assert(sizeof(DevPiece) == 40, "the kernel indexes the table in 10-dword entries");
constexpr uint32_t kPieceWords = sizeof(DevPiece) / 4;
constexpr size_t kTablePieces = kSlotBytes / sizeof(DevPiece);
// (the tile bound of chunk_pieces never cuts a chunk of these entries short)
static_assert(kTablePieces * (kMaxPieceBytes / kTileBytes) <= kMaxGridTiles, "a chunk's tiles are one launch");

// False: a request is out of range, or two destination ranges intersect
// (*pieces is unspecified then).  pieces: the requests' pieces in list order.
inline bool plan(const shmr_ec_read* r, size_t n, uint64_t nblocks, unsigned k, uint64_t shard_len, uint64_t dst_bytes,
                 std::vector<Piece>* pieces) {
    for (size_t i = 0; i < n; ++i)
        if (!valid(r[i], r[i].dst_offset, nblocks, k, shard_len, dst_bytes)) return false;
    // two writes to one destination byte: their order would be undefined
    std::vector<size_t> order;
    if (!disjoint(n, [&](size_t i) { return Key{0, r[i].dst_offset, r[i].len}; }, &order)) return false;
    pieces->clear();
    pieces->reserve(n);
    for (size_t i = 0; i < n; ++i) split(r[i], r[i].dst_offset, i, 0, pieces);
    return true;
}

inline uint32_t count_chunks(const std::vector<Piece>& ps) {
    uint32_t n = 0;
    for (size_t c0 = 0; c0 < ps.size(); c0 += chunk_pieces<DevPiece>(ps, c0)) ++n;
    return n;
}

}  // namespace read
}  // namespace shmr
