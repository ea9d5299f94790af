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
//  * Pieces: a request [offset, offset + len) becomes a byte-granular head up
//    to the next multiple of 16 (if offset is off one), vector pieces of whole
//    16-column chunks (at most kMaxPieceBytes each), and a byte-granular tail
//    -- update::split's shapes.  Chunks sit on multiples of 16 in COLUMN space:
//    with 16-byte aligned bases and pitches they are aligned loads of the
//    shards (the stores follow dst_offset).
//  * Chunks: the piece table travels in chunks of at most kTablePieces entries
//    (one slot of the upload ring) and fewer than 2^31 tiles; a chunk is one
//    launch.
//  * Cost: one sort of the read list, O(n log n).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#include "shmr_ec.h"
#include "update_plan.hpp"

namespace shmr {
namespace read {

using update::find_piece;   // the tile search, shared with the update kernel
using update::kChunk;
using update::kMaxPieceBytes;
using update::kTileBytes;
using update::kVecFlag;                         // DevPiece::shard: whole 16-byte chunks, vector accesses
using update::piece_tiles;
constexpr uint32_t kRebuildFlag = 1u << 30;     // DevPiece::shard: the shard is absent; `shard` is its plan row
constexpr size_t kSlotBytes = 256 * 1024;       // core::UploadRing::kSlotBytes (asserted in ec_core.cpp)

// One piece as the planner gives it, in request order.
struct Piece {
    uint64_t col, dst;   // first column in the shard; first byte in d_dst
    uint64_t read;       // index of the request it is a part of
    uint32_t block, shard, len;
    bool vec;            // col and len are multiples of kChunk
};

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

inline bool valid(const shmr_ec_read& r, uint64_t nblocks, unsigned k, uint64_t shard_len, uint64_t dst_bytes) {
    // (no sum is formed: offset + len and dst_offset + len may pass 2^64)
    return r.block < nblocks && r.shard < k && r.len != 0 && r.len <= shard_len && r.offset <= shard_len - r.len &&
           r.len <= dst_bytes && r.dst_offset <= dst_bytes - r.len;
}

inline void split(const shmr_ec_read& r, uint64_t index, std::vector<Piece>* out) {
    uint64_t col = r.offset, dst = r.dst_offset, left = r.len;
    auto emit = [&](uint64_t n, bool vec) {
        out->push_back(Piece{col, dst, index, r.block, r.shard, uint32_t(n), vec});
        col += n;
        dst += n;
        left -= n;
    };
    if (col % kChunk) emit(std::min<uint64_t>(left, kChunk - col % kChunk), false);
    while (left >= kChunk) emit(std::min<uint64_t>(left / kChunk * kChunk, kMaxPieceBytes), true);
    if (left) emit(left, false);
}

// False: a request is out of range, or two destination ranges intersect
// (*pieces is unspecified then).  pieces: the requests' pieces in list order.
inline bool plan(const shmr_ec_read* r, size_t n, uint64_t nblocks, unsigned k, uint64_t shard_len, uint64_t dst_bytes,
                 std::vector<Piece>* pieces) {
    for (size_t i = 0; i < n; ++i)
        if (!valid(r[i], nblocks, k, shard_len, dst_bytes)) return false;
    // two writes to one destination byte: their order would be undefined
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), size_t(0));
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) { return r[a].dst_offset < r[b].dst_offset; });
    for (size_t i = 1; i < n; ++i) {
        const shmr_ec_read &a = r[order[i - 1]], &b = r[order[i]];
        if (a.dst_offset + a.len > b.dst_offset) return false;   // (valid: no wrap)
    }
    pieces->clear();
    pieces->reserve(n);
    for (size_t i = 0; i < n; ++i) split(r[i], i, pieces);
    return true;
}

// The pieces of the table chunk that starts at piece c0: as many as a ring slot
// holds.  Its tiles fit a grid whatever the pieces are.
static_assert(kTablePieces * (kMaxPieceBytes / kTileBytes) <= 0x7fffffffull, "a chunk's tiles are one launch");
inline size_t chunk_pieces(const std::vector<Piece>& ps, size_t c0) { return std::min(kTablePieces, ps.size() - c0); }

inline uint32_t count_chunks(const std::vector<Piece>& ps) {
    return uint32_t((ps.size() + kTablePieces - 1) / kTablePieces);
}

}  // namespace read
}  // namespace shmr
