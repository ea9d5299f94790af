// Parity delta update (shmr_ec_update_batch_dev): validation of an update
// list, its split into kernel pieces, and the rounds the pieces run in.
// Host logic only, header-only (tests/test_update_plan.py compiles it on the
// CPU through tools/update_plan_check.cpp); the piece table entry and the
// tile search are also what the kernel (gf_update.hip) reads and runs.
//
// Reed-Solomon is linear: writing `new` over `old` in columns [a, b) of data
// shard j changes parity row r by C[r][j] (x) (old ^ new) in those columns and
// nowhere else.  The kernel reads and rewrites the parity bytes in place, so
// two pieces that store to the same parity byte must not run concurrently.
//
//  * Footprint rule: BYTE-EXACT.  A piece over columns [a, b) of block B
//    stores parity bytes [a, b) of every parity row of B and data bytes
//    [a, b) of its own shard -- nothing wider: interior chunks are whole
//    16-byte stores inside [a, b), edge chunks are stored byte by byte.  Two
//    pieces of one block may share a round iff their column ranges are
//    disjoint, whatever their shards.
//  * Pieces: piece_plan.hpp (head, 16-byte vector run, tail; Piece::flat is the
//    first byte in d_src), as are the range check and the table chunks.
//  * Rounds: per block, interval colouring of the updates' column ranges in
//    order of their first column -- an update takes the round of the range
//    that ended first if it ended at or before its own first column, else a new
//    one.  That is the least number of rounds (the deepest overlap), so
//    pairwise disjoint ranges take one round and m shards written over the
//    same columns take m.  Every piece inherits its update's round.  XOR
//    commutes: the order of the rounds does not matter.
//  * Cost: two sorts of the update list, O(n log n).
#pragma once

#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <functional>
#include <queue>
#include <utility>
#include <vector>

#include "piece_plan.hpp"
#include "shmr_ec.h"

namespace shmr {
namespace update {

using namespace piece;   // the range check, the split, the chunks and the tile search, shared with read_plan.hpp

constexpr bool kByteExactEdges = true;           // the footprint rule above (the checker prints it)

// One piece as the kernel reads it (32 bytes, scalar dword loads).
struct DevPiece {
    uint64_t col, src;
    uint32_t block, len;
    uint32_t shard;   // | kVecFlag
    uint32_t tile0;   // tiles of the table's pieces in front of this one
};
static_assert(sizeof(DevPiece) == 32, "the kernel indexes the table in 8-dword entries");
constexpr uint32_t kPieceWords = sizeof(DevPiece) / 4;
// (8192 pieces of kMaxPieceBytes are exactly 2^31 tiles: the tile bound of chunk_pieces is live here)
constexpr size_t kTablePieces = kSlotBytes / sizeof(DevPiece);

struct Plan {
    std::vector<uint32_t> round_of;   // per update
    uint32_t nrounds = 0;
    std::vector<Piece> pieces;        // ascending round
};

// False: an update is out of range, or two of one (block, shard) intersect
// (*out is unspecified then).  pieces = false: rounds only.
inline bool plan(const shmr_ec_update* u, size_t n, uint64_t nblocks, unsigned k, uint64_t shard_len,
                 uint64_t src_bytes, Plan* out, bool pieces = true) {
    for (size_t i = 0; i < n; ++i)
        if (!valid(u[i], u[i].src_offset, nblocks, k, shard_len, src_bytes)) return false;
    // two writes to one byte of a shard: their order would be undefined
    std::vector<size_t> order;
    auto key = [&](size_t i) { return Key{uint64_t(u[i].block) << 32 | u[i].shard, u[i].offset, u[i].len}; };
    if (!disjoint(n, key, &order)) return false;
    // rounds: per block, the ranges in order of their first column
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (u[a].block != u[b].block) return u[a].block < u[b].block;
        return u[a].offset < u[b].offset;
    });
    out->round_of.assign(n, 0);
    out->nrounds = 0;
    using Open = std::pair<uint64_t, uint32_t>;   // (end column, round) of a range still open
    std::priority_queue<Open, std::vector<Open>, std::greater<Open>> open;
    uint32_t used = 0;
    for (size_t i = 0; i < n; ++i) {
        const shmr_ec_update& x = u[order[i]];
        if (i && u[order[i - 1]].block != x.block) {
            open = {};
            used = 0;
        }
        uint32_t r;
        if (!open.empty() && open.top().first <= x.offset) {
            r = open.top().second;
            open.pop();
        } else {
            r = used++;
        }
        open.push(Open(x.offset + x.len, r));
        out->round_of[order[i]] = r;
        out->nrounds = std::max(out->nrounds, used);
    }
    out->pieces.clear();
    if (!pieces) return true;
    std::vector<Piece> all;
    all.reserve(n);
    for (size_t i = 0; i < n; ++i) split(u[i], u[i].src_offset, i, out->round_of[i], &all);
    // ascending round, stable (a counting sort)
    std::vector<size_t> at(size_t(out->nrounds) + 1, 0);
    for (const Piece& p : all) ++at[p.round + 1];
    for (size_t r = 1; r < at.size(); ++r) at[r] += at[r - 1];
    out->pieces.resize(all.size());
    for (const Piece& p : all) out->pieces[at[p.round]++] = p;
    return true;
}

}  // namespace update
}  // namespace shmr
