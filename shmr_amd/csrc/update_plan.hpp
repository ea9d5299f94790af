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
//  * Pieces: an update [offset, offset + len) becomes a byte-granular head up
//    to the next multiple of 16 (if offset is off one), vector pieces of whole
//    16-column chunks (at most kMaxPieceBytes each), and a byte-granular tail.
//    Chunks sit on multiples of 16 in COLUMN space: with 16-byte aligned
//    bases and pitches they are aligned accesses of the shards.
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
#include <numeric>
#include <queue>
#include <utility>
#include <vector>

#include "shmr_ec.h"

#if defined(__HIP__)
#define SHMR_UPDATE_HD __attribute__((host)) __attribute__((device))
#else
#define SHMR_UPDATE_HD
#endif

namespace shmr {
namespace update {

constexpr uint32_t kChunk = 16;                  // bytes of one vector access
constexpr uint32_t kTileBytes = 256 * kChunk;    // columns one workgroup covers (kern::kThreads lanes)
constexpr uint64_t kMaxPieceBytes = 1u << 30;    // a piece's length and tile count fit 32 bits
constexpr bool kByteExactEdges = true;           // the footprint rule above (the checker prints it)
constexpr uint32_t kVecFlag = 1u << 31;          // DevPiece::shard: whole 16-byte chunks, vector accesses

// One piece as the planner gives it, in round order.
struct Piece {
    uint64_t col, src;   // first column in the shard; first byte in d_src
    uint64_t update;     // index of the update it is a part of
    uint32_t block, shard, len, round;
    bool vec;            // col and len are multiples of kChunk
};

// One piece as the kernel reads it (32 bytes, scalar dword loads).
struct DevPiece {
    uint64_t col, src;
    uint32_t block, len;
    uint32_t shard;   // | kVecFlag
    uint32_t tile0;   // tiles of the table's pieces in front of this one
};
static_assert(sizeof(DevPiece) == 32, "the kernel indexes the table in 8-dword entries");

SHMR_UPDATE_HD inline uint32_t piece_tiles(uint32_t len) { return (len + kTileBytes - 1) / kTileBytes; }

// The piece of pieces [0, n) that holds `tile`: the last one whose tile0 is
// <= tile (tile0(i) ascending, tile0(0) <= tile, every piece has >= 1 tile).
template <class Tile0>
SHMR_UPDATE_HD inline uint32_t find_piece(Tile0 tile0, uint32_t n, uint32_t tile) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tile0(mid) <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

struct Plan {
    std::vector<uint32_t> round_of;   // per update
    uint32_t nrounds = 0;
    std::vector<Piece> pieces;        // ascending round
};

inline bool valid(const shmr_ec_update& u, uint64_t nblocks, unsigned k, uint64_t shard_len, uint64_t src_bytes) {
    // (no sum is formed: offset + len and src_offset + len may pass 2^64)
    return u.block < nblocks && u.shard < k && u.len != 0 && u.len <= shard_len && u.offset <= shard_len - u.len &&
           u.len <= src_bytes && u.src_offset <= src_bytes - u.len;
}

inline void split(const shmr_ec_update& u, uint64_t index, uint32_t round, std::vector<Piece>* out) {
    uint64_t col = u.offset, src = u.src_offset, left = u.len;
    auto emit = [&](uint64_t n, bool vec) {
        out->push_back(Piece{col, src, index, u.block, u.shard, uint32_t(n), round, vec});
        col += n;
        src += n;
        left -= n;
    };
    if (col % kChunk) emit(std::min<uint64_t>(left, kChunk - col % kChunk), false);
    while (left >= kChunk) emit(std::min<uint64_t>(left / kChunk * kChunk, kMaxPieceBytes), true);
    if (left) emit(left, false);
}

// False: an update is out of range, or two of one (block, shard) intersect
// (*out is unspecified then).  pieces = false: rounds only.
inline bool plan(const shmr_ec_update* u, size_t n, uint64_t nblocks, unsigned k, uint64_t shard_len,
                 uint64_t src_bytes, Plan* out, bool pieces = true) {
    for (size_t i = 0; i < n; ++i)
        if (!valid(u[i], nblocks, k, shard_len, src_bytes)) return false;
    std::vector<size_t> order(n);
    std::iota(order.begin(), order.end(), size_t(0));
    // two writes to one byte of a shard: their order would be undefined
    std::sort(order.begin(), order.end(), [&](size_t a, size_t b) {
        if (u[a].block != u[b].block) return u[a].block < u[b].block;
        if (u[a].shard != u[b].shard) return u[a].shard < u[b].shard;
        return u[a].offset < u[b].offset;
    });
    for (size_t i = 1; i < n; ++i) {
        const shmr_ec_update &a = u[order[i - 1]], &b = u[order[i]];
        if (a.block == b.block && a.shard == b.shard && a.offset + a.len > b.offset) return false;
    }
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
    for (size_t i = 0; i < n; ++i) split(u[i], i, out->round_of[i], &all);
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
