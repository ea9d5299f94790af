// Ranged pieces: what the parity delta update (update_plan.hpp) and the ranged
// read (read_plan.hpp) share.  Both take a list of byte ranges of data shards,
// each with its place in one flat device buffer (the update's d_src, the read's
// d_dst), and run it as a table of pieces.  Host logic, header-only and
// CPU-compilable; the tile search is also what both kernels run (gf_piece.hpp).
//
//  * Range check: six terms, no sum formed (offset + len may pass 2^64).
//  * Pieces: a range [offset, offset + len) becomes a byte-granular head up to
//    the next multiple of 16 (if offset is off one), vector pieces of whole
//    16-column chunks (at most kMaxPieceBytes each), and a byte-granular tail.
//    Chunks sit on multiples of 16 in COLUMN space: with 16-byte aligned bases
//    and pitches they are aligned accesses of the shards.
//  * Table entries: both DevPiece structs open with col and the flat offset and
//    close with block, len, shard | flags, tile0, whatever lies between.
//  * Chunks: the piece table travels in chunks of at most one upload-ring slot
//    of entries and fewer than 2^31 tiles (a launch's grid); chunk_pieces is
//    the one rule, for the drivers and for shmr_ec_read_plan.
#pragma once

#include <algorithm>
#include <array>
#include <cstddef>
#include <cstdint>
#include <numeric>
#include <vector>

#if defined(__HIP__)
#define SHMR_PIECE_HD __attribute__((host)) __attribute__((device))
#else
#define SHMR_PIECE_HD
#endif

namespace shmr {
namespace piece {

constexpr uint32_t kChunk = 16;                  // bytes of one vector access
constexpr uint32_t kTileBytes = 256 * kChunk;    // columns one workgroup covers (kern::kThreads lanes)
constexpr uint64_t kMaxPieceBytes = 1u << 30;    // a piece's length and tile count fit 32 bits
constexpr uint32_t kVecFlag = 1u << 31;          // DevPiece::shard: whole 16-byte chunks, vector accesses
constexpr size_t kSlotBytes = 256 * 1024;        // core::UploadRing::kSlotBytes (asserted in ec_core.cpp)
constexpr uint64_t kMaxGridTiles = 0x7fffffffull;

// One piece as the planners give it.
struct Piece {
    uint64_t col, flat;   // first column in the shard; first byte in the flat buffer
    uint64_t request;     // index of the update / read it is a part of
    uint32_t block, shard, len;
    uint32_t round;       // updates only (update_plan.hpp)
    bool vec;             // col and len are multiples of kChunk
};

SHMR_PIECE_HD inline uint32_t piece_tiles(uint32_t len) { return (len + kTileBytes - 1) / kTileBytes; }

// The piece of pieces [0, n) that holds `tile`: the last one whose tile0 is
// <= tile (tile0(i) ascending, tile0(0) <= tile, every piece has >= 1 tile).
template <class Tile0>
SHMR_PIECE_HD inline uint32_t find_piece(Tile0 tile0, uint32_t n, uint32_t tile) {
    uint32_t lo = 0, hi = n;
    while (hi - lo > 1) {
        const uint32_t mid = lo + ((hi - lo) >> 1);
        if (tile0(mid) <= tile) lo = mid;
        else hi = mid;
    }
    return lo;
}

// A request r (shmr_ec_update, shmr_ec_read): bytes [offset, offset + len) of
// a data shard, which start at `flat` in the flat buffer.
template <class R>
inline bool valid(const R& r, uint64_t flat, uint64_t nblocks, unsigned k, uint64_t shard_len, uint64_t flat_bytes) {
    // (no sum is formed: offset + len and flat + len may pass 2^64)
    return r.block < nblocks && r.shard < k && r.len != 0 && r.len <= shard_len && r.offset <= shard_len - r.len &&
           r.len <= flat_bytes && flat <= flat_bytes - r.len;
}

template <class R>
inline void split(const R& r, uint64_t flat, uint64_t index, uint32_t round, std::vector<Piece>* out) {
    uint64_t col = r.offset, left = r.len;
    auto emit = [&](uint64_t n, bool vec) {
        out->push_back(Piece{col, flat, index, r.block, r.shard, uint32_t(n), round, vec});
        col += n;
        flat += n;
        left -= n;
    };
    if (col % kChunk) emit(std::min<uint64_t>(left, kChunk - col % kChunk), false);
    while (left >= kChunk) emit(std::min<uint64_t>(left / kChunk * kChunk, kMaxPieceBytes), true);
    if (left) emit(left, false);
}

// Whether no two of n valid ranges intersect where they write.  key(i) is range
// i's {space, first byte written, bytes}: ranges of different spaces never
// meet.  *order: scratch, left sorted by key.
using Key = std::array<uint64_t, 3>;
template <class KeyOf>
inline bool disjoint(size_t n, KeyOf key, std::vector<size_t>* order) {
    order->resize(n);
    std::iota(order->begin(), order->end(), size_t(0));
    std::sort(order->begin(), order->end(), [&](size_t a, size_t b) { return key(a) < key(b); });
    for (size_t i = 1; i < n; ++i) {
        const Key a = key((*order)[i - 1]), b = key((*order)[i]);
        if (a[0] == b[0] && a[1] + a[2] > b[1]) return false;   // (valid: no wrap)
    }
    return true;
}

// The pieces of the table chunk of `Entry`s that starts at piece c0: as many as
// a ring slot holds, and fewer than 2^31 tiles (>= 1 piece: a piece has at
// most kMaxPieceBytes / kTileBytes of them).
template <class Entry>
inline size_t chunk_pieces(const std::vector<Piece>& ps, size_t c0) {
    size_t cnt = 0;
    for (uint64_t tiles = 0; c0 + cnt < ps.size() && cnt < kSlotBytes / sizeof(Entry); ++cnt)
        if ((tiles += piece_tiles(ps[c0 + cnt].len)) > kMaxGridTiles) break;
    return cnt;
}

}  // namespace piece
}  // namespace shmr
