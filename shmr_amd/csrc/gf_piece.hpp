// Device side of the ranged-piece tables (piece_plan.hpp): what the update
// kernel (gf_update.hip) and the read kernel (gf_read.hip) both open with, and
// the chunk accesses of their pieces.
#pragma once

#include "gf_tile.hpp"
#include "piece_plan.hpp"

namespace shmr {
namespace kern {

static_assert(piece::kTileBytes == uint32_t(kThreads) * 16, "a tile is one 16-byte chunk per lane");

// The lane's chunk of the piece that holds `tile`: bytes [pos, pos + n) of the
// piece whose WORDS-dword table entry is e (col, flat offset, ..., block, len,
// shard | flags, tile0); n == 0: the lane is past the piece.  The piece is
// workgroup-uniform, every word through scalar loads.  A kernel unpacks the
// entry's other words BEFORE it returns on n == 0, as both did before they
// shared this: with the unpack behind the return the same resources were
// reported but the rebuild read of 512 x 4 KiB went from 0.081 to 0.089 ms
// (profiles/r14/NOTES.md; supposedly a second, dependent scalar round trip).
struct LaneChunk {
    const cu32* e;
    uint32_t pos, n;
};
template <uint32_t WORDS>
__device__ __forceinline__ LaneChunk lane_chunk(const void* pieces, uint32_t npieces, uint32_t tile) {
    const cu32* pw = as_const<cu32>(pieces);
    const uint32_t pi = piece::find_piece([&](uint32_t i) { return pw[size_t(i) * WORDS + WORDS - 1]; }, npieces, tile);
    const cu32* e = pw + size_t(pi) * WORDS;
    const uint32_t len = e[WORDS - 3], tile0 = e[WORDS - 1];
    const uint32_t pos = (tile - tile0) * piece::kTileBytes + threadIdx.x * 16u;
    return LaneChunk{e, pos, pos >= len ? 0u : len - pos < 16u ? len - pos : 16u};
}
__device__ __forceinline__ uint64_t piece_u64(const cu32* e, uint32_t w) {
    return uint64_t(e[w]) | (uint64_t(e[w + 1]) << 32);
}

// The lane's n bytes at q (VEC: n = 16, one vector access through the
// under-aligned type; else byte by byte, exactly [q, q + n)).
template <bool VEC>
__device__ __forceinline__ u32x4 piece_load(const uint8_t* q, int64_t n) {
    if constexpr (VEC) return load16<0>(q);
    else return load_bytes(q, n);
}

template <bool VEC>
__device__ __forceinline__ void piece_store(uint8_t* q, const u32x4& v, int64_t n) {
    if constexpr (VEC) store16<0>(q, v);
    else store_bytes(q, v, n);
}

}  // namespace kern
}  // namespace shmr
