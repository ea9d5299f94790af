// GF(2^8) parity delta update kernel for gfx950 (MI355X / CDNA4):
// shmr_ec_update_batch_dev, a write into a device-resident block that keeps
// the block's parity valid without re-encoding it.
//
//   data[j][col] = new[col];   parity[r][col] ^= C[r][j] (x) (old[col] ^ new[col])
//   for every parity row r, over the columns of the piece only
//
// Algorithmic traffic (3 + 2p) * len per piece: old, new and the p parity rows
// read, new and the p parity rows written (update_plan.hpp: the identity, the
// pieces, the byte-exact footprint rule and the rounds).
//
//  * Work mapping: one workgroup per 4 KiB tile of a piece, found by a binary
//    search over the pieces' tile prefixes (DevPiece::tile0; gf_piece.hpp
//    lane_chunk, shared with the read kernel), as seg_block does
//    over segments.  A per-tile descriptor would make the table as long as the
//    written bytes / 4 KiB (a whole-shard write into each of 512 blocks: 65,536
//    entries, 2 MiB, eight slots of the upload ring) where the prefix table is
//    as long as the update list; the search is log2(pieces) scalar loads of one
//    workgroup-uniform word, nothing beside the tile's traffic.
//  * Coefficient tables: a piece has one input shard, so its p tables are
//    wave-uniform -- scalar loads through the constant address space from the
//    encode plan image (entry j * p + r), no LDS.
//  * Per lane one 16-byte chunk: old, new and parity row 0 are loaded, new is
//    stored, then all p rows in turn: the load of row r + 1 is issued before
//    the math of row r (the sched_barrier idiom of do_tile), parity ^= C (x)
//    delta, store.  The accumulator is the parity chunk itself: no row groups.
//  * Vector pieces (kVecFlag: whole chunks) move with 16-byte accesses through
//    the under-aligned type, whatever src_offset and offset are mod 16; the
//    other pieces byte by byte, exactly [col, col + len).  Nothing is loaded or
//    stored outside a piece's bytes.
//  * Cache policy: plain loads and stores (nontemporal not measured).
//  * Measured (tools/update_ab.py, RS(8,3) x 4 MiB x 512
//    blocks, one update per block against a device copy + encode_batch_dev):
//    4 KiB 14.4x, 64 KiB 8.0x, one whole shard 1.31x faster; all k shards 2.2x
//    slower (k rounds over the whole parity).  Between the last two the times
//    cross at 0.18 of a block's data: a cache that rewrites more than about a
//    fifth of a block should copy and re-encode instead.
//
// Not a gf_apply_kernel instantiation and not part of shmr_ec_kernel_inventory.
#include <hip/hip_runtime.h>

#include "gf_piece.hpp"
#include "update_plan.hpp"

namespace shmr {
namespace kern {

namespace {

// The lane's n bytes (VEC: n = 16) at d (data), s (new bytes) and par (parity
// row 0; row r at par + r * spitch).
template <bool VEC>
__device__ __forceinline__ void update_chunk(uint8_t* d, const uint8_t* s, uint8_t* par, uint64_t spitch,
                                             const uint8_t* tabs, uint32_t tab0, uint32_t p, int64_t n) {
    auto row = [&](u32x4& acc, const u32x4& delta, uint32_t r) {
        const Tab tb[1] = {read_tab(tabs, tab0 + r)};
        uint32_t a[1][4] = {{acc.x, acc.y, acc.z, acc.w}};
        mac<1, 0>(a, delta, tb);
        acc = u32x4{a[0][0], a[0][1], a[0][2], a[0][3]};
    };
    auto load = [&](const uint8_t* q) { return piece_load<VEC>(q, n); };
    auto store = [&](uint8_t* q, const u32x4& v) { piece_store<VEC>(q, v, n); };
    const u32x4 oldv = load(d);
    const u32x4 newv = load(s);
    u32x4 cur = load(par);
    __builtin_amdgcn_sched_barrier(0);
    store(d, newv);
    const u32x4 delta = oldv ^ newv;
    uint32_t r = 0;
    for (; r + 1 < p; ++r) {
        const u32x4 nxt = load(par + spitch);
        __builtin_amdgcn_sched_barrier(0);
        row(cur, delta, r);
        store(par, cur);
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
        par += spitch;
    }
    row(cur, delta, r);
    store(par, cur);
}

__global__ __launch_bounds__(kThreads) void gf_update_kernel(const UpdateArgs u) {
    const LaneChunk c = lane_chunk<update::kPieceWords>(u.pieces, u.npieces, u.tile_base + blockIdx.x);
    const uint64_t col = piece_u64(c.e, 0), src = piece_u64(c.e, 2);
    const uint32_t blk = c.e[4], sf = c.e[6], pos = c.pos, n = c.n;
    if (n == 0) return;   // (no barrier and no LDS in this kernel)
    const uint32_t shard = sf & ~update::kVecFlag;
    uint8_t* d = u.data + uint64_t(blk) * u.data_bpitch + uint64_t(shard) * u.data_spitch + col + pos;
    uint8_t* par = u.parity + uint64_t(blk) * u.par_bpitch + col + pos;
    const uint8_t* s = u.src + src + pos;
    if (sf & update::kVecFlag) update_chunk<true>(d, s, par, u.par_spitch, u.tabs, shard * u.p, u.p, 16);
    else update_chunk<false>(d, s, par, u.par_spitch, u.tabs, shard * u.p, u.p, int64_t(n));
}

}  // namespace

hipError_t launch_update(const UpdateArgs& u, hipStream_t stream) {
    if (u.ntiles == 0 || u.npieces == 0) return hipSuccess;
    if (u.ntiles > 0x7fffffffu || u.p == 0) return hipErrorInvalidValue;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    hipLaunchKernelGGL(gf_update_kernel, dim3(u.ntiles), dim3(kThreads), 0, stream, u);
    return hipGetLastError();
}

}  // namespace kern
}  // namespace shmr
