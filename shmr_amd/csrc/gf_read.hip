// GF(2^8) ranged read kernel for gfx950 (MI355X / CDNA4):
// shmr_ec_read_batch_dev, byte ranges of data shards of device-resident blocks
// copied out -- or, where the shard is absent, rebuilt -- into one destination
// buffer, without rebuilding anything outside the ranges.
//
//   present shard:  dst[x] = shard[col + x]
//   absent shard:   dst[x] = XOR_t D[row][t] (x) input_t[col + x]
//   over the columns of the piece only; D the data-only reconstruct plan of the
//   block's presence pattern, its inputs the first k present shards
//
// Algorithmic traffic per piece: 2 * len for a copy (read, write) and
// (k + 1) * len for a rebuild (k inputs read, the range written), against
// (k + 1) * shard_len for rebuilding the shard first (read_plan.hpp: the
// pieces, the byte-exact footprint rule, the table chunks).
//
//  * Work mapping: one workgroup per 4 KiB tile of a piece, found by the
//    binary search over the pieces' tile prefixes that the update kernel runs
//    (gf_piece.hpp lane_chunk, DevPiece::tile0): log2(pieces) scalar loads of one
//    workgroup-uniform word.  Blocks of different presence patterns share a
//    launch: a rebuild piece carries the address of its own plan image and its
//    row in it.
//  * Coefficient tables: a piece has one output row, so the table of input t
//    (entry t * m + row of the image's PermTab[k][m]) is wave-uniform --
//    scalar loads through the constant address space, no LDS.  The input
//    shards come from the image's in_idx the same way.  Any k: the inputs are
//    a loop, nothing is sized by k.
//  * Per lane one 16-byte chunk.  Copy: one load, one store.  Rebuild: the
//    load of input t + 1 is issued before the math of input t (the
//    sched_barrier idiom of do_tile), acc ^= D (x) input, one store.
//  * Vector pieces (kVecFlag: whole chunks) move with 16-byte accesses through
//    the under-aligned type, whatever offset and dst_offset are mod 16; the
//    other pieces byte by byte, exactly [col, col + len).  Nothing is loaded or
//    stored outside a piece's bytes; absent slots are never read.
//  * Cache policy: plain loads and stores (nontemporal not measured).
//  * Measured (tools/read_ab.py, RS(8,3) x 4 MiB x 512
//    blocks, one request per block into its lost shard, against
//    reconstruct_batch_dev_out(data_only) + a device copy of the ranges):
//    4 KiB 5.2x, 64 KiB 3.7x, one whole shard 1.16x faster.  The two small
//    sizes share a 0.079 ms floor per call (table upload, launch, eight
//    patterns' plan lookups on the host), not traffic; a whole shard is 1.19x
//    slower than reconstruct_batch_dev_out alone, where whole-shard reads
//    belong.  Copy pieces against a torch gather: 4 KiB 0.51x, 64 KiB 2.8x,
//    whole shard 6.7x.
//
// Not a gf_apply_kernel instantiation and not part of shmr_ec_kernel_inventory.
#include <hip/hip_runtime.h>

#include "gf_piece.hpp"
#include "read_plan.hpp"

namespace shmr {
namespace kern {

namespace {

// The lane's n bytes (VEC: n = 16) of row `row` of the plan image: b is the
// lane's column of shard 0 of the block, out where the bytes go.
template <bool VEC>
__device__ __forceinline__ void rebuild_chunk(const uint8_t* b, uint64_t spitch, const uint8_t* plan, uint32_t row,
                                              uint32_t k, uint8_t* out, int64_t n) {
    // Image: [u32 k][u32 m][u16 in_idx[k]][u16 out_idx[m]] padded to 32 B, PermTab[k][m] (gf256.hpp).
    const uint32_t m = as_const<cu32>(plan)[1];
    const uint16_t* in_idx = reinterpret_cast<const uint16_t*>(plan + 8);
    const uint8_t* tabs = plan + ((8u + 2u * k + 2u * m + 31u) & ~31u);
    auto step = [&](uint32_t (&acc)[1][4], const u32x4& v, uint32_t t) {
        const Tab tb[1] = {read_tab(tabs, t * m + row)};
        mac<1, 0>(acc, v, tb);
    };
    uint32_t acc[1][4] = {{0u, 0u, 0u, 0u}};
    u32x4 cur = piece_load<VEC>(b + uint64_t(plan_u16(in_idx, 0)) * spitch, n);
    uint32_t t = 0;
    for (; t + 1 < k; ++t) {
        const u32x4 nxt = piece_load<VEC>(b + uint64_t(plan_u16(in_idx, t + 1)) * spitch, n);
        __builtin_amdgcn_sched_barrier(0);
        step(acc, cur, t);
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
    }
    step(acc, cur, t);
    piece_store<VEC>(out, u32x4{acc[0][0], acc[0][1], acc[0][2], acc[0][3]}, n);
}

__global__ __launch_bounds__(kThreads) void gf_read_kernel(const ReadArgs r) {
    const LaneChunk c = lane_chunk<read::kPieceWords>(r.pieces, r.npieces, blockIdx.x);
    const uint64_t col = piece_u64(c.e, 0), dst = piece_u64(c.e, 2), plan = piece_u64(c.e, 4);
    const uint32_t blk = c.e[6], sf = c.e[8], pos = c.pos, n = c.n;
    if (n == 0) return;   // (no barrier and no LDS in this kernel)
    const uint32_t shard = sf & ~(read::kVecFlag | read::kRebuildFlag);
    const uint8_t* b = r.shards + uint64_t(blk) * r.bpitch + col + pos;
    uint8_t* out = r.dst + dst + pos;
    const bool vec = (sf & read::kVecFlag) != 0;
    if (sf & read::kRebuildFlag) {
        const uint8_t* image = reinterpret_cast<const uint8_t*>(uintptr_t(plan));
        if (vec) rebuild_chunk<true>(b, r.spitch, image, shard, r.k, out, 16);
        else rebuild_chunk<false>(b, r.spitch, image, shard, r.k, out, int64_t(n));
    } else {
        const uint8_t* s = b + uint64_t(shard) * r.spitch;
        if (vec) piece_store<true>(out, piece_load<true>(s, 16), 16);
        else piece_store<false>(out, piece_load<false>(s, int64_t(n)), int64_t(n));
    }
}

}  // namespace

hipError_t launch_read(const ReadArgs& r, hipStream_t stream) {
    if (r.ntiles == 0 || r.npieces == 0) return hipSuccess;
    if (r.ntiles > 0x7fffffffu || r.k == 0) return hipErrorInvalidValue;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    hipLaunchKernelGGL(gf_read_kernel, dim3(r.ntiles), dim3(kThreads), 0, stream, r);
    return hipGetLastError();
}

}  // namespace kern
}  // namespace shmr
