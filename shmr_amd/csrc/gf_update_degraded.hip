// GF(2^8) parity delta update of degraded blocks for gfx950 (MI355X / CDNA4):
// shmr_ec_update_degraded_batch_dev, a write into a device-resident block with
// absent shards that keeps the survivors a punctured codeword -- without
// rebuilding the block first.
//
//   shard j present:  old = data_j[col];                       data_j[col] = new[col]
//   shard j absent:   old = XOR_t D[j][t] (x) input_t[col];    slot j untouched
//   every PRESENT parity row r:  parity_r[col] ^= C[r][j] (x) (old ^ new)[col]
//   over the columns of the piece only; D the data-only reconstruct plan of the
//   block's presence pattern, its inputs the first k present shards
//
// Algorithmic traffic per piece, p' the present parity rows: (3 + 2p') * len
// with the shard present (old, new and p' rows read, new and p' rows written),
// (k + 1 + 2p') * len with it absent (k inputs, new and p' rows read, p' rows
// written), against (k + e) * shard_len for rebuilding the block's e absent
// shards first (update_degraded_plan.hpp: the identity, the byte-exact
// footprint rule, why update_plan.hpp's rounds hold as they stand).
//
//  * Work mapping: one workgroup per 4 KiB tile of a piece, found by the
//    binary search over the pieces' tile prefixes that the update and the read
//    kernel run (gf_piece.hpp lane_chunk, DevPiece::tile0).  Blocks of
//    different presence patterns share a launch: a piece carries the addresses
//    of its pattern's plan image and present-parity-row list.
//  * Coefficient tables: a piece has one data shard, so everything is
//    wave-uniform -- scalar loads through the constant address space, no LDS:
//    D[j][t] from the pattern's plan image (entry t * m + row, as gf_read.hip),
//    C[r][j] from the encode plan image (entry j * p + r, as gf_update.hip),
//    the input shards and the present parity rows from the images' u16 lists.
//    Any k and any p: both are loops, nothing is sized by either (the present
//    rows are a list because p may pass the 32 bits of a mask).
//  * Per lane one 16-byte chunk.  Rebuild: the load of input t + 1 is issued
//    before the math of input t, and the first present parity row before the
//    math of the last input.  Then delta = old ^ new, and the rows as the
//    update kernel walks them: the load of the next present row before the
//    math of this one, parity ^= C (x) delta, store.
//  * A parity shard can be an input of the rebuild and a row the same lane
//    rewrites.  Every store of a lane depends on its delta, which depends on
//    every input load of the lane, and no other lane of the launch touches the
//    lane's columns of the block (the rounds), so no input is read after it
//    was rewritten.
//  * Vector pieces (kVecFlag: whole chunks) move with 16-byte accesses through
//    the under-aligned type, whatever src_offset and offset are mod 16; the
//    other pieces byte by byte, exactly [col, col + len).  Nothing is loaded or
//    stored outside a piece's bytes; absent slots are neither read nor written.
//  * Cache policy: plain loads and stores (nontemporal not measured).
//  * Measured (tools/update_degraded_ab.py, RS(8,3) x
//    4 MiB x 512 blocks, one update per block into its lost shard, against
//    reconstruct_batch_dev(data_only) + update_batch_dev): 4 KiB 4.6x, 64 KiB
//    4.1x, 256 KiB 1.5x, the whole shard 1.12x faster; into a present shard of
//    the same blocks 4.8x, 5.1x, 2.5x, 1.73x; the lost shard and its neighbour
//    1.10x, all k shards 1.03x.  Rebuilding first never wins.  The small sizes
//    sit on a 0.09 ms floor per call (host side, eight patterns), not traffic.
//
// Not a gf_apply_kernel instantiation and not part of shmr_ec_kernel_inventory.
#include <hip/hip_runtime.h>

#include "gf_piece.hpp"
#include "update_degraded_plan.hpp"

namespace shmr {
namespace kern {

namespace {

// The lane's n bytes (VEC: n = 16) of one piece: b is the lane's column of
// shard 0 of the block, s the new bytes.  plan != nullptr: data shard `shard`
// is absent and row `row` of that image rebuilds it.  rows: the pattern's
// present parity rows.  tabs: the encode plan's PermTab[k][p].
template <bool VEC>
__device__ __forceinline__ void degraded_chunk(uint8_t* b, uint64_t spitch, const uint8_t* s, const uint8_t* plan,
                                               uint32_t shard, uint32_t row, const uint8_t* rows, const uint8_t* tabs,
                                               uint32_t k, uint32_t p, int64_t n) {
    auto load = [&](const uint8_t* q) { return piece_load<VEC>(q, n); };
    auto store = [&](uint8_t* q, const u32x4& v) { piece_store<VEC>(q, v, n); };
    // Row list image: [u32 0][u32 np][u16 row[np]] (a plan image without inputs, gf256.hpp).
    const uint32_t np = as_const<cu32>(rows)[1];
    const uint16_t* ridx = reinterpret_cast<const uint16_t*>(rows + 8);
    uint8_t* par0 = b + uint64_t(k) * spitch;
    uint32_t r = np ? plan_u16(ridx, 0) : 0u;
    const u32x4 newv = load(s);
    u32x4 oldv, cur{0u, 0u, 0u, 0u};
    if (plan) {
        // Image: [u32 k][u32 m][u16 in_idx[k]][u16 out_idx[m]] padded to 32 B, PermTab[k][m] (gf256.hpp).
        const uint32_t m = as_const<cu32>(plan)[1];
        const uint16_t* in_idx = reinterpret_cast<const uint16_t*>(plan + 8);
        const uint8_t* dtabs = plan + ((8u + 2u * k + 2u * m + 31u) & ~31u);
        auto step = [&](uint32_t (&acc)[1][4], const u32x4& v, uint32_t t) {
            const Tab tb[1] = {read_tab(dtabs, t * m + row)};
            mac<1, 0>(acc, v, tb);
        };
        uint32_t acc[1][4] = {{0u, 0u, 0u, 0u}};
        u32x4 in = load(b + uint64_t(plan_u16(in_idx, 0)) * spitch);
        uint32_t t = 0;
        for (; t + 1 < k; ++t) {
            const u32x4 nxt = load(b + uint64_t(plan_u16(in_idx, t + 1)) * spitch);
            __builtin_amdgcn_sched_barrier(0);
            step(acc, in, t);
            __builtin_amdgcn_sched_barrier(0);
            in = nxt;
        }
        if (np) cur = load(par0 + uint64_t(r) * spitch);
        __builtin_amdgcn_sched_barrier(0);
        step(acc, in, t);
        oldv = u32x4{acc[0][0], acc[0][1], acc[0][2], acc[0][3]};
    } else {
        uint8_t* d = b + uint64_t(shard) * spitch;
        oldv = load(d);
        if (np) cur = load(par0 + uint64_t(r) * spitch);
        __builtin_amdgcn_sched_barrier(0);
        store(d, newv);
    }
    if (np == 0) return;
    const u32x4 delta = oldv ^ newv;
    auto mul_row = [&](u32x4& acc, uint32_t rr) {
        const Tab tb[1] = {read_tab(tabs, shard * p + rr)};
        uint32_t a[1][4] = {{acc.x, acc.y, acc.z, acc.w}};
        mac<1, 0>(a, delta, tb);
        acc = u32x4{a[0][0], a[0][1], a[0][2], a[0][3]};
    };
    for (uint32_t i = 0; i + 1 < np; ++i) {
        const uint32_t rn = plan_u16(ridx, i + 1);
        const u32x4 nxt = load(par0 + uint64_t(rn) * spitch);
        __builtin_amdgcn_sched_barrier(0);
        mul_row(cur, r);
        store(par0 + uint64_t(r) * spitch, cur);
        __builtin_amdgcn_sched_barrier(0);
        cur = nxt;
        r = rn;
    }
    mul_row(cur, r);
    store(par0 + uint64_t(r) * spitch, cur);
}

__global__ __launch_bounds__(kThreads) void gf_update_degraded_kernel(const UpdateDegradedArgs u) {
    const LaneChunk c = lane_chunk<degraded::kPieceWords>(u.pieces, u.npieces, u.tile_base + blockIdx.x);
    const uint64_t col = piece_u64(c.e, 0), src = piece_u64(c.e, 2), plan = piece_u64(c.e, 4), rows = piece_u64(c.e, 6);
    const uint32_t blk = c.e[8], sf = c.e[10], pos = c.pos, n = c.n;
    if (n == 0) return;   // (no barrier and no LDS in this kernel)
    const uint32_t shard = sf & degraded::kShardMask, row = (sf >> degraded::kRowShift) & degraded::kRowMask;
    uint8_t* b = u.shards + uint64_t(blk) * u.bpitch + col + pos;
    const uint8_t* s = u.src + src + pos;
    const uint8_t* image = (sf & degraded::kRebuildFlag) ? reinterpret_cast<const uint8_t*>(uintptr_t(plan)) : nullptr;
    const uint8_t* rlist = reinterpret_cast<const uint8_t*>(uintptr_t(rows));
    if (sf & degraded::kVecFlag) degraded_chunk<true>(b, u.spitch, s, image, shard, row, rlist, u.tabs, u.k, u.p, 16);
    else degraded_chunk<false>(b, u.spitch, s, image, shard, row, rlist, u.tabs, u.k, u.p, int64_t(n));
}

}  // namespace

hipError_t launch_update_degraded(const UpdateDegradedArgs& u, hipStream_t stream) {
    if (u.ntiles == 0 || u.npieces == 0) return hipSuccess;
    if (u.ntiles > 0x7fffffffu || u.k == 0 || u.p == 0) return hipErrorInvalidValue;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    hipLaunchKernelGGL(gf_update_degraded_kernel, dim3(u.ntiles), dim3(kThreads), 0, stream, u);
    return hipGetLastError();
}

}  // namespace kern
}  // namespace shmr
