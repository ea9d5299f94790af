// The compare tile of the gfx950 GF(2^8) kernels that check stored shards
// against recomputed ones: the parity check and the checked reconstruct
// (gf_compare.hip).  (gf_locate.hip forms the same quantity at one chunk per
// lane with its stored rows loaded behind the ring: see there.)
//
//   s[r] = XOR_t C[r][t] (x) in[t] ^ stored[r]      (the syndrome of row r)
//
//  * Plan staging, the depth-2 register ring over the k inputs and the GF math
//    (mac) are the encode kernel's (gf_tile.hpp).  The ring's tail is peeled:
//    where the plain ring would re-read shard k-1 in its look-ahead slot, the
//    loads of the stored chunks go out, so they are in flight while the last
//    input is multiplied.
//  * MODE 0 full tiles, MODE 1 one bounds-checked partial tile per block,
//    MODE 2 byte-granular at any alignment (gf_tile.hpp ld / st): bytes at or
//    past len are neither read, stored nor compared (both sides of the compare
//    are zero there).
#pragma once

#include "gf_tile.hpp"

namespace shmr {
namespace kern {

namespace {

// One tile: lanes own columns col0 + slot_chunk(u, tid) * 16, u < U.  On return
// s[u][r] is the lane's syndrome chunk of row r.  STORES (the checked
// reconstruct): rows [0, nstore) are stored to their output slots instead --
// absent shards, never read -- and their s is zero; nstore is workgroup-
// uniform, every branch on it a scalar branch.  Without STORES nstore is
// unused: no such branch, no store.
template <int R, int U, int MODE, int F, bool STORES>
__device__ __forceinline__ void syndrome_tile(const ApplyArgs& a, const Ctx& c, uint32_t nstore, const uint8_t* ib,
                                              uint8_t* ob, uint64_t col0, uint32_t (&s)[U][R][4]) {
    constexpr int TH = kThreads;
    const uint64_t len = a.len;
    const uint32_t tid = threadIdx.x;
    // (accumulators of the tile's own, copied to s once at the end: the ring
    // keeps them in registers as the encode tile's, which it did not through s)
    uint32_t acc[U][R][4];
#pragma unroll
    for (int u = 0; u < U; ++u)
#pragma unroll
        for (int r = 0; r < R; ++r)
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[u][r][j] = 0u;

    auto load = [&](u32x4 (&buf)[U], uint32_t t) {
        const uint8_t* base = ib + c.s_in_off[t];
#pragma unroll
        for (int u = 0; u < U; ++u) buf[u] = ld<MODE, F>(base, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len);
    };
    auto consume = [&](const u32x4 (&buf)[U], uint32_t t) {
        Tab tb[R];
        read_tabs<R>(c, t, tb);
#pragma unroll
        for (int u = 0; u < U; ++u) mac<R, F>(acc[u], buf[u], tb);
    };
    // The stored chunks of the compare rows, at the addresses an encode or a
    // reconstruct would store to.
    u32x4 par[R][U];
    auto load_stored = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            if constexpr (STORES) {
#pragma unroll
                for (int u = 0; u < U; ++u) par[r][u] = u32x4{0u, 0u, 0u, 0u};
                if (uint32_t(r) < nstore) continue;
            }
            const uint8_t* base = ob + c.s_out_off[r];
#pragma unroll
            for (int u = 0; u < U; ++u) par[r][u] = ld<MODE, F>(base, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len);
        }
    };

    u32x4 ring[2][U];
    load(ring[0], 0);
    __builtin_amdgcn_sched_barrier(0);
    // gf_tile.hpp ring2_peeled, typed out for the stored-row loads behind the
    // last input load of either tail (the branch between the tails is uniform).
    // Typed out on purpose: with the ring as a function taking that slot as a
    // callable the compiler no longer merges the two tails and allocates other
    // registers (R = 3: 63 VGPRs for 79, and 7 % slower on RS(8,3)).
    const uint32_t k = a.k;
    uint32_t t = 0;
    for (; t + 2 < k; t += 2) {
        load(ring[1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
        __builtin_amdgcn_sched_barrier(0);
        load(ring[0], t + 2);
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
    }
    if (t + 1 < k) {
        load(ring[1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
        __builtin_amdgcn_sched_barrier(0);
        load_stored();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[1], t + 1);
    } else {
        load_stored();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
    }
    __builtin_amdgcn_sched_barrier(0);

#pragma unroll
    for (int r = 0; r < R; ++r) {
        if (STORES && uint32_t(r) < nstore) {
            uint8_t* o = ob + c.s_out_off[r];
#pragma unroll
            for (int u = 0; u < U; ++u) {
                st<MODE, F>(o, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len,
                            u32x4{acc[u][r][0], acc[u][r][1], acc[u][r][2], acc[u][r][3]});
#pragma unroll
                for (int j = 0; j < 4; ++j) s[u][r][j] = 0u;
            }
        } else {
#pragma unroll
            for (int u = 0; u < U; ++u) {
                s[u][r][0] = acc[u][r][0] ^ par[r][u].x;
                s[u][r][1] = acc[u][r][1] ^ par[r][u].y;
                s[u][r][2] = acc[u][r][2] ^ par[r][u].z;
                s[u][r][3] = acc[u][r][3] ^ par[r][u].w;
            }
        }
    }
}

// The lane's difference flag per row (nz[r] != 0: row r differs in one of the
// lane's columns); returns them ORed together.
template <int R, int U>
__device__ __forceinline__ uint32_t row_flags(const uint32_t (&s)[U][R][4], uint32_t (&nz)[R]) {
    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t d = 0;
#pragma unroll
        for (int u = 0; u < U; ++u) d |= s[u][r][0] | s[u][r][1] | s[u][r][2] | s[u][r][3];
        nz[r] = d;
        any |= d;
    }
    return any;
}

// Reports a tile's differing rows: one ballot says whether the wave saw any
// difference (the common answer is no, and then nothing else runs); else one
// lane ORs the wave's row mask, bit bits[r] for row r, into *word with a vector
// global atomic.  Every lane of the wave must call it.
template <int R>
__device__ __forceinline__ void report_rows(uint32_t any, const uint32_t (&nz)[R], const uint32_t* bits,
                                            uint32_t* word) {
    if (__builtin_amdgcn_ballot_w64(any != 0) == 0) return;
    uint32_t mask = 0;
#pragma unroll
    for (int r = 0; r < R; ++r)
        if (__builtin_amdgcn_ballot_w64(nz[r] != 0) != 0) mask |= 1u << (bits[r] & 31u);
    if ((threadIdx.x & 63u) == 0) atomicOr(word, mask);
}

// Host side of a launch over `ntiles` tiles with `lds` bytes of dynamic LDS:
// the opt-in above 64 KiB for kernel `kern` (its handle: passed on to the
// runtime, never called through) and the grid, one workgroup per tile up to
// the grid limit and at most max_grid (*grid == 0: nothing to launch).
inline hipError_t prepare_launch(const void* kern, size_t lds, uint64_t ntiles, uint32_t* grid,
                                 uint64_t max_grid = 0x7fffffffull) {
    *grid = uint32_t(ntiles < max_grid ? ntiles : max_grid);
    if (lds <= 64 * 1024) return hipSuccess;
    return hipFuncSetAttribute(kern, hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
}

}  // namespace
}  // namespace kern
}  // namespace shmr
