// GF(2^8) parity check kernel for gfx950 (MI355X / CDNA4): ReedSolomon::verify.
//
//   mismatch[j] |= 1 << min(row0 + r, 31)   for every parity row r of block j with
//   stored[r][col] != XOR_t C[r][t] (x) data[t][col]   at some col in [0, len)
//
// The encode tile (gf_tile.hpp do_tile) with its stores replaced by loads and a
// compare: an all-read kernel, algorithmic traffic (k + R) * len per block and
// launch group, nothing written for a block that is a codeword.
//
//  * Plan staging, the depth-2 register ring over the k data shards and the
//    GF math (mac) are the encode kernel's.  The ring's tail is peeled: where
//    the plain ring would re-read shard k-1 in its look-ahead slot, the loads
//    of the R stored parity chunks go out, so they are in flight while the last
//    data shard is multiplied.
//  * Compare: stored ^ recomputed, the four dwords ORed, per row; one ballot
//    says whether the wave saw any difference (the common answer is no, and
//    then nothing else runs); else one lane ORs the wave's row mask into the
//    block's word with a vector global atomic.
//  * MODE 0 full tiles, MODE 1 one bounds-checked partial tile per block,
//    MODE 2 byte-granular at any alignment (gf_tile.hpp ld): bytes at or past
//    len are read by neither the data nor the parity loads (both sides of the
//    compare are zero there).
//
// These kernels are not gf_apply_kernel instantiations and not part of
// shmr_ec_kernel_inventory (which lists what encode and reconstruct dispatch).
#include <hip/hip_runtime.h>

#include "gf_tile.hpp"

namespace shmr {
namespace kern {

namespace {

// One tile; returns the lane's per-row difference flags ORed into row bits.
template <int R, int U, int MODE, int F>
__device__ __forceinline__ uint32_t verify_tile(const ApplyArgs& a, const Ctx& c, const uint8_t* ib, const uint8_t* ob,
                                                uint64_t col0, uint32_t (&nz)[R]) {
    constexpr int TH = kThreads;
    const uint32_t k = a.k;
    const uint64_t len = a.len;
    const uint32_t tid = threadIdx.x;
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
    // The stored parity chunks, at the addresses an encode would store to.
    u32x4 par[R][U];
    auto load_parity = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
            const uint8_t* base = ob + c.s_out_off[r];
#pragma unroll
            for (int u = 0; u < U; ++u) par[r][u] = ld<MODE, F>(base, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len);
        }
    };

    u32x4 ring[2][U];
    load(ring[0], 0);
    __builtin_amdgcn_sched_barrier(0);
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
    // One or two shards are left; the parity loads take the look-ahead slot
    // behind the last data load (the branch is uniform).
    if (t + 1 < k) {
        load(ring[1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
        __builtin_amdgcn_sched_barrier(0);
        load_parity();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[1], t + 1);
    } else {
        load_parity();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
    }
    __builtin_amdgcn_sched_barrier(0);

    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        uint32_t d = 0;
#pragma unroll
        for (int u = 0; u < U; ++u)
            d |= (par[r][u].x ^ acc[u][r][0]) | (par[r][u].y ^ acc[u][r][1]) | (par[r][u].z ^ acc[u][r][2]) |
                 (par[r][u].w ^ acc[u][r][3]);
        nz[r] = d;
        any |= d;
    }
    return any;
}

// VerifyArgs: the encode launch's arguments (single plan, strided blocks, no
// pointer table, no segments) plus the per-block result words.
struct VerifyArgs {
    ApplyArgs a;
    uint32_t* mismatch;   // [nblk], word j for launch block j
};

template <int R, int U, int MODE, int F>
__global__ __launch_bounds__(kThreads) void gf_verify_kernel(const VerifyArgs va) {
    constexpr int TH = kThreads;
    const ApplyArgs& a = va.a;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Ctx c{};
    stage_plan<R, TH, false>(a, a.plan, smem, c, 0);
    __syncthreads();
    const uint64_t tb = uint64_t(TH) * 16 * U;
    const uint32_t tpb = a.tiles_per_block;
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t j = tile / tpb, cc = tile - j * tpb;
        const uint64_t blk = a.blk_first + j * a.blk_stride;
        const uint8_t* ib = a.in_base + blk * a.in_bpitch;
        const uint8_t* ob = a.out_base + blk * a.out_bpitch;
        uint32_t nz[R];
        const uint32_t any = verify_tile<R, U, MODE, F>(a, c, ib, ob, a.col_base + cc * tb, nz);
        // every lane of the wave is here (no lane leaves a tile early)
        if (__builtin_amdgcn_ballot_w64(any != 0) != 0) {
            uint32_t mask = 0;
#pragma unroll
            for (int r = 0; r < R; ++r) {
                const uint32_t bit = a.row0 + r < 31u ? a.row0 + r : 31u;
                if (__builtin_amdgcn_ballot_w64(nz[r] != 0) != 0) mask |= 1u << bit;
            }
            if ((threadIdx.x & 63u) == 0) atomicOr(va.mismatch + j, mask);
        }
    }
}

template <int R, int U, int MODE, int F>
hipError_t launch_verify_one(const VerifyArgs& va, hipStream_t stream) {
    const ApplyArgs& a = va.a;
    const size_t lds = size_t(a.k) * R * 32 + size_t(a.k) * 8 + size_t(R) * 8;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gf_verify_kernel<R, U, MODE, F>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    uint64_t grid = a.ntiles;   // one workgroup per tile, as the encode launches
    if (grid > 0x7fffffffull) grid = 0x7fffffffull;
    if (grid == 0) return hipSuccess;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    hipLaunchKernelGGL((gf_verify_kernel<R, U, MODE, F>), dim3(uint32_t(grid)), dim3(kThreads), lds, stream, va);
    return hipGetLastError();
}

// Full tiles: the encode policy's loads (nontemporal); the tail and the
// byte-granular kernels load plainly, as the encode's do.  The product library
// carries the full-tile kernel of verify_chunks(R) only, the tools build both
// tile sizes (tools/verify_ab.py --u-ab).
constexpr int kFullFlags = kNtLoad | kDepth2;
#ifdef SHMR_EC_TOOLS
constexpr bool kBothTileSizes = true;
#else
constexpr bool kBothTileSizes = false;
#endif

template <int R>
hipError_t dispatch_verify(const VerifyArgs& va, int u, int mode, hipStream_t stream) {
    switch (mode) {
        case 0:
            if constexpr (kBothTileSizes || verify_chunks(R) == 2)
                if (u == 2) return launch_verify_one<R, 2, 0, kFullFlags | kWaveRun>(va, stream);
            if constexpr (kBothTileSizes || verify_chunks(R) == 1)
                if (u == 1) return launch_verify_one<R, 1, 0, kFullFlags>(va, stream);
            return hipErrorInvalidValue;
        case 1: return launch_verify_one<R, 1, 1, 0>(va, stream);
        case 2: return launch_verify_one<R, 1, 2, 0>(va, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_verify(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, int u, int mode, hipStream_t stream) {
    VerifyArgs va;
    va.a = a;
    va.mismatch = mismatch;
    switch (rows) {
        case 1: return dispatch_verify<1>(va, u, mode, stream);
        case 2: return dispatch_verify<2>(va, u, mode, stream);
        case 3: return dispatch_verify<3>(va, u, mode, stream);
        case 4: return dispatch_verify<4>(va, u, mode, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace kern
}  // namespace shmr
