// GF(2^8) checked-reconstruct kernel for gfx950 (MI355X / CDNA4):
// shmr_ec_reconstruct_checked_batch_dev.
//
// One pass over the first k present shards of a degraded block does both jobs:
//
//   rows [0, nstore) of the launch group:  out[r][col] = XOR_t C[r][t] (x) in[t][col]
//       stored to the absent shard's own slot, the bytes a reconstruct writes;
//   rows [nstore, R):  mismatch[blk] |= 1 << bits[r]  where the stored bytes of
//       the surplus parity shard differ from XOR_t C[r][t] (x) in[t][col] at
//       some col in [0, len)
//
// so the surplus shards (the present ones a reconstruct never looks at) cost
// s * len more reads instead of a second pass over the k inputs.
//
//  * The tile is gf_verify.hip's: plan staging, the depth-2 register ring over
//    the k inputs, mac, and the stored chunks of the compare rows loaded in the
//    ring's peeled look-ahead slot.  nstore is a kernel argument (workgroup-
//    uniform: every branch on it is a scalar branch); only compare rows issue
//    loads of out addresses, only stored rows issue stores.
//  * The bit of a compare row is its parity row index (out_idx - k), not its
//    row number in the plan; the group's <= 4 positions travel in the launch
//    arguments.  One ballot per wave; on a difference one lane ORs the wave's
//    mask into the block's word with a vector global atomic, as verify does.
//  * The word index is the block's index in the batch: blk_first + j *
//    blk_stride, or blk_list[j] for a pattern whose blocks are no arithmetic
//    sequence.
//  * MODE 0 full tiles, MODE 1 one bounds-checked partial tile per block,
//    MODE 2 byte-granular at any alignment (gf_tile.hpp ld / st): bytes at or
//    past len are neither read, stored nor compared.
//  * In place: inputs and surplus shards are present shards, stores go to
//    absent shards only, so what a launch reads and what it writes are
//    disjoint, and later row groups of the same block read present shards only
//    -- never a byte an earlier group stored.
//
// Not gf_apply_kernel or gf_verify_kernel instantiations and not part of
// shmr_ec_kernel_inventory.
#include <hip/hip_runtime.h>

#include "gf_tile.hpp"

namespace shmr {
namespace kern {

namespace {

struct CheckArgs {
    ApplyArgs a;
    uint32_t* mismatch;                  // word blk for batch block blk
    uint32_t nstore;                     // rows [0, nstore) are stored, [nstore, R) compared
    uint32_t bits[kMaxRowsPerLaunch];    // bit position of row r's difference (compare rows)
};

// One tile; returns the lane's difference flags of the compare rows ORed
// together (nz[r] per row, 0 for a stored row).
template <int R, int U, int MODE, int F>
__device__ __forceinline__ uint32_t check_tile(const ApplyArgs& a, const Ctx& c, uint32_t nstore, const uint8_t* ib,
                                               uint8_t* ob, uint64_t col0, uint32_t (&nz)[R]) {
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
    // The stored chunks of the surplus shards (compare rows only: a stored
    // row's slot is an absent shard and is never read).
    u32x4 par[R][U];
    auto load_surplus = [&]() {
#pragma unroll
        for (int r = 0; r < R; ++r) {
#pragma unroll
            for (int u = 0; u < U; ++u) par[r][u] = u32x4{0u, 0u, 0u, 0u};
            if (uint32_t(r) >= nstore) {
                const uint8_t* base = ob + c.s_out_off[r];
#pragma unroll
                for (int u = 0; u < U; ++u)
                    par[r][u] = ld<MODE, F>(base, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len);
            }
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
    // One or two inputs are left; the surplus loads take the look-ahead slot
    // behind the last input load (the branch is uniform).
    if (t + 1 < k) {
        load(ring[1], t + 1);
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
        __builtin_amdgcn_sched_barrier(0);
        load_surplus();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[1], t + 1);
    } else {
        load_surplus();
        __builtin_amdgcn_sched_barrier(0);
        consume(ring[0], t);
    }
    __builtin_amdgcn_sched_barrier(0);

    uint32_t any = 0;
#pragma unroll
    for (int r = 0; r < R; ++r) {
        nz[r] = 0;
        if (uint32_t(r) < nstore) {
            uint8_t* o = ob + c.s_out_off[r];
#pragma unroll
            for (int u = 0; u < U; ++u)
                st<MODE, F>(o, col0 + slot_chunk<U, TH, F>(u, tid) * 16, len,
                            u32x4{acc[u][r][0], acc[u][r][1], acc[u][r][2], acc[u][r][3]});
        } else {
            uint32_t d = 0;
#pragma unroll
            for (int u = 0; u < U; ++u)
                d |= (par[r][u].x ^ acc[u][r][0]) | (par[r][u].y ^ acc[u][r][1]) | (par[r][u].z ^ acc[u][r][2]) |
                     (par[r][u].w ^ acc[u][r][3]);
            nz[r] = d;
            any |= d;
        }
    }
    return any;
}

template <int R, int U, int MODE, int F>
__global__ __launch_bounds__(kThreads) void gf_check_kernel(const CheckArgs ca) {
    constexpr int TH = kThreads;
    const ApplyArgs& a = ca.a;
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    Ctx c{};
    stage_plan<R, TH, false>(a, a.plan, smem, c, 0);
    __syncthreads();
    const uint64_t tb = uint64_t(TH) * 16 * U;
    const uint32_t tpb = a.tiles_per_block;
    const uint32_t nstore = ca.nstore;
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t j = tile / tpb, cc = tile - j * tpb;
        const uint64_t blk = a.blk_list ? uint64_t(as_const<cu32>(a.blk_list)[j]) : a.blk_first + j * a.blk_stride;
        const uint8_t* ib = a.in_base + blk * a.in_bpitch;
        uint8_t* ob = a.out_base + blk * a.out_bpitch;
        uint32_t nz[R];
        const uint32_t any = check_tile<R, U, MODE, F>(a, c, nstore, ib, ob, a.col_base + cc * tb, nz);
        // every lane of the wave is here (no lane leaves a tile early)
        if (__builtin_amdgcn_ballot_w64(any != 0) != 0) {
            uint32_t mask = 0;
#pragma unroll
            for (int r = 0; r < R; ++r)
                if (__builtin_amdgcn_ballot_w64(nz[r] != 0) != 0) mask |= 1u << (ca.bits[r] & 31u);
            if ((threadIdx.x & 63u) == 0) atomicOr(ca.mismatch + blk, mask);
        }
    }
}

template <int R, int U, int MODE, int F>
hipError_t launch_check_one(const CheckArgs& ca, hipStream_t stream) {
    const ApplyArgs& a = ca.a;
    const size_t lds = size_t(a.k) * R * 32 + size_t(a.k) * 8 + size_t(R) * 8;
    if (lds > 64 * 1024) {
        hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void*>(gf_check_kernel<R, U, MODE, F>),
                                           hipFuncAttributeMaxDynamicSharedMemorySize, int(lds));
        if (e != hipSuccess) return e;
    }
    uint64_t grid = a.ntiles;   // one workgroup per tile, as the verify launches
    if (grid > 0x7fffffffull) grid = 0x7fffffffull;
    if (grid == 0) return hipSuccess;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    hipLaunchKernelGGL((gf_check_kernel<R, U, MODE, F>), dim3(uint32_t(grid)), dim3(kThreads), lds, stream, ca);
    return hipGetLastError();
}

// Full tiles: the in-place reconstruct's loads and stores (nontemporal), 4 KiB
// tiles (U = 1: a second tile size only once measured); the tail
// and the byte-granular kernels load and store plainly, as the reconstruct's do.
constexpr int kCheckFullFlags = kNtLoad | kNtStore | kDepth2;

template <int R>
hipError_t dispatch_check(const CheckArgs& ca, int mode, hipStream_t stream) {
    switch (mode) {
        case 0: return launch_check_one<R, 1, 0, kCheckFullFlags>(ca, stream);
        case 1: return launch_check_one<R, 1, 1, 0>(ca, stream);
        case 2: return launch_check_one<R, 1, 2, 0>(ca, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_check(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, unsigned nstore, const uint32_t* bits,
                        int mode, hipStream_t stream) {
    if (rows < 1 || rows > kMaxRowsPerLaunch || nstore > rows) return hipErrorInvalidValue;
    CheckArgs ca;
    ca.a = a;
    ca.mismatch = mismatch;
    ca.nstore = nstore;
    for (unsigned r = 0; r < kMaxRowsPerLaunch; ++r) ca.bits[r] = r < rows ? bits[r] : 0u;
    switch (rows) {
        case 1: return dispatch_check<1>(ca, mode, stream);
        case 2: return dispatch_check<2>(ca, mode, stream);
        case 3: return dispatch_check<3>(ca, mode, stream);
        default: return dispatch_check<4>(ca, mode, stream);
    }
}

}  // namespace kern
}  // namespace shmr
