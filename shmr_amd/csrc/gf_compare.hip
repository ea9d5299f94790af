// GF(2^8) compare kernels for gfx950 (MI355X / CDNA4): the parity check
// (ReedSolomon::verify) and the checked reconstruct
// (shmr_ec_reconstruct_checked_batch_dev).  Both run one body over the compare
// tile of gf_syndrome.hpp:
//
//   rows [0, nstore) of the launch group:  out[r][col] = XOR_t C[r][t] (x) in[t][col]
//       stored to the row's own slot (checked reconstruct only: an absent
//       shard, the bytes a reconstruct writes);
//   rows [nstore, R):  mismatch[blk] |= 1 << bits[r]  where the stored bytes of
//       the row's slot differ from XOR_t C[r][t] (x) in[t][col] at some col in
//       [0, len)
//
//  * gf_verify_kernel: nstore = 0, compiled without the store path -- the
//    encode tile with its stores replaced by loads and a compare: an all-read
//    kernel, algorithmic traffic (k + R) * len per block and launch group,
//    nothing written for a block that is a codeword.
//  * gf_check_kernel: one pass over the first k present shards of a degraded
//    block rebuilds the absent shards and compares the surplus ones (the
//    present shards a reconstruct never looks at), s * len more reads instead of
//    a second pass over the k inputs.  nstore is a kernel argument; only
//    compare rows issue loads of out addresses, only stored rows issue stores.
//    In place: inputs and surplus shards are present shards, stores go to
//    absent shards only, so what a launch reads and what it writes are
//    disjoint, and later row groups of the same block read present shards only
//    -- never a byte an earlier group stored.
//  * The bit of a compare row travels in the launch arguments (<= 4 per
//    group): the parity row index, saturating at 31.  The word index is the
//    block's index in the batch: blk_first + j * blk_stride, or blk_list[j] for
//    a pattern whose blocks are no arithmetic sequence.
//
// These kernels are not gf_apply_kernel instantiations and not part of
// shmr_ec_kernel_inventory (which lists what encode and reconstruct dispatch).
#include <hip/hip_runtime.h>

#include "gf_syndrome.hpp"

namespace shmr {
namespace kern {

namespace {

struct CompareArgs {
    ApplyArgs a;                         // single plan, no pointer table, no segments
    uint32_t* mismatch;                  // word blk for batch block blk
    uint32_t nstore;                     // rows [0, nstore) are stored, [nstore, R) compared
    uint32_t bits[kMaxRowsPerLaunch];    // bit position of row r's difference (compare rows)
};

template <int R, int U, int MODE, int F, bool STORES>
__device__ __forceinline__ void compare_tiles(const CompareArgs& ca, uint8_t* smem) {
    constexpr int TH = kThreads;
    const ApplyArgs& a = ca.a;
    Ctx c{};
    stage_plan<R, TH, false>(a, a.plan, smem, c, 0);
    __syncthreads();
    const uint64_t tb = uint64_t(TH) * 16 * U;
    const uint32_t tpb = a.tiles_per_block;
    const uint32_t nstore = ca.nstore;
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t j = tile / tpb, cc = tile - j * tpb;
        // (block lists: the checked reconstruct only; launch_verify refuses one)
        const uint64_t blk = STORES && a.blk_list ? uint64_t(as_const<cu32>(a.blk_list)[j])
                                                  : a.blk_first + j * a.blk_stride;
        uint32_t s[U][R][4], nz[R];
        syndrome_tile<R, U, MODE, F, STORES>(a, c, nstore, a.in_base + blk * a.in_bpitch,
                                             a.out_base + blk * a.out_bpitch, a.col_base + cc * tb, s);
        // every lane of the wave is here (no lane leaves a tile early)
        report_rows<R>(row_flags<R, U>(s, nz), nz, ca.bits, ca.mismatch + blk);
    }
}

template <int R, int U, int MODE, int F>
__global__ __launch_bounds__(kThreads) void gf_verify_kernel(const CompareArgs ca) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    compare_tiles<R, U, MODE, F, false>(ca, smem);
}

template <int R, int U, int MODE, int F>
__global__ __launch_bounds__(kThreads) void gf_check_kernel(const CompareArgs ca) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    compare_tiles<R, U, MODE, F, true>(ca, smem);
}

// One workgroup per tile, as the encode launches.  (The launches are written
// out by kernel name, never through a function-pointer variable: gf_tile.hpp
// launch_one.)
template <int R, int U, int MODE, int F>
hipError_t launch_verify_one(const CompareArgs& ca, hipStream_t stream) {
    const size_t lds = plan_lds_bytes(ca.a.k, R);
    uint32_t grid = 0;
    const hipError_t e =
        prepare_launch(reinterpret_cast<const void*>(gf_verify_kernel<R, U, MODE, F>), lds, ca.a.ntiles, &grid);
    if (e != hipSuccess || grid == 0) return e;
    hipLaunchKernelGGL((gf_verify_kernel<R, U, MODE, F>), dim3(grid), dim3(kThreads), lds, stream, ca);
    return hipGetLastError();
}

template <int R, int U, int MODE, int F>
hipError_t launch_check_one(const CompareArgs& ca, hipStream_t stream) {
    const size_t lds = plan_lds_bytes(ca.a.k, R);
    uint32_t grid = 0;
    const hipError_t e =
        prepare_launch(reinterpret_cast<const void*>(gf_check_kernel<R, U, MODE, F>), lds, ca.a.ntiles, &grid);
    if (e != hipSuccess || grid == 0) return e;
    hipLaunchKernelGGL((gf_check_kernel<R, U, MODE, F>), dim3(grid), dim3(kThreads), lds, stream, ca);
    return hipGetLastError();
}

// Full tiles: the encode policy's loads (nontemporal) and, for the checked
// reconstruct, the in-place reconstruct's stores (nontemporal); the tail and
// the byte-granular kernels load and store plainly, as the encode's and the
// reconstruct's do.  Verify: the product library carries the full-tile kernel
// of verify_chunks(R) only, the tools build both tile sizes (tools/verify_ab.py
// --u-ab).  Check: 4 KiB tiles (U = 1: a second tile size only once measured,
// DESIGN.md §6).
constexpr int kFullFlags = kNtLoad | kDepth2;
constexpr int kCheckFullFlags = kNtLoad | kNtStore | kDepth2;
#ifdef SHMR_EC_TOOLS
constexpr bool kBothTileSizes = true;
#else
constexpr bool kBothTileSizes = false;
#endif

template <int R>
hipError_t dispatch_verify(const CompareArgs& ca, int u, int mode, hipStream_t stream) {
    switch (mode) {
        case 0:
            if constexpr (kBothTileSizes || verify_chunks(R) == 2)
                if (u == 2) return launch_verify_one<R, 2, 0, kFullFlags | kWaveRun>(ca, stream);
            if constexpr (kBothTileSizes || verify_chunks(R) == 1)
                if (u == 1) return launch_verify_one<R, 1, 0, kFullFlags>(ca, stream);
            return hipErrorInvalidValue;
        case 1: return launch_verify_one<R, 1, 1, 0>(ca, stream);
        case 2: return launch_verify_one<R, 1, 2, 0>(ca, stream);
        default: return hipErrorInvalidValue;
    }
}

template <int R>
hipError_t dispatch_check(const CompareArgs& ca, int mode, hipStream_t stream) {
    switch (mode) {
        case 0: return launch_check_one<R, 1, 0, kCheckFullFlags>(ca, stream);
        case 1: return launch_check_one<R, 1, 1, 0>(ca, stream);
        case 2: return launch_check_one<R, 1, 2, 0>(ca, stream);
        default: return hipErrorInvalidValue;
    }
}

}  // namespace

hipError_t launch_verify(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, int u, int mode, hipStream_t stream) {
    if (a.blk_list) return hipErrorInvalidValue;   // the contract (gf_apply.hpp): strided blocks only
    CompareArgs ca;
    ca.a = a;
    ca.mismatch = mismatch;
    ca.nstore = 0;
    for (unsigned r = 0; r < kMaxRowsPerLaunch; ++r) ca.bits[r] = a.row0 + r < 31u ? a.row0 + r : 31u;
    switch (rows) {
        case 1: return dispatch_verify<1>(ca, u, mode, stream);
        case 2: return dispatch_verify<2>(ca, u, mode, stream);
        case 3: return dispatch_verify<3>(ca, u, mode, stream);
        case 4: return dispatch_verify<4>(ca, u, mode, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_check(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, unsigned nstore, const uint32_t* bits,
                        int mode, hipStream_t stream) {
    if (rows < 1 || rows > kMaxRowsPerLaunch || nstore > rows) return hipErrorInvalidValue;
    CompareArgs ca;
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
