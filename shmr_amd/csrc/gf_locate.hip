// GF(2^8) single-shard location kernels for gfx950 (MI355X / CDNA4): the second
// half of a scrub (shmr_ec_locate_batch_dev), behind the parity check of
// gf_compare.hip.
//
//   cand[j] bit t stays set  <=>  in every column of block j,
//   s_r == q[r][t] (x) s_0 for r = 1 .. R-1,   s = C (x) data ^ stored parity
//
// (locate_plan.hpp: what a damaged data shard t, and only it, leaves behind.)
// A read-only pass over the data and the stored parity of the first row group,
// R = min(p, 4) rows; the only stores are vector global atomics (AND) to the
// candidate bitmap, which the caller presets to all ones on the same stream.
//
//  * The tile loop is the parity check's (same ApplyArgs, plan staging, ring,
//    loads and modes), grid-strided over a bounded grid.  A tile first reads
//    its block's verify word -- a scalar load, the branch is workgroup-uniform
//    -- and goes on to the next tile unless every parity row differs: clean
//    blocks and blocks with one damaged parity shard cost one word per tile,
//    and a workgroup that meets no damaged block never stages a plan.
//  * Damaged tiles: the R syndrome chunks as the parity check forms them (one
//    16-byte chunk per lane: rate on damaged blocks is no goal), then per data
//    shard t one more mac of s_0 with the ratio tables and a compare.  A
//    column with a zero syndrome eliminates nobody, so nothing is masked.
//    One ballot per shard; one lane per wave ANDs the wave's survivors into
//    the block's bitmap, 32 shards at a time, where any were eliminated.
//  * MODE 0 full tiles, MODE 1 one bounds-checked partial tile per block,
//    MODE 2 byte-granular at any alignment: bytes at or past len are read by
//    neither side (both are zero there, as in the parity check).
//  * The resolve kernel: one thread per block, locate::resolve.
//  * Degraded blocks (shmr_ec_locate_checked_batch_dev): gf_locate_checked_kernel
//    and gf_locate_checked_resolve_kernel, launched per presence pattern behind
//    the checked reconstruct of gf_compare.hip.  The same tile loop as a
//    separate instantiation (locate_tiles<.., DEG>): the pattern's compare rows
//    D in place of C, its blocks by stride or list, its row mask in the skip
//    test; locate::resolve_checked.
//  * Two damaged shards (shmr_ec_locate_pair_batch_dev, p >= 4): the preset,
//    select, pair and pair resolve kernels further down, behind the chain above.
//
// Like the parity check kernels these are not gf_apply_kernel instantiations
// and not part of shmr_ec_kernel_inventory.
#include <hip/hip_runtime.h>

#include "gf_syndrome.hpp"
#include "locate_plan.hpp"

namespace shmr {
namespace kern {

namespace {

// The lane's syndrome chunk of every row: s[r] = XOR_t C[r][t] (x) data[t] ^ stored[r].
// Not gf_syndrome.hpp's tile: its stored-row loads in the ring's look-ahead
// slot cost this kernel 10 to 28 VGPRs, and with them the residency of its
// bounded grid -- measured 0.9 % on a CLEAN batch, the case this kernel is
// built for.  Here the stored rows are loaded behind the ring.
template <int R, int MODE>
__device__ __forceinline__ void locate_syndromes(const ApplyArgs& a, const Ctx& c, const uint8_t* ib, const uint8_t* ob,
                                                 uint64_t col, uint32_t (&s)[R][4]) {
    const uint64_t len = a.len;
#pragma unroll
    for (int r = 0; r < R; ++r)
#pragma unroll
        for (int j = 0; j < 4; ++j) s[r][j] = 0u;
    auto load = [&](u32x4& buf, uint32_t t) { buf = ld<MODE, 0>(ib + c.s_in_off[t], col, len); };
    auto consume = [&](const u32x4& buf, uint32_t t) {
        Tab tb[R];
        read_tabs<R>(c, t, tb);
        mac<R, 0>(s, buf, tb);
    };
    u32x4 ring[2];
    load(ring[0], 0);
    __builtin_amdgcn_sched_barrier(0);
    ring2_peeled(load, consume, a.k, ring);
#pragma unroll
    for (int r = 0; r < R; ++r) {
        const u32x4 par = ld<MODE, 0>(ob + c.s_out_off[r], col, len);
        s[r][0] ^= par.x;
        s[r][1] ^= par.y;
        s[r][2] ^= par.z;
        s[r][3] ^= par.w;
    }
}

// The parity check launch of row group 0 (rows = R) plus what location adds.
struct LocateArgs {
    ApplyArgs a;
    const uint8_t* qtab;        // the locate plan's tables, PermTab[k][R - 1] (gf256.hpp Codec::locate_plan)
    const uint32_t* mismatch;   // [nblk] verify words, complete before this launch
    uint32_t* cand;             // [nblk][words] candidate bitmaps, preset to all ones
    uint32_t all_rows;          // the verify word of a block whose every parity row differs
    uint32_t words;             // locate::bitmap_words(k)
};

// LDS: the staged encode plan of R rows (gf_tile.hpp stage_plan), then the ratio tables.
__host__ __device__ inline uint32_t ratio_tab_off(uint32_t k, uint32_t R) { return (plan_lds_bytes(k, R) + 15) & ~15u; }

// The tile loop of both locate kernels.  DEG (degraded blocks,
// shmr_ec_locate_checked_batch_dev): the launch names the blocks of one
// presence pattern -- blk_first + j * blk_stride, or blk_list[j] -- and the
// verify word and the bitmap are the block's own (index blk, not j); `a` is the
// pattern's compare-only checked plan, so inputs and stored rows go through its
// in_idx / out_idx offsets, and all_rows is the pattern's row mask.  A template
// flag, not a launch argument: the complete-block kernel carries none of it.
template <int R, int MODE, bool DEG>
__device__ __forceinline__ void locate_tiles(const LocateArgs& la, uint8_t* smem) {
    constexpr int TH = kThreads;
    constexpr int Q = R - 1;
    const ApplyArgs& a = la.a;
    const uint32_t k = a.k;
    Ctx c{}, qc{};
    bool staged = false;
    const uint64_t tb = uint64_t(TH) * 16;
    const uint32_t tpb = a.tiles_per_block;
    for (uint64_t tile = blockIdx.x; tile < a.ntiles; tile += gridDim.x) {
        const uint64_t j = tile / tpb, cc = tile - j * tpb;
        uint64_t w = j;   // the block's index in the batch
        if constexpr (DEG)
            w = a.blk_list ? uint64_t(as_const<cu32>(a.blk_list)[j]) : a.blk_first + j * a.blk_stride;
        if (as_const<cu32>(la.mismatch)[w] != la.all_rows) continue;   // clean, or stored rows only
        if (!staged) {   // (workgroup-uniform: every lane of the workgroup is here)
            stage_plan<R, TH, false>(a, a.plan, smem, c, 0);
            u32x4* s_q = reinterpret_cast<u32x4*>(smem + ratio_tab_off(k, R));
            const u32x4* gq = reinterpret_cast<const u32x4*>(la.qtab);
            for (uint32_t i = threadIdx.x; i < k * Q * 2; i += TH) s_q[i] = gq[i];
            qc.s_tab = s_q;
            __syncthreads();
            staged = true;
        }
        const uint64_t blk = DEG ? w : a.blk_first + j * a.blk_stride;
        const uint8_t* ib = a.in_base + blk * a.in_bpitch;
        const uint8_t* ob = a.out_base + blk * a.out_bpitch;
        uint32_t s[R][4];
        locate_syndromes<R, MODE>(a, c, ib, ob, a.col_base + cc * tb + uint64_t(threadIdx.x) * 16, s);
        uint32_t any = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) any |= s[r][0] | s[r][1] | s[r][2] | s[r][3];
        // every lane of the wave is here (no lane leaves a tile early); no barrier follows
        if (__builtin_amdgcn_ballot_w64(any != 0) == 0) continue;   // this wave's columns eliminate nobody
        const u32x4 s0{s[0][0], s[0][1], s[0][2], s[0][3]};
        uint32_t* bw = la.cand + w * la.words;
        uint32_t keep = 0xffffffffu;   // wave-uniform: the survivors among shards [t & ~31, t]
        for (uint32_t t = 0; t < k; ++t) {
            Tab tq[Q];
            read_tabs<Q>(qc, t, tq);
            uint32_t m[Q][4];
#pragma unroll
            for (int r = 0; r < Q; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) m[r][i] = 0u;
            mac<Q, 0>(m, s0, tq);
            uint32_t d = 0;
#pragma unroll
            for (int r = 0; r < Q; ++r)
#pragma unroll
                for (int i = 0; i < 4; ++i) d |= s[r + 1][i] ^ m[r][i];
            if (__builtin_amdgcn_ballot_w64(d != 0) != 0) keep &= ~(1u << (t & 31u));
            if ((t & 31u) == 31u || t + 1 == k) {
                if (keep != 0xffffffffu && (threadIdx.x & 63u) == 0) atomicAnd(bw + (t >> 5), keep);
                keep = 0xffffffffu;
            }
        }
    }
}

template <int R, int MODE>
__global__ __launch_bounds__(kThreads) void gf_locate_kernel(const LocateArgs la) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    locate_tiles<R, MODE, false>(la, smem);
}

template <int R, int MODE>
__global__ __launch_bounds__(kThreads) void gf_locate_checked_kernel(const LocateArgs la) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    locate_tiles<R, MODE, true>(la, smem);
}

// Every data shard of every block is a candidate until a tile rules it out.
// (A kernel: a hipMemsetAsync of 0xff did the same eagerly, but as a memset
// node of a captured graph it left other bytes behind on replay)
__global__ __launch_bounds__(kThreads) void gf_locate_preset_kernel(uint32_t* cand, uint64_t nwords) {
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < nwords; i += uint64_t(gridDim.x) * kThreads)
        cand[i] = 0xffffffffu;
}

__global__ __launch_bounds__(kThreads) void gf_locate_resolve_kernel(const uint32_t* mismatch, const uint32_t* cand,
                                                                     int32_t* located, uint64_t nblk, uint32_t k,
                                                                     uint32_t p) {
    const uint64_t b = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (b >= nblk) return;
    located[b] = locate::resolve(mismatch[b], cand + b * locate::bitmap_words(k), k, p);
}

// The degraded form: one thread per block of a pattern's launch (blocks as in
// locate_tiles<.., DEG>), locate::resolve_checked over the pattern's s, row
// mask and index maps.  idx: in_idx[k] then out_idx[s], the header of the
// pattern's compare-only plan image; null for s < 2, where the answer comes
// from the word alone and no map is read.
struct ResolveCheckedArgs {
    const uint32_t* mismatch;
    const uint32_t* cand;
    int32_t* located;
    const uint32_t* blk_list;
    uint64_t blk_first, blk_stride, nblk;
    const uint16_t* idx;
    uint32_t k, s, mask;
};

__global__ __launch_bounds__(kThreads) void gf_locate_checked_resolve_kernel(const ResolveCheckedArgs ra) {
    const uint64_t j = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (j >= ra.nblk) return;
    const uint64_t b = ra.blk_list ? uint64_t(ra.blk_list[j]) : ra.blk_first + j * ra.blk_stride;
    ra.located[b] = locate::resolve_checked(ra.mismatch[b], ra.cand + b * locate::bitmap_words(ra.k), ra.k, ra.s,
                                            ra.mask, ra.idx, ra.idx + ra.k);
}

// Workgroups of a locate launch: the tile loop strides over them.  A clean
// batch runs them all for one word per tile each, so the grid is bounded --
// the 256-lane workgroups a CU holds at once (2048 lanes), for every CU of the
// current device -- instead of one workgroup per tile.
constexpr uint64_t kLocateWgsPerCu = 8;
hipError_t locate_grid(uint64_t* grid) {
    int dev = 0, cus = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    e = hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev);
    if (e != hipSuccess) return e;
    *grid = uint64_t(cus < 1 ? 1 : cus) * kLocateWgsPerCu;
    return hipSuccess;
}

template <int R, int MODE, bool DEG>
hipError_t launch_locate_one(const LocateArgs& la, hipStream_t stream) {
    const ApplyArgs& a = la.a;
    const size_t lds = size_t(ratio_tab_off(a.k, R)) + size_t(a.k) * (R - 1) * 32;
    uint64_t wgs = 0;
    hipError_t e = locate_grid(&wgs);
    if (e != hipSuccess) return e;
    uint32_t grid = 0;
    // (by name, never through a function-pointer variable: gf_tile.hpp launch_one)
    if constexpr (DEG) {
        e = prepare_launch(reinterpret_cast<const void*>(gf_locate_checked_kernel<R, MODE>), lds, a.ntiles, &grid, wgs);
        if (e != hipSuccess || grid == 0) return e;
        hipLaunchKernelGGL((gf_locate_checked_kernel<R, MODE>), dim3(grid), dim3(kThreads), lds, stream, la);
    } else {
        e = prepare_launch(reinterpret_cast<const void*>(gf_locate_kernel<R, MODE>), lds, a.ntiles, &grid, wgs);
        if (e != hipSuccess || grid == 0) return e;
        hipLaunchKernelGGL((gf_locate_kernel<R, MODE>), dim3(grid), dim3(kThreads), lds, stream, la);
    }
    return hipGetLastError();
}

template <int R, bool DEG>
hipError_t dispatch_locate(const LocateArgs& la, int mode, hipStream_t stream) {
    switch (mode) {
        case 0: return launch_locate_one<R, 0, DEG>(la, stream);
        case 1: return launch_locate_one<R, 1, DEG>(la, stream);
        case 2: return launch_locate_one<R, 2, DEG>(la, stream);
        default: return hipErrorInvalidValue;
    }
}

template <bool DEG>
hipError_t dispatch_locate_rows(const LocateArgs& la, unsigned rows, int mode, hipStream_t stream) {
    switch (rows) {
        case 2: return dispatch_locate<2, DEG>(la, mode, stream);
        case 3: return dispatch_locate<3, DEG>(la, mode, stream);
        case 4: return dispatch_locate<4, DEG>(la, mode, stream);
        default: return hipErrorInvalidValue;
    }
}

// ---- two damaged shards (shmr_ec_locate_pair_batch_dev) --------------------
// Behind the verify -> locate -> resolve chain above, for codecs with p >= 4
// (locate_plan.hpp has the tests and the resolve rule):
//  * preset: the pair bitmaps to all ones, the worklist counter to zero;
//  * select: one thread per block; a block that no single shard explains, with
//    at least three differing rows and every row beyond the group differing, is
//    appended to the worklist (a vector global atomic add on the counter);
//  * the pair kernel: the locate tile loop over count x tiles_per_block tiles,
//    count read from device memory -- a clean batch costs the launch one word
//    per workgroup; the 4-row plan and the pair tables staged once; per tile the
//    4 syndrome chunks, then one ballot per candidate and one vector atomic AND
//    per group of 32 candidates where any were eliminated.  `skip`: a wave first
//    reads the group's bitmap word and leaves out candidates that are already
//    cleared (bits only ever clear: a stale word costs work, never an answer);
//  * resolve: one thread per block, locate::resolve_pair.

struct PairArgs {
    ApplyArgs a;             // the parity check launch of row group 0 (4 rows) over the whole batch
    const uint8_t* ptab;     // the pair plan's tables, PermTab[pair_coeff_count(k)] (gf256.hpp Codec::locate_pair_plan)
    const uint32_t* list;    // [count] the worklist: block indices, in any order
    const uint32_t* count;   // its length, complete before this launch
    uint32_t* pairs;         // [nblk][words] pair bitmaps, preset to all ones
    uint32_t words;          // locate::pair_bitmap_words(k)
    uint32_t skip;
};

// Whether rows v0, v1 of the syndrome are the coefficient multiples of row SRC
// (0 for every byte that agrees).
template <int SRC, int V0, int V1>
__device__ __forceinline__ uint32_t pair_ratio_diff(const uint32_t (&s)[4][4], const Tab (&tq)[2]) {
    uint32_t m[2][4];
#pragma unroll
    for (int r = 0; r < 2; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) m[r][i] = 0u;
    mac<2, 0>(m, u32x4{s[SRC][0], s[SRC][1], s[SRC][2], s[SRC][3]}, tq);
    uint32_t d = 0;
#pragma unroll
    for (int i = 0; i < 4; ++i) d |= (s[V0][i] ^ m[0][i]) | (s[V1][i] ^ m[1][i]);
    return d;
}

template <int MODE>
__global__ __launch_bounds__(kThreads) void gf_locate_pair_kernel(const PairArgs pa) {
    extern __shared__ __attribute__((aligned(16))) uint8_t smem[];
    constexpr int TH = kThreads, R = 4;
    const ApplyArgs& a = pa.a;
    const uint32_t k = a.k;
    const uint32_t tpb = a.tiles_per_block;
    uint64_t count = as_const<cu32>(pa.count)[0];
    if (count > a.nblk) count = a.nblk;   // (select appends a block once)
    const uint64_t ntiles = count * tpb;
    if (blockIdx.x >= ntiles) return;     // (workgroup-uniform; an empty worklist ends every workgroup here)
    Ctx c{}, qc{};
    stage_plan<R, TH, false>(a, a.plan, smem, c, 0);
    {
        u32x4* s_q = reinterpret_cast<u32x4*>(smem + ratio_tab_off(k, R));
        const u32x4* gq = reinterpret_cast<const u32x4*>(pa.ptab);
        for (uint32_t i = threadIdx.x; i < locate::pair_coeff_count(k) * 2; i += TH) s_q[i] = gq[i];
        qc.s_tab = s_q;
    }
    __syncthreads();
    const uint32_t ndd = locate::pair_dd_count(k), npairs = locate::pair_count(k);
    const uint64_t tb = uint64_t(TH) * 16;
    for (uint64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const uint64_t j = tile / tpb, cc = tile - j * tpb;
        uint64_t w = as_const<cu32>(pa.list)[j];
        if (w >= a.nblk) continue;
        const uint8_t* ib = a.in_base + w * a.in_bpitch;
        const uint8_t* ob = a.out_base + w * a.out_bpitch;
        uint32_t s[R][4];
        locate_syndromes<R, MODE>(a, c, ib, ob, a.col_base + cc * tb + uint64_t(threadIdx.x) * 16, s);
        uint32_t any = 0;
#pragma unroll
        for (int r = 0; r < R; ++r) any |= s[r][0] | s[r][1] | s[r][2] | s[r][3];
        // every lane of the wave is here (no lane leaves a tile early); no barrier follows
        if (__builtin_amdgcn_ballot_w64(any != 0) == 0) continue;   // this wave's columns eliminate nobody
        uint32_t* bw = pa.pairs + w * pa.words;
        uint32_t keep = 0xffffffffu;   // wave-uniform: the survivors among candidates [i & ~31, i]
        uint32_t live = 0xffffffffu;   // wave-uniform: the candidates of that group still to test
        for (uint32_t i = 0; i < npairs; ++i) {
            if ((i & 31u) == 0 && pa.skip)
                live = uint32_t(__builtin_amdgcn_readfirstlane(int(__atomic_load_n(bw + (i >> 5), __ATOMIC_RELAXED))));
            if ((live >> (i & 31u)) & 1u) {   // (a scalar branch: every lane of the wave takes it)
                uint32_t d;
                if (i < ndd) {   // data shards a < b: entries 4 i .. 4 i + 3 = al, be, ga, de
                    Tab t01[2], t23[2];
                    read_tabs<2>(qc, 2 * i, t01);
                    read_tabs<2>(qc, 2 * i + 1, t23);
                    const Tab of_s0[2] = {t01[0], t23[0]}, of_s1[2] = {t01[1], t23[1]};
                    uint32_t m[2][4];
#pragma unroll
                    for (int r = 0; r < 2; ++r)
#pragma unroll
                        for (int x = 0; x < 4; ++x) m[r][x] = 0u;
                    mac<2, 0>(m, u32x4{s[0][0], s[0][1], s[0][2], s[0][3]}, of_s0);
                    mac<2, 0>(m, u32x4{s[1][0], s[1][1], s[1][2], s[1][3]}, of_s1);
                    d = 0;
#pragma unroll
                    for (int x = 0; x < 4; ++x) d |= (s[2][x] ^ m[0][x]) | (s[3][x] ^ m[1][x]);
                } else {         // data shard a with parity shard k + r: entries 4 ndd + 2 (a * 4 + r), + 1
                    Tab tq[2];
                    read_tabs<2>(qc, 2 * ndd + (i - ndd), tq);
                    switch ((i - ndd) & 3u) {
                        case 0: d = pair_ratio_diff<1, 2, 3>(s, tq); break;
                        case 1: d = pair_ratio_diff<0, 2, 3>(s, tq); break;
                        case 2: d = pair_ratio_diff<0, 1, 3>(s, tq); break;
                        default: d = pair_ratio_diff<0, 1, 2>(s, tq); break;
                    }
                }
                if (__builtin_amdgcn_ballot_w64(d != 0) != 0) keep &= ~(1u << (i & 31u));
            }
            if ((i & 31u) == 31u || i + 1 == npairs) {
                if (keep != 0xffffffffu && (threadIdx.x & 63u) == 0) atomicAnd(bw + (i >> 5), keep);
                keep = 0xffffffffu;
            }
        }
    }
}

__global__ __launch_bounds__(kThreads) void gf_locate_pair_preset_kernel(uint32_t* pairs, uint64_t nwords,
                                                                         uint32_t* count) {
    if (blockIdx.x == 0 && threadIdx.x == 0) *count = 0u;
    for (uint64_t i = uint64_t(blockIdx.x) * kThreads + threadIdx.x; i < nwords; i += uint64_t(gridDim.x) * kThreads)
        pairs[i] = 0xffffffffu;
}

__global__ __launch_bounds__(kThreads) void gf_locate_pair_select_kernel(const uint32_t* mismatch, const int32_t* single,
                                                                         uint32_t* list, uint32_t* count,
                                                                         uint64_t nblk, uint32_t p) {
    const uint64_t b = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (b >= nblk) return;
    if (locate::pair_listed(mismatch[b], single[b], p)) list[atomicAdd(count, 1u)] = uint32_t(b);
}

__global__ __launch_bounds__(kThreads) void gf_locate_pair_resolve_kernel(const uint32_t* mismatch,
                                                                          const int32_t* single, const uint32_t* pairs,
                                                                          int32_t* located, uint64_t nblk, uint32_t k,
                                                                          uint32_t p) {
    const uint64_t b = uint64_t(blockIdx.x) * kThreads + threadIdx.x;
    if (b >= nblk) return;
    int32_t out[2];
    locate::resolve_pair(mismatch[b], single[b], pairs + b * locate::pair_bitmap_words(k), k, p, out);
    located[2 * b] = out[0];
    located[2 * b + 1] = out[1];
}

template <int MODE>
hipError_t launch_pair_one(const PairArgs& pa, hipStream_t stream) {
    const ApplyArgs& a = pa.a;
    // (locate_plan.hpp restates the staged plan's size for the host)
    if (ratio_tab_off(a.k, 4) != locate::pair_tab_off(a.k)) return hipErrorInvalidValue;
    const size_t lds = locate::pair_lds_bytes(a.k);
    uint64_t wgs = 0;
    hipError_t e = locate_grid(&wgs);
    if (e != hipSuccess) return e;
    uint32_t grid = 0;
    e = prepare_launch(reinterpret_cast<const void*>(gf_locate_pair_kernel<MODE>), lds, a.ntiles, &grid, wgs);
    if (e != hipSuccess || grid == 0) return e;
    hipLaunchKernelGGL((gf_locate_pair_kernel<MODE>), dim3(grid), dim3(kThreads), lds, stream, pa);
    return hipGetLastError();
}

}  // namespace

hipError_t launch_locate_pair_preset(uint32_t* pairs, uint32_t* count, uint64_t nblk, unsigned k, hipStream_t stream) {
    const uint64_t nwords = nblk * locate::pair_bitmap_words(k);
    uint64_t grid = (nwords + kThreads - 1) / kThreads, cap = 0;
    const hipError_t ge = locate_grid(&cap);
    if (ge != hipSuccess) return ge;
    if (grid > cap) grid = cap;
    if (grid == 0) grid = 1;   // the counter
    hipLaunchKernelGGL(gf_locate_pair_preset_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, pairs, nwords,
                       count);
    return hipGetLastError();
}

hipError_t launch_locate_pair_select(const uint32_t* mismatch, const int32_t* single, uint32_t* list, uint32_t* count,
                                     uint64_t nblk, unsigned p, hipStream_t stream) {
    const uint64_t grid = (nblk + kThreads - 1) / kThreads;
    if (grid == 0) return hipSuccess;
    if (nblk > 0xffffffffull) return hipErrorInvalidValue;   // the worklist is 32-bit
    hipLaunchKernelGGL(gf_locate_pair_select_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, mismatch, single,
                       list, count, nblk, uint32_t(p));
    return hipGetLastError();
}

hipError_t launch_locate_pair(const ApplyArgs& a, const uint8_t* ptab, const uint32_t* list, const uint32_t* count,
                              uint32_t* pairs, int mode, bool skip, hipStream_t stream) {
    if (a.row0 != 0 || a.m < 4 || !locate::pair_supported(a.k, a.m)) return hipErrorInvalidValue;
    PairArgs pa;
    pa.a = a;
    pa.ptab = ptab;
    pa.list = list;
    pa.count = count;
    pa.pairs = pairs;
    pa.words = locate::pair_bitmap_words(a.k);
    pa.skip = skip ? 1u : 0u;
    switch (mode) {
        case 0: return launch_pair_one<0>(pa, stream);
        case 1: return launch_pair_one<1>(pa, stream);
        case 2: return launch_pair_one<2>(pa, stream);
        default: return hipErrorInvalidValue;
    }
}

hipError_t launch_locate_pair_resolve(const uint32_t* mismatch, const int32_t* single, const uint32_t* pairs,
                                      int32_t* located, uint64_t nblk, unsigned k, unsigned p, hipStream_t stream) {
    const uint64_t grid = (nblk + kThreads - 1) / kThreads;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gf_locate_pair_resolve_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, mismatch, single,
                       pairs, located, nblk, uint32_t(k), uint32_t(p));
    return hipGetLastError();
}

hipError_t launch_locate(const ApplyArgs& a, const uint8_t* qtab, const uint32_t* mismatch, uint32_t* cand,
                         unsigned rows, unsigned p, int mode, hipStream_t stream) {
    LocateArgs la;
    la.a = a;
    la.qtab = qtab;
    la.mismatch = mismatch;
    la.cand = cand;
    la.all_rows = locate::all_rows(p);
    la.words = locate::bitmap_words(a.k);
    return dispatch_locate_rows<false>(la, rows, mode, stream);
}

hipError_t launch_locate_checked(const ApplyArgs& a, const uint8_t* qtab, const uint32_t* mismatch, uint32_t* cand,
                                 unsigned rows, uint32_t row_mask, int mode, hipStream_t stream) {
    if (a.row0 != 0 || rows > a.m) return hipErrorInvalidValue;   // the first rows of the pattern's compare rows
    LocateArgs la;
    la.a = a;
    la.qtab = qtab;
    la.mismatch = mismatch;
    la.cand = cand;
    la.all_rows = row_mask;
    la.words = locate::bitmap_words(a.k);
    return dispatch_locate_rows<true>(la, rows, mode, stream);
}

hipError_t launch_locate_checked_resolve(const ApplyArgs& a, const uint32_t* mismatch, const uint32_t* cand,
                                         int32_t* located, const uint16_t* idx, unsigned s, uint32_t row_mask,
                                         hipStream_t stream) {
    const uint64_t grid = (a.nblk + kThreads - 1) / kThreads;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull || (s >= 2 && !idx)) return hipErrorInvalidValue;
    ResolveCheckedArgs ra;
    ra.mismatch = mismatch;
    ra.cand = cand;
    ra.located = located;
    ra.blk_list = a.blk_list;
    ra.blk_first = a.blk_first;
    ra.blk_stride = a.blk_stride;
    ra.nblk = a.nblk;
    ra.idx = idx;
    ra.k = a.k;
    ra.s = s;
    ra.mask = row_mask;
    hipLaunchKernelGGL(gf_locate_checked_resolve_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, ra);
    return hipGetLastError();
}

hipError_t launch_locate_preset(uint32_t* cand, uint64_t nblk, unsigned k, hipStream_t stream) {
    const uint64_t nwords = nblk * locate::bitmap_words(k);
    uint64_t grid = (nwords + kThreads - 1) / kThreads, cap = 0;
    if (grid == 0) return hipSuccess;
    const hipError_t ge = locate_grid(&cap);
    if (ge != hipSuccess) return ge;
    if (grid > cap) grid = cap;
    hipLaunchKernelGGL(gf_locate_preset_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, cand, nwords);
    return hipGetLastError();
}

hipError_t launch_locate_resolve(const uint32_t* mismatch, const uint32_t* cand, int32_t* located, uint64_t nblk,
                                 unsigned k, unsigned p, hipStream_t stream) {
    const uint64_t grid = (nblk + kThreads - 1) / kThreads;
    if (grid == 0) return hipSuccess;
    if (grid > 0x7fffffffull) return hipErrorInvalidValue;
    hipLaunchKernelGGL(gf_locate_resolve_kernel, dim3(uint32_t(grid)), dim3(kThreads), 0, stream, mismatch, cand,
                       located, nblk, uint32_t(k), uint32_t(p));
    return hipGetLastError();
}

}  // namespace kern
}  // namespace shmr
