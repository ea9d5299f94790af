// Launch interface of the gfx950 GF(2^8) matrix-apply kernel (gf_apply.hip).
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace shmr {
namespace update {
struct DevPiece;   // update_plan.hpp
}
namespace read {
struct DevPiece;   // read_plan.hpp
}
namespace degraded {
struct DevPiece;   // update_degraded_plan.hpp
}
namespace kern {

constexpr int kThreads = 256;                          // lanes per workgroup (4 waves)
// A tile = kThreads * 16 * U bytes of columns of one block; U (16-byte chunks
// per lane per shard) is a launch parameter in {1, 2, 4}.
inline uint64_t tile_bytes(int u, int threads = kThreads) { return uint64_t(threads) * 16 * uint64_t(u); }
constexpr unsigned kMaxRowsPerLaunch = 4;

// Multi-plan launches described in the kernel arguments (no table upload):
// launch blocks j in [start, start + count) of a segment are blocks
// first + (j - start) * stride, all using `plan` (a device plan image).
#ifndef SHMR_MAX_SEGS
#define SHMR_MAX_SEGS 32
#endif
constexpr unsigned kMaxSegs = SHMR_MAX_SEGS;
struct Seg {
    uint32_t start;
    uint32_t first;
    uint32_t stride;
    uint32_t pad_;
    const uint8_t* plan;
};

// Shard t of block b lives at in_base + b * in_bpitch + in_idx[t] * in_spitch,
// output r of block b at out_base + b * out_bpitch + (out_idx[row0 + r] - out_bias) * out_spitch.
// Blocks of a launch: blk_list[j] if blk_list, else blk_first + j * blk_stride.
struct ApplyArgs {
    const uint8_t* in_base;
    uint8_t* out_base;
    uint64_t in_bpitch, in_spitch;
    uint64_t out_bpitch, out_spitch;
    const uint32_t* blk_list;
    uint64_t blk_first, blk_stride;
    uint64_t nblk;
    uint64_t len;            // shard length in bytes
    uint64_t col_base;       // column of tile 0 (tail launches start at the last partial tile)
    uint64_t ntiles;         // nblk * tiles_per_block
    uint32_t tiles_per_block;
    uint32_t k;              // inputs per block
    uint32_t m;              // rows in the plan image
    uint32_t row0;           // first plan row handled by this launch
    uint32_t out_bias;       // output r at (out_idx[row0 + r] - out_bias) * out_spitch
    const uint8_t* plan;     // device plan image (gf256.hpp Plan::image), single-plan launches
    // Multi-plan launches (plan_table != nullptr): block j uses plan
    // plan_table[blk_plan[j]]; every plan of a launch has the same k and m.
    const uint8_t* const* plan_table;
    const uint16_t* blk_plan;
    uint32_t tab_off;        // byte offset of the PermTab array in the image
    uint32_t in_identity;    // every plan of the launch reads input t from shard t (in_idx[t] == t)
    // Shard-pointer launches (shard_ptrs != nullptr; in/out bases and pitches
    // are then 0): block b's row shard_ptrs[b * total ..] is in PLAN ORDER --
    // input t at [t], output row r (plan row) at [k + r] -- so no address
    // depends on a load of the plan's in_idx / out_idx (the host permutes the
    // caller's shard-index table: ec_core permute_ptr_rows).  E.g. per-shard
    // device buffers, or Block-Cache buffers in mapped (pinned) host memory,
    // which the kernel reads and writes across PCIe without a staging copy.
    const uint64_t* shard_ptrs;
    uint32_t total;
    // Fused tails (kernels compiled with the fused-tail flag): the first
    // lead_tails tiles of the grid are the partial last tiles of blocks
    // j = 0 .. lead_tails-1 (column col_base + tiles_per_block * tile bytes),
    // run bounds-checked; tile lead_tails + t is full tile t.  Leading, so the
    // latency-bound partial tiles start first and finish under the full ones.
    uint64_t lead_tails;
    // Segment launches (nseg > 0; plan / plan_table / blk_list unused): block
    // j of the launch is found in segs[0 .. nseg) (ascending start, segs[0].start = 0).
    uint32_t nseg;
    Seg segs[kMaxSegs];
};

// Kernel variant flags (template parameter F of gf_apply_kernel).  The values
// are part of the kernels' mangled names: never renumber.
constexpr int kNtLoad = 1;       // nontemporal loads
constexpr int kNtStore = 2;      // nontemporal stores
constexpr int kOcc8 = 8;         // tools: ask for 8 waves / SIMD (<= 64 VGPRs)
constexpr int kDiagXor = 16;     // tools: XOR without GF multiply (wrong results)
constexpr int kTh128 = 32;       // tools: 128-lane workgroups (default 256)
constexpr int kTh512 = 64;       // tools: 512-lane workgroups
constexpr int kDepth5 = 128;     // tools: 4 shards of loads in flight (default 2)
constexpr int kDepth9 = 256;     // tools: 8 shards of loads in flight
constexpr int kDepth2 = 512;     // 1 shard of loads in flight
constexpr int kDepth1 = 1024;    // tools: no look-ahead (load, wait, multiply)
constexpr int kEarly = 1 << 16;  // first data loads issued before the plan's LDS staging completes
constexpr int kSPre = 1 << 17;   // tools: tables + offsets by scalar loads one shard ahead, no LDS
constexpr int kFuse = 1 << 18;   // leading partial tiles (ApplyArgs::lead_tails) in a MODE 0 launch; a
                                 // separate instantiation: the bounds-checked path costs 4-7 VGPRs
// Launch forms a full-tile (MODE 0) kernel supports only when compiled with
// the flag, so the lean encode kernel carries none of their code (measured:
// the runtime checks alone cost the RS(8,3) encode 1.3 %).  The tail and
// byte-granular kernels (MODE 1, 2) always support both.
constexpr int kPtrs = 1 << 19;   // shard-pointer tables (ApplyArgs::shard_ptrs)
constexpr int kSegs = 1 << 20;   // segment launches (ApplyArgs::segs)
constexpr int kGlds = 1 << 21;   // tools: input ring in LDS filled by LDS-DMA
// GF math one dword at a time: a scheduling fence after each of a lane's four
// dwords keeps the scheduler from computing every perm of a 16-byte chunk
// before the first XOR (48 live temporaries at R = 4), trading ILP inside a
// wave for registers (more waves per SIMD).
constexpr int kSerial = 1 << 22;
// Stores with the sc1 cache policy instead of nontemporal (compact rebuilt-
// shard outputs: a separate, densely written array; raw buffer stores)
constexpr int kSc1Store = 1 << 23;
constexpr int kRealign = 1 << 24;   // tools: misaligned shards by aligned loads realigned across lanes (DPP)
// The depth-2 ring with its tail peeled: no look-ahead load past the last
// shard (the plain ring re-reads shard k-1 there: one extra wave load per
// shard run, an L2 hit) and still no load behind a branch inside the loop
constexpr int kPeel = 1 << 25;
// U > 1 slots of a lane in wave-contiguous runs (chunk (w * U + u) * 64 +
// lane: each wave covers one contiguous U KiB run) instead of workgroup-
// strided slots (u * TH + tid)
constexpr int kWaveRun = 1 << 26;
constexpr int kStAlign = 1 << 27;   // tools: misaligned output rows stored aligned (DPP-shifted)
constexpr int kXcd = 1 << 28;       // tools: XCD-grouped tile order
// tools: two neighbouring tiles per workgroup (one workgroup per pair): the
// second tile of a block finds the block's pointer-table row in the scalar
// cache its first tile filled
constexpr int kPair = 1 << 29;
// Bits 12-15: occupancy target in waves per SIMD (0 = compiler's choice);
// the register allocator must then fit 512 / target VGPRs.
constexpr int kOccShift = 12;

// A full-tile kernel variant (MODE 0): the launch policy's choice (below), or
// a measurement variant of the tools build (knobs, ec_core.cpp).
struct Variant {
    int u = 1;               // 16-byte chunks per lane per shard (1, 2, 4)
    bool nt_load = false;    // nontemporal loads
    bool nt_store = false;   // nontemporal stores
    bool occ8 = false;       // __launch_bounds__ for 8 waves / SIMD
    bool diag = false;       // diagnostics: XOR-only (wrong results)
    int threads = kThreads;  // lanes per workgroup (128, 256, 512)
    int depth = 3;           // register ring depth: shards of loads in flight + 1 (1, 2, 3, 5, 9)
    int wgs_per_cu = 0;      // > 0: cap resident workgroups per CU (LDS padding; not a template flag)
    int occ = 0;             // > 0: register budget for this many waves per SIMD (6, 7)
    bool early = false;      // first data loads before the plan's LDS staging completes
    bool spre = false;       // tables/offsets by scalar loads one shard ahead (no LDS)
    bool fuse_tail = false;  // partial last tiles inside the full-tile launch (ApplyArgs::lead_tails)
    bool ptrs = false;       // full-tile kernel that reads shard-pointer tables
    bool segs = false;       // full-tile kernel that takes segment launches
    bool glds = false;       // input ring in LDS filled by LDS-DMA (depth = slots; full tiles only)
    bool serial = false;     // GF math one dword at a time (fewer live registers, more waves)
    bool sc1_store = false;  // stores with the sc1 cache policy instead of nontemporal
    bool realign = false;    // misaligned shards: aligned loads realigned across lanes (DPP), unaligned stores
    bool peel = false;       // depth-2 ring with the tail peeled (no look-ahead load past the last shard)
    bool wave_run = false;   // U > 1 slots in wave-contiguous runs
    bool st_align = false;   // misaligned output rows: aligned stores realigned across lanes (tools)
    bool xcd = false;        // XCD-grouped tile order: neighbouring tiles on one XCD's L2 (tools)
    bool pair = false;       // two neighbouring tiles per workgroup (tools)
};

// Template flags of a variant (its instantiation; wgs_per_cu is a launch
// parameter, not a flag).
constexpr int variant_flags(const Variant& v) {
    return (v.nt_load ? kNtLoad : 0) | (v.nt_store ? kNtStore : 0) | (v.occ8 ? kOcc8 : 0) |
           (v.diag ? kDiagXor : 0) | (v.threads == 128 ? kTh128 : 0) | (v.threads == 512 ? kTh512 : 0) |
           (v.depth == 5 ? kDepth5 : 0) | (v.depth == 9 ? kDepth9 : 0) | (v.depth == 2 ? kDepth2 : 0) |
           (v.depth == 1 ? kDepth1 : 0) | ((v.occ & 15) << kOccShift) | (v.early ? kEarly : 0) |
           (v.spre ? kSPre : 0) | (v.fuse_tail ? kFuse : 0) | (v.ptrs ? kPtrs : 0) | (v.segs ? kSegs : 0) |
           (v.glds ? kGlds : 0) | (v.serial ? kSerial : 0) | (v.sc1_store ? kSc1Store : 0) |
           (v.realign ? kRealign : 0) | (v.peel ? kPeel : 0) | (v.wave_run ? kWaveRun : 0) |
           (v.st_align ? kStAlign : 0) | (v.xcd ? kXcd : 0) | (v.pair ? kPair : 0);
}

// ---- launch policy -----------------------------------------------------------
// Everything a full-tile launch's kernel depends on.  ec_core.cpp launch_set
// fills it per launch group (<= 4 rows); gf_apply.hip derives the product
// library's instantiation list from policy_variant over every valid shape at
// compile time, so each compiled full-tile kernel is reachable and each
// reachable shape has its kernel (tests/test_gpu_kernel_sweep.py launches them
// all against the oracle).
struct LaunchShape {
    bool decode = false;       // reconstruct (else encode)
    bool small_k = false;      // k <= 8 data shards
    unsigned rows = 1;         // output rows of the launch, 1 .. kMaxRowsPerLaunch
    bool host_mapped = false;  // shards in mapped host memory (zero-copy across PCIe)
    bool ptrs = false;         // shards named by a pointer table (ApplyArgs::shard_ptrs)
    bool segs = false;         // segment launch (block runs, decode: their plans, in the kernel arguments)
    bool compact = false;      // decode into a compact output (shmr_ec_reconstruct_batch_dev_out)
    bool sc1_ok = false;       // outputs in device memory, 16-byte aligned, shorter than 2 GiB - 4 KiB
    bool fused = false;        // the shard length leaves a partial last tile after >= 1 full tile
};

// The shapes a call can produce: encodes take no compact output, and segment
// launches only over device pitch layouts (r06: the slot runs of a pool or of
// merged per-block calls, launch_slots); compact outputs are device pitch
// layouts; sc1 needs device memory.
constexpr bool shape_valid(const LaunchShape& s) {
    if (s.rows < 1 || s.rows > kMaxRowsPerLaunch) return false;
    if (!s.decode && (s.compact || (s.segs && (s.ptrs || s.host_mapped)))) return false;
    if (s.compact && (s.ptrs || s.host_mapped)) return false;
    if (s.sc1_ok && s.host_mapped) return false;
    return true;
}

// The measured policy (profiles/ and DESIGN.md §6; every adoption is an
// interleaved A/B in one process of >= 1 point of HBM peak, or repeated on
// three boxes).
constexpr Variant policy_variant(const LaunchShape& s) {
    Variant v;
    const bool dec = s.decode, hm = s.host_mapped;
    v.depth = 2;                        // one shard of loads in flight: beats depth 1/3/5/9 on every shape
    v.u = s.rows >= 4 ? 2 : 1;          // 8 KiB tiles for 4-row launches (encode and rebuild alike)
    v.nt_load = !hm;                    // temporal loads across PCIe: the look-ahead re-read hits L2
    v.nt_store = true;
    v.fuse_tail = s.fused;              // partial tiles at the head of the full-tile grid
    v.ptrs = s.ptrs;
    v.segs = s.segs;
    // early prologue: encodes with k <= 8 (short workgroups) and 4-row encodes
    // (with the per-dword math order, fewer live VGPRs at U = 2)
    v.early = !dec && (s.small_k || s.rows >= 4) && !hm;
    v.serial = !dec && s.rows >= 4 && !hm;
    v.peel = dec && !hm;                // reconstructs: no look-ahead load past the last input
    if (dec && s.rows == 1 && !hm) v.wgs_per_cu = 7;   // 1-row rebuilds in place: cap 7 WGs / CU
    // rebuilt shards into buffers of their own (compact output, device pointer
    // tables): sc1 stores, no residency cap; the early prologue pays for 4 rows
    if (dec && !hm && (s.compact || s.ptrs)) {
        v.sc1_store = true;
        v.nt_store = false;
        v.wgs_per_cu = 0;
        v.early = s.rows >= 4;
    }
    if (s.ptrs) {
        if (hm) {
            v.early = v.serial = false;   // the mapped policy: the plain LDS-staged tile
        } else {
            // first loads addressed from scalar loads of the block's table row:
            // RS(8,3) encode and every rebuild gain; RS(10,4) encode loses
            v.early = dec || s.small_k;
            if (!v.early) v.serial = false;
        }
    }
    v.wave_run = v.u > 1 && !hm;
    // sc1 stores are raw buffer stores: device memory, 16-byte aligned rows,
    // a 2 GiB resource per row
    if (v.sc1_store && !s.sc1_ok) {
        v.sc1_store = false;
        v.nt_store = true;
    }
    return v;
}

// rows in [1, kMaxRowsPerLaunch].  mode 0: full tiles, every shard base
// (base + b*bpitch + idx*spitch) 16-byte aligned (variant v); mode 1: one
// partial tail tile per block (aligned, U = 1); mode 2: any alignment,
// byte-granular (U = 1); mode 3: full 4 KiB tiles at any alignment, vector
// loads and stores realigned in registers (U = 1).  The variant only affects
// mode 0.  Modes 0 and 1 also run on misaligned shards where the device's
// unaligned vector access was verified (probe_unaligned_vector).
// grid_cap: -1 one workgroup per tile; 0 balanced persistent grid sized by
// occupancy; > 0 persistent grid capped at grid_cap.  hipErrorInvalidValue:
// the variant is not compiled into this library.
hipError_t launch_apply(const ApplyArgs& a, unsigned rows, const Variant& v, int mode, int grid_cap,
                        hipStream_t stream);

// Whether the full-tile kernel for variant v at `rows` rows is compiled into
// the library.
bool variant_compiled(const Variant& v, unsigned rows);

#ifdef SHMR_EC_TOOLS
// Full-tile measurement variants (gf_apply_tools.hip, tools build only):
// launch_apply / variant_compiled fall through to these for variants the
// product list does not carry.
hipError_t launch_full_tools(const ApplyArgs& a, unsigned rows, const Variant& v, int grid_cap, hipStream_t stream);
bool variant_compiled_tools(const Variant& v);
#endif

// Every gf_apply_kernel instantiation of the product list (gf_apply.hip) and
// the MODE 1-3 kernels, with the launches each has served in this process
// (shmr_ec_kernel_inventory).
struct KernelInfo {
    uint32_t rows, chunks, mode, flags;
    uint64_t launches;
};
size_t kernel_inventory(KernelInfo* out, size_t cap);

// The compare kernels (gf_compare.hip) share one body over the compare tile of
// gf_syndrome.hpp: plan rows are recomputed from the k inputs and either
// stored or compared with the bytes at their output slots.  Not part of
// kernel_inventory.
//
// The parity check (ReedSolomon::verify): `a` as for an encode launch of `rows`
// parity rows from a.row0 (single plan; a.blk_list must be null, else
// hipErrorInvalidValue; out_base = the STORED parity, which is only read).  ORs bit min(a.row0 + r, 31) into mismatch[blk]
// for every row r of a block whose stored bytes differ from the recomputed
// ones in this launch's tiles; writes nothing for a block without a
// difference.  blk = a.blk_first + j * a.blk_stride is the block's index, as
// for launch_check below: the one caller (ec_core verify_on_device) launches
// blk_first = 0, blk_stride = 1, so word j is launch block j's.  mode 0: full
// tiles of u = verify_chunks(rows) chunks per lane (the tools build: 1 or 2);
// mode 1: one partial tail tile per block; mode 2: byte-granular, any
// alignment.  One workgroup per tile.
// The measured tile size (profiles/r07/verify_ab*.jsonl): 8 KiB
// full tiles (U = 2, wave-contiguous runs) at 3 and 4 rows, +1.4 / +1.7 points
// of HBM peak over 4 KiB; 1 and 2 rows keep the encode policy's U = 1.
constexpr int verify_chunks(unsigned rows) { return rows >= 3 ? 2 : 1; }
hipError_t launch_verify(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, int u, int mode, hipStream_t stream);

// The checked reconstruct (shmr_ec_reconstruct_checked_batch_dev): `a` as for
// an in-place reconstruct
// launch of `rows` plan rows from a.row0 (single plan; blocks blk_first + j *
// blk_stride, or a.blk_list[j]; in_base == out_base, out_bias 0).  Rows
// [0, nstore) of the group are computed and stored to their out_idx slots (absent
// shards); rows [nstore, rows) are computed and compared with the bytes at
// their out_idx slots (present surplus shards, only read): a difference in this
// launch's tiles ORs bit bits[r] (< 32) into mismatch[blk], blk the block's
// index as above -- not its position in the launch.  Writes no word of a
// block without a difference.  mode 0: full 4 KiB tiles; mode 1: one partial
// tail tile per block; mode 2: byte-granular, any alignment.  One workgroup per
// tile.
hipError_t launch_check(const ApplyArgs& a, uint32_t* mismatch, unsigned rows, unsigned nstore, const uint32_t* bits,
                        int mode, hipStream_t stream);

// The single-shard location kernels (gf_locate.hip; shmr_ec_locate_batch_dev),
// behind a launch_verify of the same blocks: `a` as for launch_verify of the
// first row group (a.row0 = 0, rows = min(p, 4) in [2, 4]); mismatch[j] the
// complete verify word of launch block j (p <= 32 parity rows: a bit each);
// qtab the tables of the codec's locate plan (PermTab[k][rows - 1]).  In a
// block whose every parity row differs, clears bit t of cand[j * words ..]
// (words = ceil(k / 32), preset to all ones by the caller) for every data
// shard t that this launch's tiles rule out; reads one word per tile of any
// other block.  Modes as launch_verify, 4 KiB tiles; a bounded grid strides
// over the tiles.  Not part of kernel_inventory.
hipError_t launch_locate(const ApplyArgs& a, const uint8_t* qtab, const uint32_t* mismatch, uint32_t* cand,
                         unsigned rows, unsigned p, int mode, hipStream_t stream);
// cand[0 .. nblk * words) = all ones (a kernel: see gf_locate.hip).
hipError_t launch_locate_preset(uint32_t* cand, uint64_t nblk, unsigned k, hipStream_t stream);
// located[b] = locate::resolve(mismatch[b], cand + b * words, k, p) (locate_plan.hpp), b < nblk.
hipError_t launch_locate_resolve(const uint32_t* mismatch, const uint32_t* cand, int32_t* located, uint64_t nblk,
                                 unsigned k, unsigned p, hipStream_t stream);

// The degraded forms (shmr_ec_locate_checked_batch_dev), behind a launch_check
// of the same blocks: `a` as for launch_check of the pattern's compare-only
// checked plan (in_base == out_base, a.row0 = 0; blocks blk_first + j *
// blk_stride, or a.blk_list[j]), rows = min(s, 4) in [2, 4] of its s = a.m
// compare rows; row_mask the word of a block whose every compared row differs;
// qtab the tables of the pattern's ratio plan (PermTab[k][rows - 1]).
// mismatch and cand are indexed by the block's index in the batch, not by j.
// Reads the k inputs and the first `rows` surplus shards of a block whose word
// is row_mask, one word per tile of any other; stores nothing but the atomics.
hipError_t launch_locate_checked(const ApplyArgs& a, const uint8_t* qtab, const uint32_t* mismatch, uint32_t* cand,
                                 unsigned rows, uint32_t row_mask, int mode, hipStream_t stream);
// located[blk] = locate::resolve_checked(mismatch[blk], cand + blk * words, k, s, row_mask, idx, idx + k) for
// the blocks `a` names.  idx: in_idx[k] then out_idx[s] in device memory (the
// header of the compare-only plan image, + 8); may be null for s < 2.
hipError_t launch_locate_checked_resolve(const ApplyArgs& a, const uint32_t* mismatch, const uint32_t* cand,
                                         int32_t* located, const uint16_t* idx, unsigned s, uint32_t row_mask,
                                         hipStream_t stream);

// The two-shard location kernels (gf_locate.hip; shmr_ec_locate_pair_batch_dev),
// behind launch_locate_resolve of the same blocks (single[b] its answers), for
// codecs of locate::pair_supported; words = locate::pair_bitmap_words(k).
// Not part of kernel_inventory.
// pairs[0 .. nblk * words) = all ones, *count = 0.
hipError_t launch_locate_pair_preset(uint32_t* pairs, uint32_t* count, uint64_t nblk, unsigned k, hipStream_t stream);
// Appends every block b < nblk of locate::pair_listed(mismatch[b], single[b], p)
// to list[] (nblk entries, any order) and counts them in *count.
hipError_t launch_locate_pair_select(const uint32_t* mismatch, const int32_t* single, uint32_t* list, uint32_t* count,
                                     uint64_t nblk, unsigned p, hipStream_t stream);
// `a` as for launch_verify of the first row group (a.row0 = 0, 4 rows) over the
// whole batch; ptab the tables of the codec's pair plan.  For each listed
// block, clears the bit of every candidate pair that this launch's tiles rule
// out; reads *count and nothing else when the list is empty.  Modes and grid
// as launch_locate.
hipError_t launch_locate_pair(const ApplyArgs& a, const uint8_t* ptab, const uint32_t* list, const uint32_t* count,
                              uint32_t* pairs, int mode, bool skip, hipStream_t stream);
// located[2 b], located[2 b + 1] = locate::resolve_pair(mismatch[b], single[b], pairs + b * words, k, p), b < nblk.
hipError_t launch_locate_pair_resolve(const uint32_t* mismatch, const int32_t* single, const uint32_t* pairs,
                                      int32_t* located, uint64_t nblk, unsigned k, unsigned p, hipStream_t stream);

// The parity delta update kernel (gf_update.hip; shmr_ec_update_batch_dev):
// one launch over pieces [0, npieces) of a piece table (update_plan.hpp
// DevPiece, device memory), all of one round: no two of them store to the same
// parity byte.  One workgroup per 4 KiB tile of a piece; tile_base = the first
// piece's tile0, ntiles = the tiles of these pieces (< 2^31).  tabs: the
// PermTab[k][p] tables of the codec's encode plan image (entry j * p + r).
// Stores bytes [col, col + len) of the piece's data shard and of every parity
// row of its block, nothing else; loads the same bytes and len bytes of src.
// A piece without kVecFlag moves byte by byte: the edges, and every piece whose
// addresses are off 16-byte alignment on a device without unaligned vector
// access.  Not part of kernel_inventory.
struct UpdateArgs {
    uint8_t* data;
    uint8_t* parity;
    const uint8_t* src;
    const uint8_t* tabs;
    const update::DevPiece* pieces;
    uint64_t data_bpitch, data_spitch, par_bpitch, par_spitch;
    uint32_t p, npieces, tile_base, ntiles;
};
hipError_t launch_update(const UpdateArgs& u, hipStream_t stream);

// The ranged read kernel (gf_read.hip; shmr_ec_read_batch_dev): one launch
// over pieces [0, npieces) of a piece table (read_plan.hpp DevPiece, device
// memory, tile0 of the first piece 0).  One workgroup per 4 KiB tile of a
// piece; ntiles = the tiles of these pieces (< 2^31).  All shards of block b
// at shards + b * bpitch + i * spitch.  A copy piece loads bytes [col, col +
// len) of its shard; a rebuild piece (kRebuildFlag) those columns of the k
// inputs its plan image names (DevPiece::plan: a data-only reconstruct plan
// image, DevPiece::shard its row).  Stores dst[DevPiece::dst, + len) and
// nothing else.  A piece without kVecFlag moves byte by byte: the edges, and
// every piece whose addresses are off 16-byte alignment on a device without
// unaligned vector access.  Not part of kernel_inventory.
struct ReadArgs {
    const uint8_t* shards;
    uint8_t* dst;
    const read::DevPiece* pieces;
    uint64_t bpitch, spitch;
    uint32_t k, npieces, ntiles;
};
hipError_t launch_read(const ReadArgs& r, hipStream_t stream);

// The degraded update kernel (gf_update_degraded.hip;
// shmr_ec_update_degraded_batch_dev): one launch over pieces [0, npieces) of a
// piece table (update_degraded_plan.hpp DevPiece, device memory), all of one
// round: no two of them touch the same column of one block.  One workgroup per
// 4 KiB tile of a piece; tile_base = the first piece's tile0, ntiles = the
// tiles of these pieces (< 2^31).  All shards of block b at shards + b *
// bpitch + i * spitch.  tabs: the PermTab[k][p] tables of the codec's encode
// plan image (entry j * p + r).  A piece of a present shard loads and stores
// bytes [col, col + len) of it; a rebuild piece (kRebuildFlag) loads those
// columns of the k inputs its plan image names (DevPiece::plan, a data-only
// reconstruct plan image, and its row there) and leaves the shard's slot alone.
// Either loads len bytes of src and loads and stores bytes [col, col + len) of
// the parity rows DevPiece::rows lists (the block's present ones), nothing
// else.  A piece without kVecFlag moves byte by byte, as in launch_update.
// Not part of kernel_inventory.
struct UpdateDegradedArgs {
    uint8_t* shards;
    const uint8_t* src;
    const uint8_t* tabs;
    const degraded::DevPiece* pieces;
    uint64_t bpitch, spitch;
    uint32_t k, p, npieces, tile_base, ntiles;
};
hipError_t launch_update_degraded(const UpdateDegradedArgs& u, hipStream_t stream);

// The submission queue's completion mark (submit.cpp): a one-wave kernel on
// `stream` that stores `seq` to `word` -- pinned host memory, a system-scope
// release store -- once every earlier kernel of the stream has completed, so
// waiting callers poll a host word instead of the HIP runtime.
hipError_t launch_mark(uint64_t* word, uint64_t seq, hipStream_t stream);

// Runs a one-wave kernel on `stream` (current device) that loads and stores 16
// bytes at addresses off 16-byte alignment (plain and nontemporal), waits for
// it, and sets *ok if the bytes arrived where they belong: the memory
// system's unaligned access mode serves the vector kernels on misaligned
// shards (ec_core launch_set).  Scratch: kProbeScratchBytes of device memory
// and of pinned host memory.
constexpr int kProbeScratchBytes = 4 * (64 * 16 + 64);
hipError_t probe_unaligned_vector(bool* ok, uint8_t* d_scratch, uint8_t* h_scratch, hipStream_t stream);

}  // namespace kern
}  // namespace shmr
