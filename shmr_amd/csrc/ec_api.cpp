// C ABI of the MI355X erasure path (include/shmr_ec.h).
//
// Validation in the crate's order, then device work through ec_core (device
// batches) or host_engine (host-buffer batches).  There is deliberately no
// CPU compute path: without a GPU every compute entry point fails with
// SHMR_EC_NO_DEVICE.
#include "shmr_ec.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <new>
#include <vector>

#include "ec_core.hpp"
#include "host_engine.hpp"
#include "locate_plan.hpp"
#include "submit.hpp"

using shmr::core::Codec;
using shmr::core::Plan;
namespace core = shmr::core;

namespace {
// No C++ exception (allocation failure, thread or stream creation) crosses the
// C ABI: it becomes a status code, so a Rust/C caller never sees an abort.
// Every entry point runs under the relaxed capture mode (core::RelaxedCapture).
template <class F>
int guarded(F&& f) noexcept {
    try {
        core::RelaxedCapture relaxed;
        return f();
    } catch (const std::bad_alloc&) {
        return SHMR_EC_OUT_OF_MEMORY;
    } catch (...) {
        return SHMR_EC_DEVICE_ERROR;
    }
}
// The submission queue's per-block entry points make no HIP call in the
// caller's thread except through the queue (whose launches, watcher and
// creation enter the relaxed mode themselves): no mode switch per call -- two
// runtime calls per block that the 16-thread per-block shape pays in
// contention (r06, tools/perblock_dev.cpp).
template <class F>
int guarded_light(F&& f) noexcept {
    try {
        return f();
    } catch (const std::bad_alloc&) {
        return SHMR_EC_OUT_OF_MEMORY;
    } catch (...) {
        return SHMR_EC_DEVICE_ERROR;
    }
}
// Slabs handed out by shmr_ec_device_alloc_shards (base -> device; `freeing`
// while a shmr_ec_device_free_shards of it runs: one of two racing frees wins,
// and a failed free leaves the entry, so the slab can still be freed).
struct SlabEntry {
    int device;
    bool freeing;
};
std::mutex g_slab_mu;
std::map<uintptr_t, SlabEntry> g_slabs;

// The crate's checks of one presence pattern for the host-only *_plan exports.
int check_pattern(const shmr_ec_t* rs, const uint8_t* present, size_t nshards) {
    const unsigned k = rs->codec->k(), t = k + rs->codec->p();
    if (nshards < t) return SHMR_EC_TOO_FEW_SHARDS;
    if (nshards > t) return SHMR_EC_TOO_MANY_SHARDS;
    unsigned np = 0;
    for (unsigned i = 0; i < t; ++i) np += present[i] ? 1 : 0;
    return np < k ? SHMR_EC_TOO_FEW_SHARDS_PRESENT : SHMR_EC_OK;
}

// A plan's k inputs, its first n_out outputs and the n_rows rows of `rows`
// (null: none) to the caller of a *_plan export; rows_len: what out_rows holds.
int copy_plan_out(const Plan& plan, unsigned n_out, const Plan* rows, uint16_t* in_idx, uint16_t* out_idx,
                  uint8_t* out_rows, size_t rows_len) {
    const size_t k = plan.k, n_rows = rows ? rows->m : 0;
    if (rows_len < n_rows * k) return SHMR_EC_INVALID_ARGUMENT;
    std::memcpy(in_idx, plan.in_idx.data(), 2 * k);
    if (n_out) std::memcpy(out_idx, plan.out_idx.data(), 2 * size_t(n_out));
    if (n_rows) std::memcpy(out_rows, rows->rows.d.data(), n_rows * k);
    return SHMR_EC_OK;
}
}  // namespace

extern "C" {

const char* shmr_ec_status_name(int st) {
    switch (st) {
        case SHMR_EC_OK: return "Ok";
        case SHMR_EC_TOO_FEW_SHARDS: return "TooFewShards";
        case SHMR_EC_TOO_MANY_SHARDS: return "TooManyShards";
        case SHMR_EC_TOO_FEW_DATA_SHARDS: return "TooFewDataShards";
        case SHMR_EC_TOO_MANY_DATA_SHARDS: return "TooManyDataShards";
        case SHMR_EC_TOO_FEW_PARITY_SHARDS: return "TooFewParityShards";
        case SHMR_EC_TOO_MANY_PARITY_SHARDS: return "TooManyParityShards";
        case SHMR_EC_TOO_FEW_BUFFER_SHARDS: return "TooFewBufferShards";
        case SHMR_EC_TOO_MANY_BUFFER_SHARDS: return "TooManyBufferShards";
        case SHMR_EC_INCORRECT_SHARD_SIZE: return "IncorrectShardSize";
        case SHMR_EC_TOO_FEW_SHARDS_PRESENT: return "TooFewShardsPresent";
        case SHMR_EC_EMPTY_SHARD: return "EmptyShard";
        case SHMR_EC_INVALID_SHARD_FLAGS: return "InvalidShardFlags";
        case SHMR_EC_INVALID_INDEX: return "InvalidIndex";
        case SHMR_EC_INVALID_ARGUMENT: return "InvalidArgument";
        case SHMR_EC_NO_DEVICE: return "NoDevice";
        case SHMR_EC_DEVICE_ERROR: return "DeviceError";
        case SHMR_EC_OUT_OF_MEMORY: return "OutOfMemory";
        default: return "Unknown";
    }
}

#ifndef SHMR_EC_KERNEL_ID
#define SHMR_EC_KERNEL_ID "unknown"
#endif
#ifdef SHMR_EC_TOOLS
#define SHMR_EC_FLAVOUR "tools"
#else
#define SHMR_EC_FLAVOUR "product"
#endif

const char* shmr_ec_version(void) { return "shmr_ec 0.3.0 (gfx950, " SHMR_EC_FLAVOUR ")"; }

const char* shmr_ec_build_id(void) { return SHMR_EC_KERNEL_ID; }

int shmr_ec_is_tools_build(void) {
#ifdef SHMR_EC_TOOLS
    return 1;
#else
    return 0;
#endif
}

size_t shmr_ec_shard_size(uint64_t length, uint32_t data_shards) {
    if (data_shards == 0) return 0;
    // Rust: (length as f32 / data_shards as f32).ceil() as usize
    const float q = static_cast<float>(length) / static_cast<float>(data_shards);
    const float c = std::ceil(q);
    if (!(c > 0.0f)) return 0;
    if (c >= 18446744073709551615.0f) return SIZE_MAX;
    return static_cast<size_t>(c);
}

int shmr_ec_new(uint32_t data_shards, uint32_t parity_shards, shmr_ec_t** out) {
    if (!out) return SHMR_EC_INVALID_ARGUMENT;
    *out = nullptr;
    if (data_shards == 0) return SHMR_EC_TOO_FEW_DATA_SHARDS;
    if (parity_shards == 0) return SHMR_EC_TOO_FEW_PARITY_SHARDS;
    if (uint64_t(data_shards) + parity_shards > 256) return SHMR_EC_TOO_MANY_SHARDS;
    try {
        auto* rs = new shmr_ec;
        rs->codec = shmr::gf::get_codec(data_shards, parity_shards);
        *out = rs;
    } catch (...) {
        return SHMR_EC_OUT_OF_MEMORY;
    }
    return SHMR_EC_OK;
}

void shmr_ec_free(shmr_ec_t* rs) { delete rs; }

uint32_t shmr_ec_data_shard_count(const shmr_ec_t* rs) { return rs ? rs->codec->k() : 0; }
uint32_t shmr_ec_parity_shard_count(const shmr_ec_t* rs) { return rs ? rs->codec->p() : 0; }
uint32_t shmr_ec_total_shard_count(const shmr_ec_t* rs) { return rs ? rs->codec->k() + rs->codec->p() : 0; }

int shmr_ec_matrix(const shmr_ec_t* rs, uint8_t* out, size_t out_len) {
    if (!rs || !out) return SHMR_EC_INVALID_ARGUMENT;
    const auto& m = rs->codec->matrix();
    if (out_len < m.d.size()) return SHMR_EC_INVALID_ARGUMENT;
    std::memcpy(out, m.d.data(), m.d.size());
    return SHMR_EC_OK;
}

int shmr_ec_reconstruct_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards, int data_only,
                             uint16_t* in_idx, uint16_t* out_idx, uint8_t* out_rows, size_t out_rows_len,
                             uint32_t* n_out) {
    return guarded([&]() -> int {
        if (!rs || !present || !in_idx || !out_idx || !out_rows || !n_out) return SHMR_EC_INVALID_ARGUMENT;
        int rc = check_pattern(rs, present, nshards);
        if (rc) return rc;
        const unsigned t = rs->codec->k() + rs->codec->p();
        if (std::all_of(present, present + t, [](uint8_t x) { return x != 0; })) {   // crate: all present -> Ok(())
            *n_out = 0;
            return SHMR_EC_OK;
        }
        std::vector<uint8_t> pr(present, present + t);
        auto plan = rs->codec->reconstruct_plan(pr, data_only != 0);
        if ((rc = copy_plan_out(*plan, plan->m, plan.get(), in_idx, out_idx, out_rows, out_rows_len))) return rc;
        *n_out = plan->m;
        return SHMR_EC_OK;
    });
}

int shmr_ec_set_device(shmr_ec_t* rs, int device) {
    if (!rs || device < 0) return SHMR_EC_INVALID_ARGUMENT;
    rs->device = device;
    return SHMR_EC_OK;
}

int shmr_ec_set_tuning(const char* key, int value) {
    return guarded([&]() -> int {
        if (!key) return SHMR_EC_INVALID_ARGUMENT;
        bool known = false;
        const int rc = core::set_submit_tuning(key, value, &known);
        return known ? rc : core::set_tuning(key, value);
    });
}
int shmr_ec_get_tuning(const char* key) {
    return guarded([&]() -> int {
        if (!key) return SHMR_EC_INVALID_ARGUMENT;
        bool known = false;
        const int v = core::get_submit_tuning(key, &known);
        return known ? v : core::get_tuning(key);
    });
}

int shmr_ec_queue_stats(int device, uint64_t* out, size_t n) {
    if (!out || device < 0) return SHMR_EC_INVALID_ARGUMENT;
    core::submit_stats(device, out, n);
    return SHMR_EC_OK;
}

int shmr_ec_describe_variant(int decode, uint32_t data_shards, uint32_t rows, char* buf, size_t len) {
    if (!buf || len == 0 || rows == 0) return SHMR_EC_INVALID_ARGUMENT;
    if (decode < 0 || decode > 4) return SHMR_EC_INVALID_ARGUMENT;
    const core::OpClass op = (decode == 1 || decode == 2 || decode == 4) ? core::kDecode : core::kEncode;
    const uint32_t r = std::min<uint32_t>(rows, shmr::kern::kMaxRowsPerLaunch);
    // 3 / 4: encode / reconstruct over device shard-pointer tables (aligned
    // shards); the variant of a shard length with a partial last tile
    const shmr::kern::LaunchShape s =
        core::shape_of(op, data_shards, r, false, decode >= 3, false, decode == 2, true, true);
    const auto v = core::select_variant(op, s);
    auto lean = v;   // the full-tile kernel without fused tails must always exist
    lean.fuse_tail = false;
    const bool compiled = shmr::kern::variant_compiled(lean, r) && (!v.fuse_tail || shmr::kern::variant_compiled(v, r));
    std::snprintf(buf, len,
                  "chunks=%d nt_load=%d nt_store=%d occ8=%d threads=%d grid=%d diag=%d depth=%d "
                  "wgs_per_cu=%d occ=%d early=%d spre=%d fuse_tail=%d compiled=%d",
                  v.u, int(v.nt_load), int(v.nt_store), int(v.occ8), v.threads,
                  core::grid_mode(op), int(v.diag), v.depth, v.wgs_per_cu, v.occ, int(v.early), int(v.spre), int(v.fuse_tail),
                  int(compiled));
    // the later flags are appended only when set: records keyed by the string stay valid
    core::describe_variant_tail(v, buf, len);
    return SHMR_EC_OK;
}

size_t shmr_ec_kernel_inventory(shmr_ec_kernel_info* out, size_t cap) {
    static_assert(sizeof(shmr_ec_kernel_info) == sizeof(shmr::kern::KernelInfo), "kernel info layout");
    return shmr::kern::kernel_inventory(reinterpret_cast<shmr::kern::KernelInfo*>(out), out ? cap : 0);
}

int shmr_ec_cache_stats(const shmr_ec_t* rs, uint64_t* hits, uint64_t* misses) {
    if (!rs) return SHMR_EC_INVALID_ARGUMENT;
    if (hits) *hits = rs->codec->decode_cache_hits();
    if (misses) *misses = rs->codec->decode_cache_misses();
    return SHMR_EC_OK;
}

int shmr_ec_device_count(void) { return core::device_count(); }

int shmr_ec_device_init(int device) {
    return guarded([&]() -> int {
        const int rc = core::check_device(device);
        if (rc) return rc;
        return core::device_init(device, nullptr);
    });
}

int shmr_ec_capture_reserve(int device, size_t bytes) {
    return guarded([&]() -> int {
        const int rc = core::check_device(device);
        if (rc) return rc;
        return core::capture_reserve(device, bytes);
    });
}

int shmr_ec_device_stats(int device, uint64_t* out, size_t n) {
    if (!out || device < 0) return SHMR_EC_INVALID_ARGUMENT;
    core::device_stats(device, out, n);
    return SHMR_EC_OK;
}

int shmr_ec_path_stats(uint64_t* zero_copy_blocks, uint64_t* staged_blocks) {
    core::path_stats(zero_copy_blocks, staged_blocks);
    return SHMR_EC_OK;
}

// ---- device memory for batches -------------------------------------------------
int shmr_ec_device_alloc(int device, size_t bytes, int contiguous, void** out) {
    return guarded([&]() -> int {
        if (!out) return SHMR_EC_INVALID_ARGUMENT;
        *out = nullptr;
        int rc = core::check_device(device);
        if (rc) return rc;
        hipError_t e;
        {
            core::DeviceScope scope(device);
            if (!scope.ok()) return SHMR_EC_DEVICE_ERROR;
            const size_t n = bytes ? bytes : 1;
            core::RelaxedCapture relaxed;
            e = contiguous ? hipExtMallocWithFlags(out, n, hipDeviceMallocContiguous) : hipMalloc(out, n);
        }
        if (e != hipSuccess) {
            (void)hipGetLastError();
            *out = nullptr;
            return SHMR_EC_OUT_OF_MEMORY;
        }
        return SHMR_EC_OK;
    });
}

int shmr_ec_device_free(int device, void* p) {
    return guarded([&]() -> int {
        if (!p) return SHMR_EC_OK;
        int rc = core::check_device(device);
        if (rc) return rc;
        // A slab freed this way leaves no registry entry for a later allocation
        // at the same address to inherit: dropped now (the address is still
        // ours) -- unless free_shards is freeing it, which keeps the entry until
        // the memory is gone, so a failed free can be retried.
        {
            std::lock_guard<std::mutex> lk(g_slab_mu);
            auto it = g_slabs.find(uintptr_t(p));
            if (it != g_slabs.end() && it->second.device == device && !it->second.freeing) g_slabs.erase(it);
        }
        {
            core::DeviceScope scope(device);
            if (!scope.ok()) return SHMR_EC_DEVICE_ERROR;
            core::RelaxedCapture relaxed;
            if (hipFree(p) != hipSuccess) {
                (void)hipGetLastError();
                return SHMR_EC_DEVICE_ERROR;
            }
        }
        std::lock_guard<std::mutex> lk(g_slab_mu);
        auto it = g_slabs.find(uintptr_t(p));   // (an entry a new slab at this address made is not ours)
        if (it != g_slabs.end() && it->second.device == device && it->second.freeing) g_slabs.erase(it);
        return SHMR_EC_OK;
    });
}

// ---- shard buffers in slot placement (pointer-table calls) ----------------------
int shmr_ec_device_alloc_shards(int device, size_t nblocks, size_t shards_per_block, size_t shard_len,
                                uint8_t** out_ptrs) {
    return guarded([&]() -> int {
        if (!out_ptrs || nblocks == 0 || shards_per_block == 0 || shard_len == 0) return SHMR_EC_INVALID_ARGUMENT;
        const uint64_t n = uint64_t(nblocks) * shards_per_block;
        if (n / nblocks != shards_per_block) return SHMR_EC_INVALID_ARGUMENT;
        // page-aligned slots, one page more for a
        // power-of-two stride (the bench layout's placement)
        uint64_t pitch = core::round_up(shard_len, 4096);
        if (pitch % 65536 == 0) pitch += 4096;
        if (pitch < shard_len || n > UINT64_MAX / pitch) return SHMR_EC_INVALID_ARGUMENT;
        void* slab = nullptr;
        const int rc = shmr_ec_device_alloc(device, size_t(n * pitch), 0, &slab);
        if (rc) return rc;
        try {
            std::lock_guard<std::mutex> lk(g_slab_mu);
            g_slabs[uintptr_t(slab)] = SlabEntry{device, false};
        } catch (...) {
            (void)shmr_ec_device_free(device, slab);
            throw;
        }
        uint8_t* base = static_cast<uint8_t*>(slab);
        for (uint64_t j = 0; j < n; ++j) out_ptrs[j] = base + j * pitch;
        return SHMR_EC_OK;
    });
}

int shmr_ec_device_free_shards(int device, uint8_t* first) {
    return guarded([&]() -> int {
        if (!first) return SHMR_EC_OK;
        {
            std::lock_guard<std::mutex> lk(g_slab_mu);
            auto it = g_slabs.find(uintptr_t(first));
            if (it == g_slabs.end() || it->second.device != device || it->second.freeing)
                return SHMR_EC_INVALID_ARGUMENT;
            it->second.freeing = true;   // under the lock: one of two racing frees wins
        }
        const int rc = shmr_ec_device_free(device, first);   // erases the entry once freed
        if (rc) {
            std::lock_guard<std::mutex> lk(g_slab_mu);
            auto it = g_slabs.find(uintptr_t(first));
            if (it != g_slabs.end()) it->second.freeing = false;   // still allocated: freeable again
        }
        return rc;
    });
}

// ---- pinned host memory (Block Cache buffers) --------------------------------
// Mapped + portable: every GPU of the node can address it, so the host-buffer
// entry points run their kernels on it in place (zero-copy).
int shmr_ec_host_alloc(size_t bytes, void** out) {
    return guarded([&]() -> int {
        if (!out) return SHMR_EC_INVALID_ARGUMENT;
        *out = nullptr;
        int rc = core::check_device(0);
        if (rc) return rc;
        const size_t n = bytes ? bytes : 1;
        core::RelaxedCapture relaxed;
        if (hipHostMalloc(out, n, hipHostMallocMapped | hipHostMallocPortable) != hipSuccess) {
            (void)hipGetLastError();
            *out = nullptr;
            return SHMR_EC_OUT_OF_MEMORY;
        }
        void* dev = nullptr;
        if (hipHostGetDevicePointer(&dev, *out, 0) == hipSuccess && dev) {
            try {
                core::mapped_add(*out, n, dev);
            } catch (...) {   // registry allocation failed: hand nothing out
                (void)hipHostFree(*out);
                *out = nullptr;
                throw;
            }
        } else {
            (void)hipGetLastError();   // still pinned: the staged DMA path takes it
        }
        return SHMR_EC_OK;
    });
}

void shmr_ec_host_free(void* p) {
    if (!p) return;
    core::mapped_remove(p);
    core::RelaxedCapture relaxed;
    if (hipHostFree(p) != hipSuccess) (void)hipGetLastError();
}

int shmr_ec_host_register(void* p, size_t bytes) {
    return guarded([&]() -> int {
        if (!p || bytes == 0) return SHMR_EC_INVALID_ARGUMENT;
        int rc = core::check_device(0);
        if (rc) return rc;
        core::RelaxedCapture relaxed;
        if (hipHostRegister(p, bytes, hipHostRegisterMapped | hipHostRegisterPortable) != hipSuccess) {
            (void)hipGetLastError();
            return SHMR_EC_DEVICE_ERROR;
        }
        void* dev = nullptr;
        if (hipHostGetDevicePointer(&dev, p, 0) != hipSuccess || !dev) {
            (void)hipGetLastError();
            (void)hipHostUnregister(p);
            return SHMR_EC_DEVICE_ERROR;
        }
        try {
            core::mapped_add(p, bytes, dev);
        } catch (...) {
            (void)hipHostUnregister(p);
            throw;
        }
        return SHMR_EC_OK;
    });
}

int shmr_ec_host_unregister(void* p) {
    return guarded([&]() -> int {
        if (!p || !core::mapped_remove(p)) return SHMR_EC_INVALID_ARGUMENT;
        core::RelaxedCapture relaxed;
        if (hipHostUnregister(p) == hipSuccess) return SHMR_EC_OK;
        (void)hipGetLastError();
        return SHMR_EC_DEVICE_ERROR;
    });
}

}  // extern "C"

// ---- validation in the crate's order (shared by host and device forms) -------------
namespace {
// ReedSolomon::encode: check_piece_count!(all), then check_slices!(multi).
int check_encode(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards, size_t* len) {
    if (!rs || !shards || !shard_lens) return SHMR_EC_INVALID_ARGUMENT;
    const unsigned t = rs->codec->k() + rs->codec->p();
    if (nshards < t) return SHMR_EC_TOO_FEW_SHARDS;
    if (nshards > t) return SHMR_EC_TOO_MANY_SHARDS;
    *len = shard_lens[0];
    if (*len == 0) return SHMR_EC_EMPTY_SHARD;
    for (unsigned i = 0; i < t; ++i)
        if (shard_lens[i] != *len) return SHMR_EC_INCORRECT_SHARD_SIZE;
    for (unsigned i = 0; i < t; ++i)
        if (!shards[i]) return SHMR_EC_INVALID_ARGUMENT;
    return SHMR_EC_OK;
}

// ReedSolomon::reconstruct{,_data}: per present shard len 0 -> EmptyShard,
// mismatch -> IncorrectShardSize, in index order; then the presence count.
// *plan = nullptr: every shard present (the crate returns Ok without work).
int check_reconstruct(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, const uint8_t* present,
                      size_t nshards, int data_only, size_t* len, std::shared_ptr<Plan>* plan) {
    if (!rs || !shards || !shard_lens || !present) return SHMR_EC_INVALID_ARGUMENT;
    Codec& c = *rs->codec;
    const unsigned k = c.k(), t = k + c.p();
    if (nshards < t) return SHMR_EC_TOO_FEW_SHARDS;
    if (nshards > t) return SHMR_EC_TOO_MANY_SHARDS;
    unsigned np = 0;
    bool have_len = false;
    *len = 0;
    for (unsigned i = 0; i < t; ++i) {
        if (!present[i]) continue;
        if (shard_lens[i] == 0) return SHMR_EC_EMPTY_SHARD;
        ++np;
        if (have_len && shard_lens[i] != *len) return SHMR_EC_INCORRECT_SHARD_SIZE;
        *len = shard_lens[i];
        have_len = true;
    }
    plan->reset();
    if (np == t) return SHMR_EC_OK;
    if (np < k) return SHMR_EC_TOO_FEW_SHARDS_PRESENT;
    std::vector<uint8_t> pr(present, present + t);
    auto pl = c.reconstruct_plan(pr, data_only != 0);
    for (unsigned m = 0; m < pl->m; ++m)
        if (!shards[pl->out_idx[m]]) return SHMR_EC_INVALID_ARGUMENT;
    for (unsigned i = 0; i < k; ++i)
        if (!shards[pl->in_idx[i]]) return SHMR_EC_INVALID_ARGUMENT;
    if (pl->m) *plan = pl;
    return SHMR_EC_OK;
}

// A queue request for one validated block (row: device addresses, shard
// index order, 0 where the call touches nothing).
std::unique_ptr<core::SubmitReq> make_req(shmr_ec_t* rs, core::OpClass op, bool data_only, bool host_mapped,
                                          size_t len, int dev, std::vector<uint64_t> row, const uint8_t* present) {
    std::unique_ptr<core::SubmitReq> r(new core::SubmitReq);
    r->codec = rs->codec.get();
    r->op = op;
    r->data_only = data_only;
    r->host_mapped = host_mapped;
    r->len = len;
    r->dev = dev;
    r->set_row(row.data(), present, unsigned(row.size()));   // (after len and host_mapped: its time estimate)
    return r;
}

// Submits r; with `queued` (a *_start call) hands it over pending, else waits.
int run_req(std::unique_ptr<core::SubmitReq> r, core::SubmitReq** queued) {
    const int rc = core::submit(r.get());
    if (rc) return rc;
    if (queued) {
        *queued = r.release();
        return SHMR_EC_OK;
    }
    return core::wait(r.get());
}

// idx[i] = i for i < t: the shard lists of a call that takes shards in index order.
void identity_idx(uint16_t (&idx)[256], unsigned t) {
    for (unsigned i = 0; i < t; ++i) idx[i] = uint16_t(i);
}

// The staged leg of a single-block host call: shards in[0 .. nin) are gathered
// into pooled device staging (a pitch layout with `extra` bytes behind it; the
// pool grows without freeing), `run(staging, pitch)` works on it, and shards
// out[0 .. nout) are copied back.
template <class Run>
int run_staged(uint8_t* const* shards, size_t len, unsigned t, int dev, const uint16_t* in, unsigned nin,
               const uint16_t* out, unsigned nout, size_t extra, Run&& run) {
    core::DeviceScope scope(dev);
    if (!scope.ok()) return SHMR_EC_DEVICE_ERROR;
    const uint64_t pitch = core::round_up(len, 256);
    int rc = SHMR_EC_OK;
    core::StagingLease lease;
    lease.s = core::StagingPool::get().acquire(dev, pitch * t + extra, &rc);
    if (!lease.s) return rc;
    core::Staging& s = *lease.s;
    for (unsigned i = 0; i < nin; ++i)
        SHMR_HIP_TRY(hipMemcpyAsync(s.dbuf + in[i] * pitch, shards[in[i]], len, hipMemcpyHostToDevice, s.stream));
    rc = run(s, pitch);
    if (rc) return rc;
    for (unsigned m = 0; m < nout; ++m)
        SHMR_HIP_TRY(hipMemcpyAsync(shards[out[m]], s.dbuf + out[m] * pitch, len, hipMemcpyDeviceToHost, s.stream));
    SHMR_HIP_TRY(core::sync_stream(s.stream));
    return SHMR_EC_OK;
}

// One validated block in host buffers (shmr_ec_encode, shmr_ec_reconstruct and
// their _start forms), by the first leg that applies:
//  * knob "coalesce" and mapped shards: through the submission queue, merged
//    with concurrent calls and coded in place;
//  * mapped shards: coded in place by the kernel (zero-copy);
//  * pageable and small (bounce_limit): one bounce, one launch;
//  * else staged: shards in[0 .. k) copied to the device, `run`, shards
//    out[0 .. nout) copied back.
// async != nullptr (a _start call): shards in mapped memory are coded by kernels
// left running (a pooled stream in *async, or a request in *queued); every
// other leg finishes here.
template <class Run>
int host_block(shmr_ec_t* rs, core::OpClass op, bool data_only, uint8_t* const* shards, const uint8_t* present,
               size_t len, const uint16_t* in, const uint16_t* out, unsigned nout, core::Staging** async,
               core::SubmitReq** queued, Run&& run) {
    Codec& c = *rs->codec;
    const unsigned k = c.k(), t = k + c.p();
    const int dev = rs->device;
    int rc = core::check_device(dev);
    if (rc) return rc;
    const core::HostJob job{c, op, data_only, shards, present, 1, len, 0, 1};
    if (core::coalesce_host()) {
        std::vector<uint64_t> row;
        if (core::map_rows(job, &row)) {
            core::count_blocks(true, 1);
            return run_req(make_req(rs, op, data_only, true, len, dev, std::move(row), present),
                           async ? queued : nullptr);
        }
    }
    bool handled = false;
    rc = core::run_mapped_job(job, &dev, 1, &handled, true, async);
    if (handled || rc) return rc;
    if (uint64_t(t) * len <= core::bounce_limit()) return core::run_bounced_job(job, dev);
    core::count_blocks(false, 1);
    return run_staged(shards, len, t, dev, in, k, out, nout, 0, run);
}

int arg_ok(bool ok) { return ok ? SHMR_EC_OK : SHMR_EC_INVALID_ARGUMENT; }

// Result words (uint32_t / int32_t arrays in device memory): given, and 4-byte aligned.
bool words_given(const void* p) { return p && uintptr_t(p) % alignof(uint32_t) == 0; }

// The data / parity pitch layout of the *_batch_dev calls.  The layout's
// output side is the parity, also where a call only reads it (verify, locate).
core::Layout batch_layout(const Codec& c, const uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                          const uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch) {
    return core::Layout{d_data,           const_cast<uint8_t*>(d_parity), data_block_pitch, data_shard_pitch,
                        parity_block_pitch, parity_shard_pitch,             c.k()};
}

// A batch call on device memory, after its checks of rs and the presence flags:
// an empty batch is done, empty shards are refused, then `check` (the call's own
// pointers and flags, before any device is asked for), then `launch` with the
// device selected.
template <class Check, class Launch>
int batch_dev(size_t nblocks, size_t shard_len, int device, Check&& check, Launch&& launch) {
    if (nblocks == 0) return SHMR_EC_OK;
    if (shard_len == 0) return SHMR_EC_EMPTY_SHARD;
    int rc = check();
    if (rc) return rc;
    rc = core::check_device(device);
    if (rc) return rc;
    core::DeviceScope scope(device);
    if (!scope.ok()) return SHMR_EC_DEVICE_ERROR;
    return launch();
}

// The host checks of a read list behind rs, the empty call and shard_len, in the
// header's order: the pointers, the requests and their destinations (the
// pieces come out of the same pass), then every block's presence flags.
int read_checks(const Codec& c, bool pointers, const uint8_t* present, size_t nblocks, size_t shard_len,
                const shmr_ec_read* reads, size_t nreads, size_t dst_bytes, std::vector<shmr::read::Piece>* pieces) {
    if (!pointers || !present || !reads ||
        !shmr::read::plan(reads, nreads, nblocks, c.k(), shard_len, dst_bytes, pieces))
        return SHMR_EC_INVALID_ARGUMENT;
    return core::validate_presence(c, present, nblocks);
}

// The host checks of a degraded update behind rs, the empty call and shard_len,
// in the header's order: the pointers, the updates and their intersections (the
// rounds, and with `pieces` the pieces, come out of the same pass), then every
// block's presence flags.
int update_degraded_checks(const Codec& c, bool pointers, const uint8_t* present, size_t nblocks, size_t shard_len,
                           const shmr_ec_update* updates, size_t nupdates, size_t src_bytes, shmr::update::Plan* up,
                           bool pieces) {
    if (!pointers || !present || !updates ||
        !shmr::update::plan(updates, nupdates, nblocks, c.k(), shard_len, src_bytes, up, pieces))
        return SHMR_EC_INVALID_ARGUMENT;
    return shmr::degraded::enough_present(present, nblocks, c.k(), c.k() + c.p()) ? SHMR_EC_OK
                                                                                   : SHMR_EC_TOO_FEW_SHARDS_PRESENT;
}

// The flags of the checked calls that this build knows.
constexpr int kCheckFlags = SHMR_EC_CHECK_DATA_ONLY | SHMR_EC_CHECK_NO_REBUILD;

// Locate, rebuild, verify again (scrub, reconstruct-repair), blocking.
// check(): the call's own pointers and flags, as batch_dev takes it.
// locate(d_words, d_located, d_cand) enqueues the call's locate into pooled
// scratch; rebuild(hit, located) rebuilds the located blocks `hit` and returns
// its status and the layout of the closing verify.  counts (clean, repaired,
// not repairable) are written only by a call that is accepted; a rebuilt block
// that still differs is demoted to SHMR_EC_LOCATE_NONE.
template <class Check, class Locate, class Rebuild>
int locate_rebuild_verify(shmr_ec_t* rs, size_t nblocks, size_t shard_len, int32_t* located_host, uint64_t* counts,
                          int device, hipStream_t stream, Check&& check, Locate&& locate, Rebuild&& rebuild) {
    if (!rs || !counts || !rs->codec->locate_plan()) return SHMR_EC_INVALID_ARGUMENT;
    // (an empty batch is accepted)
    if (nblocks == 0) counts[0] = counts[1] = counts[2] = 0;
    Codec& c = *rs->codec;
    return batch_dev(nblocks, shard_len, device, check, [&]() -> int {
        int rc = core::refuse_capture(device, stream);   // it waits for its own results
        if (rc) return rc;
        counts[0] = counts[1] = counts[2] = 0;
        // pooled scratch (grown without a free): the words, the answers, the candidate bitmaps
        const size_t words_bytes = size_t(core::round_up(nblocks * sizeof(uint32_t), 256));
        core::StagingLease lease;
        lease.s = core::StagingPool::get().acquire(device, 2 * words_bytes + core::locate_work_bytes(c, nblocks), &rc);
        if (!lease.s) return rc;
        uint32_t* d_words = reinterpret_cast<uint32_t*>(lease.s->dbuf);
        int32_t* d_located = reinterpret_cast<int32_t*>(lease.s->dbuf + words_bytes);
        uint32_t* d_cand = reinterpret_cast<uint32_t*>(lease.s->dbuf + 2 * words_bytes);
        // (a failure below still waits: the scratch goes back to the pool idle)
        auto fetch = [&](void* dst, const void* src) -> int {
            const hipError_t e = hipMemcpyAsync(dst, src, nblocks * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
            const hipError_t w = core::sync_stream(stream);
            return e == hipSuccess && w == hipSuccess ? SHMR_EC_OK : SHMR_EC_DEVICE_ERROR;
        };
        std::vector<int32_t> own;
        int32_t* located = located_host;
        if (!located) {
            own.resize(nblocks);
            located = own.data();
        }
        rc = locate(d_words, d_located, d_cand);
        const int frc = fetch(located, d_located);
        if (rc || frc) return rc ? rc : frc;
        std::vector<size_t> hit;
        for (size_t b = 0; b < nblocks; ++b) {
            if (located[b] >= 0) hit.push_back(b);
            else ++counts[located[b] == SHMR_EC_LOCATE_CLEAN ? 0 : 2];
        }
        if (hit.empty()) return SHMR_EC_OK;
        const std::pair<int, core::Layout> rebuilt = rebuild(hit, located);
        rc = rebuilt.first;
        // the closing verify (every slot has been written by now): damage
        // beyond what locate looked at shows here
        if (rc == SHMR_EC_OK) rc = core::verify_on_device(c, device, rebuilt.second, nblocks, shard_len, d_words, stream);
        std::vector<uint32_t> words(nblocks);
        const int wrc = fetch(words.data(), d_words);
        if (rc || wrc) return rc ? rc : wrc;
        for (size_t b : hit) {
            if (words[b] != 0) located[b] = SHMR_EC_LOCATE_NONE;
            ++counts[words[b] != 0 ? 2 : 1];
        }
        return SHMR_EC_OK;
    });
}

// Every shard a batch call reads or writes has a buffer: all of an encode, and
// of a reconstruct all but absent parity under data_only.
bool needed_shards_given(uint8_t* const* shards, const uint8_t* present, size_t nblocks, unsigned k, unsigned t,
                         bool data_only) {
    for (size_t b = 0; b < nblocks; ++b)
        for (unsigned i = 0; i < t; ++i) {
            const bool needed = !present || present[b * t + i] || i < k || !data_only;
            if (needed && !shards[b * t + i]) return false;
        }
    return true;
}
}  // namespace

extern "C" {

// ---- host-buffer encode (ReedSolomon::encode) --------------------------------------
static int encode_impl(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards,
                       core::Staging** async, core::SubmitReq** queued) {
    return guarded([&]() -> int {
        size_t len = 0;
        const int rc = check_encode(rs, shards, shard_lens, nshards, &len);
        if (rc) return rc;
        Codec& c = *rs->codec;
        const unsigned k = c.k(), p = c.p();
        uint16_t idx[256];
        identity_idx(idx, k + p);
        return host_block(rs, core::kEncode, false, shards, nullptr, len, idx, idx + k, p, async, queued,
                          [&](core::Staging& s, uint64_t pitch) {
                              const core::Layout L{s.dbuf, s.dbuf, 0, pitch, 0, pitch, 0};
                              return core::encode_on_device(c, rs->device, L, 1, len, s.stream);
                          });
    });
}

// ---- host-buffer reconstruct (ReedSolomon::reconstruct{,_data}) ---------------------
static int reconstruct_impl(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, const uint8_t* present,
                            size_t nshards, int data_only, core::Staging** async, core::SubmitReq** queued) {
    return guarded([&]() -> int {
        size_t len = 0;
        std::shared_ptr<Plan> plan;
        const int rc = check_reconstruct(rs, shards, shard_lens, present, nshards, data_only, &len, &plan);
        if (rc || !plan) return rc;
        Codec& c = *rs->codec;
        const unsigned t = c.k() + c.p();
        return host_block(rs, core::kDecode, data_only != 0, shards, present, len, plan->in_idx.data(),
                          plan->out_idx.data(), plan->m, async, queued, [&](core::Staging& s, uint64_t pitch) {
                              return core::reconstruct_on_device(c, rs->device, s.dbuf, pitch, pitch * t, present, 1,
                                                                 len, data_only != 0, s.stream);
                          });
    });
}

// ---- one block on device buffers, through the submission queue -----------------
// The crate's encode / reconstruct of ONE block (block.rs:427, :560) whose
// shards are device buffers; concurrent calls on the device merge into batch
// launches (submit.hpp).
static int encode_dev_impl(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, size_t nshards,
                           int device, core::SubmitReq** queued) {
    return guarded_light([&]() -> int {
        size_t len = 0;
        int rc = check_encode(rs, d_shards, shard_lens, nshards, &len);
        if (rc) return rc;
        if ((rc = core::check_device(device))) return rc;
        std::vector<uint64_t> row(nshards);
        for (size_t i = 0; i < nshards; ++i) row[i] = uint64_t(uintptr_t(d_shards[i]));
        return run_req(make_req(rs, core::kEncode, false, false, len, device, std::move(row), nullptr), queued);
    });
}

static int reconstruct_dev_impl(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens,
                                const uint8_t* present, size_t nshards, int data_only, int device,
                                core::SubmitReq** queued) {
    return guarded_light([&]() -> int {
        size_t len = 0;
        std::shared_ptr<Plan> plan;
        int rc = check_reconstruct(rs, d_shards, shard_lens, present, nshards, data_only, &len, &plan);
        if (rc || !plan) return rc;
        if ((rc = core::check_device(device))) return rc;
        std::vector<uint64_t> row(nshards, 0);
        for (unsigned i = 0; i < plan->k; ++i) row[plan->in_idx[i]] = uint64_t(uintptr_t(d_shards[plan->in_idx[i]]));
        for (unsigned m = 0; m < plan->m; ++m) row[plan->out_idx[m]] = uint64_t(uintptr_t(d_shards[plan->out_idx[m]]));
        return run_req(make_req(rs, core::kDecode, data_only != 0, false, len, device, std::move(row), present), queued);
    });
}

int shmr_ec_encode(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards) {
    return encode_impl(rs, shards, shard_lens, nshards, nullptr, nullptr);
}

int shmr_ec_reconstruct(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, const uint8_t* present,
                        size_t nshards, int data_only) {
    return reconstruct_impl(rs, shards, shard_lens, present, nshards, data_only, nullptr, nullptr);
}

// ---- host-buffer verify (ReedSolomon::verify) ---------------------------------------
// The staged leg over every shard, with the result word behind the block:
// checked by the batch kernels, and the word copied back.
int shmr_ec_verify(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards,
                   int* consistent) {
    return guarded([&]() -> int {
        size_t len = 0;
        int rc = check_encode(rs, shards, shard_lens, nshards, &len);
        if (rc) return rc;
        if (!consistent) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        const unsigned k = c.k(), t = k + c.p();
        const int dev = rs->device;
        rc = core::check_device(dev);
        if (rc) return rc;
        uint16_t idx[256];
        identity_idx(idx, t);
        uint32_t word = 0;
        rc = run_staged(shards, len, t, dev, idx, t, nullptr, 0, 256, [&](core::Staging& s, uint64_t pitch) -> int {
            uint32_t* d_word = reinterpret_cast<uint32_t*>(s.dbuf + pitch * t);
            const core::Layout L{s.dbuf, s.dbuf + k * pitch, 0, pitch, 0, pitch, k};
            const int vrc = core::verify_on_device(c, dev, L, 1, len, d_word, s.stream);
            if (vrc) return vrc;
            SHMR_HIP_TRY(hipMemcpyAsync(&word, d_word, sizeof(word), hipMemcpyDeviceToHost, s.stream));
            return SHMR_EC_OK;
        });
        if (rc) return rc;
        *consistent = word == 0;
        return SHMR_EC_OK;
    });
}

int shmr_ec_encode_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, size_t nshards,
                       int device) {
    return encode_dev_impl(rs, d_shards, shard_lens, nshards, device, nullptr);
}

int shmr_ec_reconstruct_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, const uint8_t* present,
                            size_t nshards, int data_only, int device) {
    return reconstruct_dev_impl(rs, d_shards, shard_lens, present, nshards, data_only, device, nullptr);
}

// ---- asynchronous single-block calls -----------------------------------------------
struct shmr_ec_op {
    core::Staging* s = nullptr;     // pending zero-copy kernels' stream, or none
    core::SubmitReq* req = nullptr; // or a request of the submission queue
};

}  // extern "C"

// A _start call: `call(&s, &req)` is the blocking call's body, which may leave
// kernels running on a pooled stream or a request pending; *op takes them over.
template <class Call>
static int start_op(shmr_ec_op_t** op, Call&& call) {
    if (!op) return SHMR_EC_INVALID_ARGUMENT;
    *op = nullptr;
    core::Staging* s = nullptr;
    core::SubmitReq* req = nullptr;
    const int rc = call(&s, &req);
    auto drop = [&] {
        if (s) (void)core::finish_async(s);
        if (req) {
            (void)core::wait(req);
            delete req;
        }
    };
    if (rc != SHMR_EC_OK) {
        drop();
        return rc;
    }
    return guarded_light([&]() -> int {
        try {
            *op = new shmr_ec_op;
        } catch (...) {
            drop();
            throw;
        }
        (*op)->s = s;
        (*op)->req = req;
        return SHMR_EC_OK;
    });
}

extern "C" {

int shmr_ec_encode_start(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, size_t nshards,
                         shmr_ec_op_t** op) {
    return start_op(op, [&](core::Staging** s, core::SubmitReq** q) {
        return encode_impl(rs, shards, shard_lens, nshards, s, q);
    });
}

int shmr_ec_reconstruct_start(shmr_ec_t* rs, uint8_t* const* shards, const size_t* shard_lens, const uint8_t* present,
                              size_t nshards, int data_only, shmr_ec_op_t** op) {
    return start_op(op, [&](core::Staging** s, core::SubmitReq** q) {
        return reconstruct_impl(rs, shards, shard_lens, present, nshards, data_only, s, q);
    });
}

int shmr_ec_encode_dev_start(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens, size_t nshards,
                             int device, shmr_ec_op_t** op) {
    return start_op(op, [&](core::Staging**, core::SubmitReq** q) {
        return encode_dev_impl(rs, d_shards, shard_lens, nshards, device, q);
    });
}

int shmr_ec_reconstruct_dev_start(shmr_ec_t* rs, uint8_t* const* d_shards, const size_t* shard_lens,
                                  const uint8_t* present, size_t nshards, int data_only, int device,
                                  shmr_ec_op_t** op) {
    return start_op(op, [&](core::Staging**, core::SubmitReq** q) {
        return reconstruct_dev_impl(rs, d_shards, shard_lens, present, nshards, data_only, device, q);
    });
}

int shmr_ec_op_wait(shmr_ec_op_t* op) {
    if (!op) return SHMR_EC_INVALID_ARGUMENT;
    int rc = SHMR_EC_OK;
    if (op->s) rc = guarded([&] { return core::finish_async(op->s); });
    if (op->req) {
        rc = guarded_light([&] { return core::wait(op->req); });
        delete op->req;
    }
    delete op;
    return rc;
}

// ---- device-resident batches --------------------------------------------------------
int shmr_ec_encode_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                             uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch, size_t nblocks,
                             size_t shard_len, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        return batch_dev(nblocks, shard_len, device, [&] { return arg_ok(d_data && d_parity); }, [&] {
            Codec& c = *rs->codec;
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            return core::encode_on_device(c, device, L, nblocks, shard_len, static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_verify_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                             const uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch,
                             size_t nblocks, size_t shard_len, uint32_t* d_mismatch, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        const bool given = d_data && d_parity && words_given(d_mismatch);
        return batch_dev(nblocks, shard_len, device, [&] { return arg_ok(given); }, [&] {
            Codec& c = *rs->codec;
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            return core::verify_on_device(c, device, L, nblocks, shard_len, d_mismatch, static_cast<hipStream_t>(stream));
        });
    });
}

// ---- scrub: locate and repair one damaged shard per block ----------------------------
size_t shmr_ec_locate_work_size(const shmr_ec_t* rs, size_t nblocks) {
    return rs && rs->codec->locate_plan() ? core::locate_work_bytes(*rs->codec, nblocks) : 0;
}

int shmr_ec_locate_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                             const uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch,
                             size_t nblocks, size_t shard_len, uint32_t* d_mismatch, int32_t* d_located, void* d_work,
                             size_t work_bytes, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs || !rs->codec->locate_plan()) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        const bool given = d_data && d_parity && words_given(d_mismatch) && words_given(d_located) &&
                           words_given(d_work) && work_bytes >= core::locate_work_bytes(c, nblocks);
        return batch_dev(nblocks, shard_len, device, [&] { return arg_ok(given); }, [&] {
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            return core::locate_on_device(c, device, L, nblocks, shard_len, d_mismatch, d_located,
                                          static_cast<uint32_t*>(d_work), static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_scrub_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                            uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch, size_t nblocks,
                            size_t shard_len, int32_t* located_host, uint64_t* counts, int device, void* stream_) {
    return guarded([&]() -> int {
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        auto layout = [&] {
            return batch_layout(*rs->codec, d_data, data_shard_pitch, data_block_pitch, d_parity, parity_shard_pitch,
                                parity_block_pitch);
        };
        return locate_rebuild_verify(
            rs, nblocks, shard_len, located_host, counts, device, stream, [&] { return arg_ok(d_data && d_parity); },
            [&](uint32_t* d_words, int32_t* d_located, uint32_t* d_cand) {
                return core::locate_on_device(*rs->codec, device, layout(), nblocks, shard_len, d_words, d_located,
                                              d_cand, stream);
            },
            // the located shard of every such block, rebuilt from the block's other shards
            [&](const std::vector<size_t>& hit, const int32_t* located) {
                Codec& c = *rs->codec;
                const unsigned k = c.k(), t = k + c.p();
                std::vector<uint64_t> tab(hit.size() * t);
                std::vector<uint8_t> present(hit.size() * t, 1);
                for (size_t i = 0; i < hit.size(); ++i) {
                    const size_t b = hit[i];
                    for (unsigned s = 0; s < t; ++s)
                        tab[i * t + s] = s < k ? uint64_t(uintptr_t(d_data + b * data_block_pitch + s * data_shard_pitch))
                                               : uint64_t(uintptr_t(d_parity + b * parity_block_pitch +
                                                                    (s - k) * parity_shard_pitch));
                    present[i * t + size_t(located[b])] = 0;
                }
                return std::make_pair(core::ptrs_launch(c, tab.data(), present.data(), hit.size(), shard_len, false,
                                                        device, stream, core::kDecode, false, false),
                                      layout());
            });
    });
}

// ---- scrub, parity >= 4: locate and repair two damaged shards per block ---------------
size_t shmr_ec_locate_pair_work_size(const shmr_ec_t* rs, size_t nblocks) {
    return rs && rs->codec->locate_pair_plan() ? core::locate_pair_work_bytes(*rs->codec, nblocks) : 0;
}

int shmr_ec_locate_pair_plan(shmr_ec_t* rs, uint8_t* coeffs, size_t coeffs_len, uint32_t* npairs) {
    return guarded_light([&]() -> int {
        if (!rs || !coeffs || !npairs) return SHMR_EC_INVALID_ARGUMENT;
        const auto pp = rs->codec->locate_pair_plan();
        if (!pp || coeffs_len < pp->rows.d.size()) return SHMR_EC_INVALID_ARGUMENT;
        std::memcpy(coeffs, pp->rows.d.data(), pp->rows.d.size());
        *npairs = shmr::locate::pair_count(rs->codec->k());
        return SHMR_EC_OK;
    });
}

int shmr_ec_locate_pair_batch_dev(shmr_ec_t* rs, const uint8_t* d_data, size_t data_shard_pitch,
                                  size_t data_block_pitch, const uint8_t* d_parity, size_t parity_shard_pitch,
                                  size_t parity_block_pitch, size_t nblocks, size_t shard_len, uint32_t* d_mismatch,
                                  int32_t* d_located, void* d_work, size_t work_bytes, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs || !rs->codec->locate_pair_plan()) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        const bool given = d_data && d_parity && words_given(d_mismatch) && words_given(d_located) &&
                           words_given(d_work) && work_bytes >= core::locate_pair_work_bytes(c, nblocks);
        return batch_dev(nblocks, shard_len, device, [&] { return arg_ok(given); }, [&] {
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            return core::locate_pair_on_device(c, device, L, nblocks, shard_len, d_mismatch, d_located,
                                               static_cast<uint8_t*>(d_work), static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_scrub_pair_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                                 uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch,
                                 size_t nblocks, size_t shard_len, int32_t* located_host, uint64_t* counts, int device,
                                 void* stream_) {
    return guarded([&]() -> int {
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        if (!rs || !counts || !rs->codec->locate_pair_plan()) return SHMR_EC_INVALID_ARGUMENT;
        // (an empty batch is accepted)
        if (nblocks == 0) std::fill(counts, counts + 4, uint64_t(0));
        Codec& c = *rs->codec;
        return batch_dev(nblocks, shard_len, device, [&] { return arg_ok(d_data && d_parity); }, [&]() -> int {
            int rc = core::refuse_capture(device, stream);   // it waits for its own results
            if (rc) return rc;
            std::fill(counts, counts + 4, uint64_t(0));
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            // pooled scratch (grown without a free): the words, the answers, the location's own
            const size_t words_bytes = size_t(core::round_up(nblocks * sizeof(uint32_t), 256));
            core::StagingLease lease;
            lease.s = core::StagingPool::get().acquire(
                device, 3 * words_bytes + core::locate_pair_work_bytes(c, nblocks), &rc);
            if (!lease.s) return rc;
            uint32_t* d_words = reinterpret_cast<uint32_t*>(lease.s->dbuf);
            int32_t* d_located = reinterpret_cast<int32_t*>(lease.s->dbuf + words_bytes);
            uint8_t* d_work = lease.s->dbuf + 3 * words_bytes;
            // (a failure below still waits: the scratch goes back to the pool idle)
            auto fetch = [&](void* dst, const void* src, size_t n) -> int {
                const hipError_t e = hipMemcpyAsync(dst, src, n * sizeof(uint32_t), hipMemcpyDeviceToHost, stream);
                const hipError_t w = core::sync_stream(stream);
                return e == hipSuccess && w == hipSuccess ? SHMR_EC_OK : SHMR_EC_DEVICE_ERROR;
            };
            std::vector<int32_t> own;
            int32_t* located = located_host;
            if (!located) {
                own.resize(2 * nblocks);
                located = own.data();
            }
            rc = core::locate_pair_on_device(c, device, L, nblocks, shard_len, d_words, d_located, d_work, stream);
            const int frc = fetch(located, d_located, 2 * nblocks);
            if (rc || frc) return rc ? rc : frc;
            std::vector<size_t> hit;
            for (size_t b = 0; b < nblocks; ++b) {
                if (located[2 * b] >= 0) hit.push_back(b);
                else ++counts[located[2 * b] == SHMR_EC_LOCATE_CLEAN ? 0 : 3];
            }
            if (hit.empty()) return SHMR_EC_OK;
            // the located shards of every such block, rebuilt from the block's other shards
            const unsigned k = c.k(), t = k + c.p();
            std::vector<uint64_t> tab(hit.size() * t);
            std::vector<uint8_t> present(hit.size() * t, 1);
            for (size_t i = 0; i < hit.size(); ++i) {
                const size_t b = hit[i];
                for (unsigned s = 0; s < t; ++s)
                    tab[i * t + s] = s < k ? uint64_t(uintptr_t(d_data + b * data_block_pitch + s * data_shard_pitch))
                                           : uint64_t(uintptr_t(d_parity + b * parity_block_pitch +
                                                                (s - k) * parity_shard_pitch));
                present[i * t + size_t(located[2 * b])] = 0;
                if (located[2 * b + 1] >= 0) present[i * t + size_t(located[2 * b + 1])] = 0;
            }
            rc = core::ptrs_launch(c, tab.data(), present.data(), hit.size(), shard_len, false, device, stream,
                                   core::kDecode, false, false);
            // the closing verify: damage beyond what the location looked at shows here
            if (rc == SHMR_EC_OK) rc = core::verify_on_device(c, device, L, nblocks, shard_len, d_words, stream);
            std::vector<uint32_t> words(nblocks);
            const int wrc = fetch(words.data(), d_words, nblocks);
            if (rc || wrc) return rc ? rc : wrc;
            for (size_t b : hit) {
                const bool two = located[2 * b + 1] >= 0;
                if (words[b] != 0) located[2 * b] = located[2 * b + 1] = SHMR_EC_LOCATE_NONE;
                ++counts[words[b] != 0 ? 3 : (two ? 2 : 1)];
            }
            return SHMR_EC_OK;
        });
    });
}

// ---- parity delta update: writes into device-resident blocks -------------------------
int shmr_ec_update_batch_dev(shmr_ec_t* rs, uint8_t* d_data, size_t data_shard_pitch, size_t data_block_pitch,
                             uint8_t* d_parity, size_t parity_shard_pitch, size_t parity_block_pitch, size_t nblocks,
                             size_t shard_len, const shmr_ec_update* updates, size_t nupdates, const uint8_t* d_src,
                             size_t src_bytes, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        if (nupdates == 0) return SHMR_EC_OK;
        Codec& c = *rs->codec;
        shmr::update::Plan up;
        auto check = [&] {
            return arg_ok(d_data && d_parity && updates && d_src &&
                          shmr::update::plan(updates, nupdates, nblocks, c.k(), shard_len, src_bytes, &up));
        };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            const core::Layout L = batch_layout(c, d_data, data_shard_pitch, data_block_pitch, d_parity,
                                                parity_shard_pitch, parity_block_pitch);
            return core::update_on_device(c, device, L, up, d_src, static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_update_rounds(const shmr_ec_t* rs, const shmr_ec_update* updates, size_t nupdates, size_t nblocks,
                          size_t shard_len, size_t src_bytes, uint32_t* round_of, uint32_t* nrounds) {
    return guarded_light([&]() -> int {
        if (!rs || !nrounds) return SHMR_EC_INVALID_ARGUMENT;
        *nrounds = 0;
        if (nupdates == 0 || nblocks == 0) return SHMR_EC_OK;
        if (shard_len == 0) return SHMR_EC_EMPTY_SHARD;
        shmr::update::Plan up;
        if (!updates || !shmr::update::plan(updates, nupdates, nblocks, rs->codec->k(), shard_len, src_bytes, &up, false))
            return SHMR_EC_INVALID_ARGUMENT;
        if (round_of) std::copy(up.round_of.begin(), up.round_of.end(), round_of);
        *nrounds = up.nrounds;
        return SHMR_EC_OK;
    });
}

int shmr_ec_reconstruct_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                  const uint8_t* present, size_t nblocks, size_t shard_len, int data_only, int device,
                                  void* stream) {
    return guarded([&]() -> int {
        if (!rs || !present) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        // (no launch on a bad batch)
        auto check = [&] { return d_shards ? core::validate_presence(c, present, nblocks) : arg_ok(false); };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            return core::reconstruct_on_device(c, device, d_shards, shard_pitch, block_pitch, present, nblocks, shard_len,
                                               data_only != 0, static_cast<hipStream_t>(stream));
        });
    });
}

// ---- ranged reads from device-resident blocks ----------------------------------------
int shmr_ec_read_batch_dev(shmr_ec_t* rs, const uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                           const uint8_t* present, size_t nblocks, size_t shard_len, const shmr_ec_read* reads,
                           size_t nreads, uint8_t* d_dst, size_t dst_bytes, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        if (nreads == 0) return SHMR_EC_OK;
        Codec& c = *rs->codec;
        std::vector<shmr::read::Piece> pieces;
        auto check = [&] {
            return read_checks(c, d_shards && d_dst, present, nblocks, shard_len, reads, nreads, dst_bytes, &pieces);
        };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            return core::read_on_device(c, device, d_shards, shard_pitch, block_pitch, present, pieces, d_dst,
                                        static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_read_plan(shmr_ec_t* rs, const uint8_t* present, size_t nblocks, size_t shard_len,
                      const shmr_ec_read* reads, size_t nreads, size_t dst_bytes, uint8_t* rebuilt, uint32_t* npieces,
                      uint32_t* nchunks) {
    return guarded_light([&]() -> int {
        if (!rs || !npieces || !nchunks) return SHMR_EC_INVALID_ARGUMENT;
        *npieces = *nchunks = 0;
        if (nreads == 0 || nblocks == 0) return SHMR_EC_OK;
        if (shard_len == 0) return SHMR_EC_EMPTY_SHARD;
        const Codec& c = *rs->codec;
        std::vector<shmr::read::Piece> pieces;
        const int rc = read_checks(c, true, present, nblocks, shard_len, reads, nreads, dst_bytes, &pieces);
        if (rc) return rc;
        const size_t t = c.k() + c.p();
        if (rebuilt)
            for (size_t i = 0; i < nreads; ++i) rebuilt[i] = present[reads[i].block * t + reads[i].shard] ? 0 : 1;
        if (pieces.size() > 0xffffffffull) return SHMR_EC_INVALID_ARGUMENT;
        *npieces = uint32_t(pieces.size());
        *nchunks = shmr::read::count_chunks(pieces);
        return SHMR_EC_OK;
    });
}

// ---- parity delta update of degraded device-resident blocks --------------------------
int shmr_ec_update_degraded_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                      const uint8_t* present, size_t nblocks, size_t shard_len,
                                      const shmr_ec_update* updates, size_t nupdates, const uint8_t* d_src,
                                      size_t src_bytes, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        if (nupdates == 0) return SHMR_EC_OK;
        Codec& c = *rs->codec;
        shmr::update::Plan up;
        auto check = [&] {
            return update_degraded_checks(c, d_shards && d_src, present, nblocks, shard_len, updates, nupdates, src_bytes,
                                          &up, true);
        };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            return core::update_degraded_on_device(c, device, d_shards, shard_pitch, block_pitch, present, up, d_src,
                                                   static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_update_degraded_plan(shmr_ec_t* rs, const uint8_t* present, size_t nblocks, size_t shard_len,
                                 const shmr_ec_update* updates, size_t nupdates, size_t src_bytes, uint32_t* round_of,
                                 uint32_t* nrounds, uint8_t* rebuilt, uint32_t* npieces, uint32_t* nchunks) {
    return guarded_light([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        for (uint32_t* out : {nrounds, npieces, nchunks})
            if (out) *out = 0;
        if (nupdates == 0 || nblocks == 0) return SHMR_EC_OK;
        if (shard_len == 0) return SHMR_EC_EMPTY_SHARD;
        const Codec& c = *rs->codec;
        shmr::update::Plan up;
        const int rc = update_degraded_checks(c, true, present, nblocks, shard_len, updates, nupdates, src_bytes, &up,
                                              npieces || nchunks);
        if (rc) return rc;
        const size_t t = c.k() + c.p();
        if (round_of) std::copy(up.round_of.begin(), up.round_of.end(), round_of);
        if (nrounds) *nrounds = up.nrounds;
        if (rebuilt)
            for (size_t i = 0; i < nupdates; ++i) rebuilt[i] = present[updates[i].block * t + updates[i].shard] ? 0 : 1;
        if (up.pieces.size() > 0xffffffffull) return SHMR_EC_INVALID_ARGUMENT;
        if (npieces) *npieces = uint32_t(up.pieces.size());
        if (nchunks) *nchunks = shmr::degraded::count_chunks(up.pieces);
        return SHMR_EC_OK;
    });
}

// ---- checked reconstruct: the surplus shards compared while rebuilding ---------------
int shmr_ec_reconstruct_checked_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                          const uint8_t* present, size_t nblocks, size_t shard_len, int flags,
                                          uint32_t* d_mismatch, int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        const bool given = d_shards && present && words_given(d_mismatch) && (flags & ~kCheckFlags) == 0;
        // (no launch on a bad batch)
        auto check = [&] { return given ? core::validate_presence(c, present, nblocks) : arg_ok(false); };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            return core::checked_on_device(c, device, d_shards, shard_pitch, block_pitch, present, nblocks, shard_len,
                                           (flags & SHMR_EC_CHECK_DATA_ONLY) != 0,
                                           (flags & SHMR_EC_CHECK_NO_REBUILD) != 0, d_mismatch,
                                           static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_checked_rows(const shmr_ec_t* rs, const uint8_t* present, size_t nshards, uint32_t* rows) {
    return guarded_light([&]() -> int {
        if (!rs || !present || !rows) return SHMR_EC_INVALID_ARGUMENT;
        const int rc = check_pattern(rs, present, nshards);
        if (rc) return rc;
        // the present shards behind the first k present ones: always parity
        const unsigned k = rs->codec->k(), t = k + rs->codec->p();
        uint32_t mask = 0;
        unsigned seen = 0;
        for (unsigned i = 0; i < t; ++i) {
            if (!present[i]) continue;
            if (seen++ >= k) mask |= 1u << std::min(i - k, 31u);
        }
        *rows = mask;
        return SHMR_EC_OK;
    });
}

int shmr_ec_checked_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards, int flags, uint16_t* in_idx,
                         uint16_t* out_idx, uint8_t* out_rows, size_t out_rows_len, uint32_t* n_store,
                         uint32_t* n_check) {
    return guarded_light([&]() -> int {
        if (!rs || !present || !in_idx || !out_idx || !out_rows || !n_store || !n_check) return SHMR_EC_INVALID_ARGUMENT;
        if ((flags & ~kCheckFlags) != 0) return SHMR_EC_INVALID_ARGUMENT;
        int rc = check_pattern(rs, present, nshards);
        if (rc) return rc;
        std::vector<uint8_t> pr(present, present + rs->codec->k() + rs->codec->p());
        auto plan = rs->codec->checked_plan(pr, (flags & SHMR_EC_CHECK_DATA_ONLY) != 0,
                                            (flags & SHMR_EC_CHECK_NO_REBUILD) != 0);
        // (exactly k present and nothing rebuilt: an empty plan)
        if ((rc = copy_plan_out(*plan, plan->m, plan.get(), in_idx, out_idx, out_rows, out_rows_len))) return rc;
        *n_store = plan->m - plan->n_check;
        *n_check = plan->n_check;
        return SHMR_EC_OK;
    });
}

// ---- degraded blocks: locate a damaged survivor, and rebuild around it ---------------
int shmr_ec_locate_checked_plan(shmr_ec_t* rs, const uint8_t* present, size_t nshards, uint16_t* in_idx,
                                uint16_t* out_idx, uint8_t* ratio_rows, size_t ratio_rows_len, uint32_t* n_rows,
                                uint32_t* row_mask) {
    return guarded_light([&]() -> int {
        if (!rs || !present || !in_idx || !out_idx || !ratio_rows || !n_rows || !row_mask) return SHMR_EC_INVALID_ARGUMENT;
        int rc = check_pattern(rs, present, nshards);
        if (rc) return rc;
        const unsigned k = rs->codec->k();
        std::vector<uint8_t> pr(present, present + k + rs->codec->p());
        const auto cp = rs->codec->checked_plan(pr, false, true);
        const unsigned s = cp->n_check;
        bool singular = false;
        const auto lp = rs->codec->locate_checked_plan(pr, &singular);
        if (singular) return SHMR_EC_INVALID_ARGUMENT;
        if ((rc = copy_plan_out(*cp, s, lp.get(), in_idx, out_idx, ratio_rows, ratio_rows_len))) return rc;
        *n_rows = lp ? lp->m : 0;
        *row_mask = shmr::locate::row_mask(cp->out_idx.data(), s, k);
        return SHMR_EC_OK;
    });
}

int shmr_ec_locate_checked_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                     const uint8_t* present, size_t nblocks, size_t shard_len, int flags,
                                     uint32_t* d_mismatch, int32_t* d_located, void* d_work, size_t work_bytes,
                                     int device, void* stream) {
    return guarded([&]() -> int {
        if (!rs || !rs->codec->locate_plan()) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        const bool given = d_shards && present && words_given(d_mismatch) && words_given(d_located) &&
                           words_given(d_work) && work_bytes >= core::locate_work_bytes(c, nblocks) &&
                           (flags & ~kCheckFlags) == 0;
        // (no launch on a bad batch)
        auto check = [&] { return given ? core::validate_presence(c, present, nblocks) : arg_ok(false); };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            return core::locate_checked_on_device(c, device, d_shards, shard_pitch, block_pitch, present, nblocks,
                                                  shard_len, (flags & SHMR_EC_CHECK_DATA_ONLY) != 0,
                                                  (flags & SHMR_EC_CHECK_NO_REBUILD) != 0, d_mismatch, d_located,
                                                  static_cast<uint32_t*>(d_work), static_cast<hipStream_t>(stream));
        });
    });
}

int shmr_ec_reconstruct_repair_batch_dev(shmr_ec_t* rs, uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                         const uint8_t* present, size_t nblocks, size_t shard_len,
                                         int32_t* located_host, uint64_t* counts, int device, void* stream_) {
    return guarded([&]() -> int {
        hipStream_t stream = static_cast<hipStream_t>(stream_);
        return locate_rebuild_verify(
            rs, nblocks, shard_len, located_host, counts, device, stream,
            // (no launch on a bad batch)
            [&] { return d_shards && present ? core::validate_presence(*rs->codec, present, nblocks) : arg_ok(false); },
            // every absent shard rebuilt, every surplus shard compared, one pass
            [&](uint32_t* d_words, int32_t* d_located, uint32_t* d_cand) {
                return core::locate_checked_on_device(*rs->codec, device, d_shards, shard_pitch, block_pitch, present,
                                                      nblocks, shard_len, false, false, d_words, d_located, d_cand,
                                                      stream);
            },
            // a located block: its absent shards (rebuilt above from a damaged input,
            // where it was one) and the located shard, from the good survivors.
            // Every other block counts as complete here: nothing to rebuild.
            [&](const std::vector<size_t>& hit, const int32_t* located) {
                Codec& c = *rs->codec;
                const unsigned k = c.k(), t = k + c.p();
                std::vector<uint8_t> pr(nblocks * t, 1);
                for (size_t b : hit) {
                    for (unsigned i = 0; i < t; ++i) pr[b * t + i] = present[b * t + i] ? 1 : 0;
                    pr[b * t + size_t(located[b])] = 0;
                }
                return std::make_pair(
                    core::reconstruct_on_device(c, device, d_shards, shard_pitch, block_pitch, pr.data(), nblocks,
                                                shard_len, false, stream),
                    batch_layout(c, d_shards, shard_pitch, block_pitch, d_shards + k * shard_pitch, shard_pitch,
                                 block_pitch));
            });
    });
}

int shmr_ec_reconstruct_batch_dev_out(shmr_ec_t* rs, const uint8_t* d_shards, size_t shard_pitch, size_t block_pitch,
                                      const uint8_t* present, size_t nblocks, size_t shard_len, int data_only,
                                      uint8_t* d_out, size_t out_shard_pitch, size_t out_block_pitch, int device,
                                      void* stream) {
    return guarded([&]() -> int {
        if (!rs || !present) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        // (no launch on a bad batch)
        auto check = [&] { return d_shards && d_out ? core::validate_presence(c, present, nblocks) : arg_ok(false); };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            core::Layout L{d_shards, d_out, block_pitch, shard_pitch, out_block_pitch, out_shard_pitch, 0};
            L.compact = true;
            return core::reconstruct_on_device(c, device, L, present, nblocks, shard_len, data_only != 0,
                                               static_cast<hipStream_t>(stream));
        });
    });
}

// ---- device-resident shards anywhere: shard-pointer tables --------------------------
// The crate's own shape (block.rs:408-427: every shard its own Vec<u8>; :556-565:
// every None shard rebuilt into a fresh buffer) on device memory: validation
// here, dispatch in core::ptrs_launch (a slot lattice -> the strided kernels over
// its slots; else the table, from the device's table cache or uploaded on the
// caller's stream; inside a capture into the capture reserve).
static int ptrs_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const uint8_t* present, size_t nblocks,
                    size_t shard_len, int data_only, int device, void* stream_, core::OpClass op) {
    return guarded([&]() -> int {
        if (!rs || !d_shards) return SHMR_EC_INVALID_ARGUMENT;
        if (op == core::kDecode && !present) return SHMR_EC_INVALID_ARGUMENT;
        Codec& c = *rs->codec;
        auto check = [&] {
            const int rc = op == core::kDecode ? core::validate_presence(c, present, nblocks) : SHMR_EC_OK;
            return rc ? rc : arg_ok(needed_shards_given(d_shards, present, nblocks, c.k(), c.k() + c.p(), data_only != 0));
        };
        return batch_dev(nblocks, shard_len, device, check, [&] {
            static_assert(sizeof(uint8_t*) == sizeof(uint64_t), "64-bit device pointers");
            return core::ptrs_launch(c, reinterpret_cast<const uint64_t*>(d_shards), present, nblocks, shard_len,
                                     data_only != 0, device, static_cast<hipStream_t>(stream_), op, false, true);
        });
    });
}

int shmr_ec_encode_ptrs_dev(shmr_ec_t* rs, uint8_t* const* d_shards, size_t nblocks, size_t shard_len, int device,
                            void* stream) {
    return ptrs_dev(rs, d_shards, nullptr, nblocks, shard_len, 0, device, stream, core::kEncode);
}

int shmr_ec_reconstruct_ptrs_dev(shmr_ec_t* rs, uint8_t* const* d_shards, const uint8_t* present, size_t nblocks,
                                 size_t shard_len, int data_only, int device, void* stream) {
    return ptrs_dev(rs, d_shards, present, nblocks, shard_len, data_only, device, stream, core::kDecode);
}

// ---- host-buffer batches over one or more GPUs -------------------------------------
static int host_batch(shmr_ec_t* rs, uint8_t* const* host_shards, const uint8_t* present, size_t nblocks,
                      size_t shard_len, int data_only, const int* devices, int ndev, core::OpClass op) {
    return guarded([&]() -> int {
        if (!rs || !host_shards || !devices || ndev <= 0) return SHMR_EC_INVALID_ARGUMENT;
        if (op == core::kDecode && !present) return SHMR_EC_INVALID_ARGUMENT;
        if (nblocks == 0) return SHMR_EC_OK;
        if (shard_len == 0) return SHMR_EC_EMPTY_SHARD;
        Codec& c = *rs->codec;
        // (absent shards of a decode still need an output buffer)
        int rc = arg_ok(needed_shards_given(host_shards, present, nblocks, c.k(), c.k() + c.p(), data_only != 0));
        for (int d = 0; d < ndev && !rc; ++d) rc = core::check_device(devices[d]);
        if (rc) return rc;
        core::HostJob job{c, op, data_only != 0, host_shards, present, nblocks, shard_len, 64ull << 20,
                          core::copy_threads_default()};
        return core::run_host_job(job, devices, ndev);
    });
}

int shmr_ec_encode_blocks_host(shmr_ec_t* rs, uint8_t* const* host_shards, size_t nblocks, size_t shard_len,
                               const int* devices, int ndev) {
    return host_batch(rs, host_shards, nullptr, nblocks, shard_len, 0, devices, ndev, core::kEncode);
}

int shmr_ec_reconstruct_blocks_host(shmr_ec_t* rs, uint8_t* const* host_shards, const uint8_t* present,
                                    size_t nblocks, size_t shard_len, int data_only, const int* devices, int ndev) {
    return host_batch(rs, host_shards, present, nblocks, shard_len, data_only, devices, ndev, core::kDecode);
}

}  // extern "C"
