// Arithmetic runs of a launch's block list: what travels in the kernel
// arguments as segments (kern::Seg) instead of an uploaded list.
// Host logic only, header-only (tests/test_run_split.py compiles it on the CPU).
#pragma once

#include <cstddef>
#include <cstdint>
#include <vector>

namespace shmr {
namespace grid {

// Launch blocks [start, next run's start) are first + (j - start) * stride,
// all under plan index `plan` (0 without plan indices).
struct Run {
    uint64_t start, first, stride;
    uint32_t plan;
};

// Splits blocks[0 .. n) into its maximal arithmetic runs, greedily from the
// front: a run ends where the stride changes, where the plan index changes
// (plan_idx, nullable: one entry per block) or where the sequence stops
// ascending; a single-block run has stride 1.  Returns the number of runs, or
// limit + 1 as soon as there are more than `limit` (it stops there); `out`
// (nullable) receives the first min(runs, limit) of them.
// The slot lists of launch_slots / slots_launch_fits are ascending and distinct
// by contract (ec_core.hpp), so for them the ascending rule never ends a run.
template <class T>
size_t split_runs(const T* blocks, size_t n, const uint16_t* plan_idx, size_t limit, std::vector<Run>* out) {
    if (out) out->clear();
    size_t runs = 0;
    for (size_t i = 0; i < n;) {
        size_t e = i + 1;
        const uint64_t st = e < n ? uint64_t(blocks[e]) - uint64_t(blocks[i]) : 1;
        while (e < n && (!plan_idx || plan_idx[e] == plan_idx[i]) && blocks[e] > blocks[e - 1] &&
               uint64_t(blocks[e]) - uint64_t(blocks[e - 1]) == st)
            ++e;
        if (++runs > limit) return runs;
        if (out) out->push_back({i, uint64_t(blocks[i]), e - i > 1 ? st : 1, plan_idx ? plan_idx[i] : 0u});
        i = e;
    }
    return runs;
}

}  // namespace grid
}  // namespace shmr
