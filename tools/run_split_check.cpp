// CPU driver of shmr::grid::split_runs (shmr_amd/csrc/run_split.hpp) for
// tests/test_run_split.py: reads cases "n has_plan limit" then n lines "block"
// or "block plan" from stdin; prints the returned count, then one line
// "start first stride plan" per run it was given.  Lists with plan indices are
// 32-bit blocks (a reconstruct's groups), the others 64-bit (slot lists).
#include <cstdint>
#include <cstdio>
#include <vector>

#include "run_split.hpp"

int main() {
    unsigned long long n, has_plan, limit;
    while (std::scanf("%llu %llu %llu", &n, &has_plan, &limit) == 3) {
        std::vector<uint64_t> b64(n);
        std::vector<uint32_t> b32(n);
        std::vector<uint16_t> plan(n);
        for (size_t i = 0; i < n; ++i) {
            unsigned long long b, p = 0;
            if (std::scanf("%llu", &b) != 1 || (has_plan && std::scanf("%llu", &p) != 1)) return 2;
            b64[i] = b;
            b32[i] = uint32_t(b);
            plan[i] = uint16_t(p);
        }
        std::vector<shmr::grid::Run> runs;
        const size_t count = has_plan ? shmr::grid::split_runs(b32.data(), n, plan.data(), limit, &runs)
                                      : shmr::grid::split_runs(b64.data(), n, nullptr, limit, &runs);
        if (count != shmr::grid::split_runs(b64.data(), n, has_plan ? plan.data() : nullptr, limit, nullptr)) return 3;
        std::printf("%zu %zu\n", count, runs.size());
        for (const auto& r : runs)
            std::printf("%llu %llu %llu %u\n", (unsigned long long)r.start, (unsigned long long)r.first,
                        (unsigned long long)r.stride, r.plan);
    }
    return 0;
}
