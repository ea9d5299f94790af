// Stand-alone CPU check of Codec::checked_plan (shmr_amd/csrc/gf256.cpp), also the
// program the host sanitizers run over it:
//
//   g++ -std=c++17 -O1 -g -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I shmr_amd/csrc tools/checked_plan_check.cpp shmr_amd/csrc/gf256.cpp -lpthread
//
// Over every presence pattern of RS(4,2) and RS(8,3) and a seeded sample of
// RS(10,4), RS(5,6), RS(4,6) and RS(2,34) (exactly k present, every shard
// present and random erasures), under each flag combination, it checks without
// a matrix inverse of its own:
//   - inputs: the first k present shards;
//   - stored rows: reconstruct_plan's rows and shards, verbatim (none with
//     no_rebuild or with every shard present);
//   - check rows: one per surplus shard in ascending index, all parity shards,
//     with row * M[inputs] == M[surplus shard] (so row == M[shard] * inv(M[inputs])),
//     every coefficient non-zero (MDS);
//   - a second request returns the cached plan.
// Prints "ok <plans>" or the first violation.
#include <cstdint>
#include <cstdio>
#include <random>
#include <vector>

#include "gf256.hpp"

namespace gf = shmr::gf;

static const char* check(gf::Codec& c, const std::vector<uint8_t>& pr, bool data_only, bool no_rebuild) {
    const unsigned k = c.k(), t = k + c.p();
    std::vector<uint16_t> valid, surplus;
    unsigned absent = 0;
    for (unsigned i = 0; i < t; ++i) {
        if (!pr[i]) ++absent;
        else if (valid.size() < k) valid.push_back(uint16_t(i));
        else surplus.push_back(uint16_t(i));
    }
    auto plan = c.checked_plan(pr, data_only, no_rebuild);
    if (c.checked_plan(pr, data_only, no_rebuild) != plan) return "plan not cached";
    if (plan->k != k || plan->in_idx != valid) return "inputs are not the first k present";
    if (plan->n_check != surplus.size() || plan->m < plan->n_check || plan->out_idx.size() != plan->m ||
        plan->rows.rows != plan->m || plan->rows.cols != k)
        return "shape";
    const unsigned m_store = plan->m - plan->n_check;
    if (absent && !no_rebuild) {
        auto rp = c.reconstruct_plan(pr, data_only);
        if (rp->m != m_store) return "stored row count";
        for (unsigned r = 0; r < m_store; ++r) {
            if (rp->out_idx[r] != plan->out_idx[r]) return "stored shard";
            for (unsigned j = 0; j < k; ++j)
                if (rp->rows.at(r, j) != plan->rows.at(r, j)) return "stored row differs from reconstruct_plan";
        }
    } else if (m_store) {
        return "stored rows without a rebuild";
    }
    for (unsigned s = 0; s < surplus.size(); ++s) {
        const unsigned j = surplus[s], r = m_store + s;
        if (j < k) return "surplus data shard";
        if (plan->out_idx[r] != j) return "check rows not in ascending shard order";
        for (unsigned col = 0; col < k; ++col) {
            if (!plan->rows.at(r, col)) return "zero coefficient in a check row";
            uint8_t acc = 0;
            for (unsigned i = 0; i < k; ++i) acc ^= gf::mul(plan->rows.at(r, i), c.matrix().at(valid[i], col));
            if (acc != c.matrix().at(j, col)) return "check row * M[inputs] != M[surplus]";
        }
    }
    const std::vector<uint8_t> img = plan->image();
    if (img.size() < 32 + size_t(32) * k * plan->m) return "image size";
    return nullptr;
}

int main() {
    struct Code {
        unsigned k, p, sample;
    };
    const Code codes[] = {{4, 2, 0}, {8, 3, 0}, {10, 4, 200}, {5, 6, 200}, {4, 6, 200}, {2, 34, 200}};
    size_t plans = 0;
    for (const Code& cd : codes) {
        gf::Codec c(cd.k, cd.p);
        const unsigned k = cd.k, t = cd.k + cd.p;
        std::vector<std::vector<uint8_t>> patterns;
        if (!cd.sample) {
            for (uint32_t bits = 0; bits < (1u << t); ++bits) {
                std::vector<uint8_t> pr(t);
                unsigned np = 0;
                for (unsigned i = 0; i < t; ++i) np += (pr[i] = (bits >> i) & 1);
                if (np >= k) patterns.push_back(pr);
            }
        } else {
            std::mt19937 rng(cd.k * 100 + cd.p);
            patterns.push_back(std::vector<uint8_t>(t, 1));
            std::vector<uint8_t> head(t, 0), tail(t, 0);
            for (unsigned i = 0; i < k; ++i) head[i] = tail[t - 1 - i] = 1;
            patterns.push_back(head);
            patterns.push_back(tail);
            for (unsigned n = 0; n < cd.sample; ++n) {
                std::vector<uint8_t> pr(t, 1);
                const unsigned lose = 1 + rng() % cd.p;
                for (unsigned l = 0; l < lose;) {
                    const unsigned i = rng() % t;
                    if (pr[i]) {
                        pr[i] = 0;
                        ++l;
                    }
                }
                patterns.push_back(pr);
            }
        }
        for (const auto& pr : patterns)
            for (int f = 0; f < 4; ++f) {
                const char* bad = check(c, pr, (f & 1) != 0, (f & 2) != 0);
                if (bad) {
                    std::printf("bad RS(%u,%u) flags %d: %s; present =", cd.k, cd.p, f, bad);
                    for (uint8_t x : pr) std::printf(" %u", x);
                    std::printf("\n");
                    return 1;
                }
                ++plans;
            }
    }
    std::printf("ok %zu\n", plans);
    return 0;
}
