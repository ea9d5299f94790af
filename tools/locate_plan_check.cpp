// CPU driver of shmr_amd/csrc/locate_plan.hpp and of the locate plan a codec
// caches (gf256.cpp Codec::locate_plan) for tests/test_locate_plan.py.  Reads
// commands from stdin:
//   "plan k p"               -> "rows R k" (R = 0: the codec has no locate plan),
//                               then p lines of the parity matrix C and R lines
//                               of ratio rows, k numbers each
//   "ratios k R" + R*k bytes -> "ok" and R-1 lines of k ratios, or "zero"
//   "resolve k p word n w.." -> the answer for that verify word and n bitmap words
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gf256.hpp"
#include "locate_plan.hpp"

static void print_row(const uint8_t* row, unsigned k) {
    for (unsigned j = 0; j < k; ++j) std::printf("%u%c", row[j], j + 1 == k ? '\n' : ' ');
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "plan")) {
            unsigned k, p;
            if (std::scanf("%u %u", &k, &p) != 2) return 2;
            shmr::gf::Codec c(k, p);
            const auto lp = c.locate_plan();
            if (lp && (lp->k != k || lp->m + 1 != shmr::locate::rows_used(p) || lp->in_idx.size() != k ||
                       lp->out_idx.size() != lp->m))
                return 3;
            std::printf("rows %u %u\n", lp ? lp->m : 0u, k);
            for (unsigned r = 0; r < p; ++r) print_row(c.matrix().row(k + r), k);
            for (unsigned r = 0; lp && r < lp->m; ++r) print_row(lp->rows.row(r), k);
        } else if (!std::strcmp(cmd, "ratios")) {
            unsigned k, R;
            if (std::scanf("%u %u", &k, &R) != 2 || R < 1) return 2;
            std::vector<uint8_t> C(size_t(R) * k), q(size_t(R - 1) * k + 1);
            for (auto& x : C) {
                unsigned v;
                if (std::scanf("%u", &v) != 1) return 2;
                x = uint8_t(v);
            }
            if (!shmr::locate::ratio_rows(C.data(), k, R, shmr::gf::div, q.data())) {
                std::printf("zero\n");
                continue;
            }
            std::printf("ok\n");
            for (unsigned r = 0; r + 1 < R; ++r) print_row(q.data() + size_t(r) * k, k);
        } else if (!std::strcmp(cmd, "resolve")) {
            unsigned k, p, word, n;
            if (std::scanf("%u %u %u %u", &k, &p, &word, &n) != 4 || n != shmr::locate::bitmap_words(k)) return 2;
            std::vector<uint32_t> bm(n);
            for (auto& x : bm)
                if (std::scanf("%u", &x) != 1) return 2;
            std::printf("%d\n", shmr::locate::resolve(word, bm.data(), k, p));
        } else {
            return 2;
        }
    }
    return 0;
}
