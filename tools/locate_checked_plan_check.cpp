// CPU driver of the degraded half of shmr_amd/csrc/locate_plan.hpp and of the
// per-pattern ratio plan a codec caches (gf256.cpp Codec::locate_checked_plan)
// for tests/test_locate_checked_plan.py.  Reads commands from stdin:
//   "plan k p f0 .. f(k+p-1)"  -> "plan s R mask" (R ratio rows; "singular" instead
//                                 where some D[0][t] is 0), then one line in_idx,
//                                 one line out_idx (s entries, "-" for none), s
//                                 lines of D and R lines of ratio rows, k numbers each
//   "resolve k s mask n w.. word i0 .. i(k-1) o0 .. o(s-1)"
//                              -> locate::resolve_checked for that word, n bitmap
//                                 words and the pattern's index maps
//   "both k p word n w.."      -> "a b": locate::resolve and resolve_checked of the
//                                 complete pattern of RS(k, p)
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gf256.hpp"
#include "locate_plan.hpp"

static void print_row(const uint8_t* row, unsigned k) {
    for (unsigned j = 0; j < k; ++j) std::printf("%u%c", row[j], j + 1 == k ? '\n' : ' ');
}

static void print_idx(const uint16_t* idx, unsigned n) {
    if (n == 0) std::printf("-\n");
    for (unsigned j = 0; j < n; ++j) std::printf("%u%c", idx[j], j + 1 == n ? '\n' : ' ');
}

template <class T>
static bool read_n(std::vector<T>& v) {
    for (auto& x : v) {
        unsigned u;
        if (std::scanf("%u", &u) != 1) return false;
        x = T(u);
    }
    return true;
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "plan")) {
            unsigned k, p;
            if (std::scanf("%u %u", &k, &p) != 2) return 2;
            std::vector<uint8_t> present(k + p);
            if (!read_n(present)) return 2;
            shmr::gf::Codec c(k, p);
            const auto cp = c.checked_plan(present, false, true);
            const unsigned s = cp->n_check;
            if (cp->m != s || cp->in_idx.size() != k || cp->out_idx.size() != s) return 3;
            bool singular = false;
            const auto lp = c.locate_checked_plan(present, &singular);
            if (singular) {
                std::printf("singular\n");
                continue;
            }
            if ((s < 2) != !lp) return 3;
            if (lp && (lp->k != k || lp->m + 1 != shmr::locate::rows_used(s) || lp->in_idx != cp->in_idx ||
                       lp->out_idx.size() != lp->m || lp != c.locate_checked_plan(present)))
                return 3;   // (the second call: the cached plan)
            std::printf("plan %u %u %u\n", s, lp ? lp->m : 0u, shmr::locate::row_mask(cp->out_idx.data(), s, k));
            print_idx(cp->in_idx.data(), k);
            print_idx(cp->out_idx.data(), s);
            for (unsigned r = 0; r < s; ++r) print_row(cp->rows.row(r), k);
            for (unsigned r = 0; lp && r < lp->m; ++r) print_row(lp->rows.row(r), k);
        } else if (!std::strcmp(cmd, "resolve")) {
            unsigned k, s, mask, n, word;
            if (std::scanf("%u %u %u %u", &k, &s, &mask, &n) != 4 || n != shmr::locate::bitmap_words(k)) return 2;
            // (exact sizes: a read past an index map is the sanitizer's to report)
            std::vector<uint32_t> bm(n);
            std::vector<uint16_t> in_idx(k), out_idx(s);
            if (!read_n(bm) || std::scanf("%u", &word) != 1 || !read_n(in_idx) || !read_n(out_idx)) return 2;
            std::printf("%d\n", shmr::locate::resolve_checked(word, bm.data(), k, s, mask, in_idx.data(),
                                                              s ? out_idx.data() : nullptr));
        } else if (!std::strcmp(cmd, "both")) {
            unsigned k, p, word, n;
            if (std::scanf("%u %u %u %u", &k, &p, &word, &n) != 4 || n != shmr::locate::bitmap_words(k)) return 2;
            std::vector<uint32_t> bm(n);
            if (!read_n(bm)) return 2;
            std::vector<uint16_t> in_idx(k), out_idx(p);
            for (unsigned i = 0; i < k; ++i) in_idx[i] = uint16_t(i);
            for (unsigned r = 0; r < p; ++r) out_idx[r] = uint16_t(k + r);
            std::printf("%d %d\n", shmr::locate::resolve(word, bm.data(), k, p),
                        shmr::locate::resolve_checked(word, bm.data(), k, p, shmr::locate::row_mask(out_idx.data(), p, k),
                                                      in_idx.data(), out_idx.data()));
        } else {
            return 2;
        }
    }
    return 0;
}
