// CPU driver of the two-shard part of shmr_amd/csrc/locate_plan.hpp and of the
// pair plan a codec caches (gf256.cpp Codec::locate_pair_plan) for
// tests/test_locate_pair_plan.py.  Reads commands from stdin:
//   "limits"                  -> "pair_min_parity pair_max_data lds(pair_max_data) lds(pair_max_data + 1)"
//   "plan k p"                -> "coeffs N npairs words" (N = 0: the codec has no pair plan),
//                                then one line of N coefficient bytes
//   "index k"                 -> per candidate i < pair_count(k) a line "i e f" from pair_shards,
//                                then "ok" when pair_index_dd / pair_index_dp give i back for each
//   "resolve k p word single n w.." -> the two answers for that verify word,
//                                single answer and n pair bitmap words
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

#include "gf256.hpp"
#include "locate_plan.hpp"

namespace L = shmr::locate;

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "limits")) {
            std::printf("%u %u %u %u\n", L::pair_min_parity, L::pair_max_data, L::pair_lds_bytes(L::pair_max_data),
                        L::pair_lds_bytes(L::pair_max_data + 1));
        } else if (!std::strcmp(cmd, "plan")) {
            unsigned k, p;
            if (std::scanf("%u %u", &k, &p) != 2) return 2;
            shmr::gf::Codec c(k, p);
            const auto pp = c.locate_pair_plan();
            if (bool(pp) != L::pair_supported(k, p)) return 3;
            if (pp && (pp->k != 1 || pp->m != L::pair_coeff_count(k) || pp->rows.d.size() != pp->m ||
                       pp->image().size() % 32 != 0 || pp->image().size() < size_t(pp->m) * 32))
                return 3;
            std::printf("coeffs %u %u %u\n", pp ? pp->m : 0u, L::pair_count(k), L::pair_bitmap_words(k));
            for (unsigned i = 0; pp && i < pp->m; ++i) std::printf("%u%c", pp->rows.d[i], i + 1 == pp->m ? '\n' : ' ');
        } else if (!std::strcmp(cmd, "index")) {
            unsigned k;
            if (std::scanf("%u", &k) != 1 || k < 1) return 2;
            bool ok = true;
            for (unsigned i = 0; i < L::pair_count(k); ++i) {
                int32_t out[2];
                L::pair_shards(i, k, out);
                std::printf("%u %d %d\n", i, out[0], out[1]);
                const unsigned back = unsigned(out[1]) < k ? L::pair_index_dd(unsigned(out[0]), unsigned(out[1]), k)
                                                           : L::pair_index_dp(unsigned(out[0]), unsigned(out[1]) - k, k);
                ok = ok && back == i;
            }
            std::printf("%s\n", ok ? "ok" : "bad");
        } else if (!std::strcmp(cmd, "resolve")) {
            unsigned k, p, word, n;
            int single;
            if (std::scanf("%u %u %u %d %u", &k, &p, &word, &single, &n) != 5 || n != L::pair_bitmap_words(k)) return 2;
            std::vector<uint32_t> bm(n);
            for (auto& x : bm)
                if (std::scanf("%u", &x) != 1) return 2;
            int32_t out[2];
            L::resolve_pair(word, single, bm.data(), k, p, out);
            std::printf("%d %d\n", out[0], out[1]);
        } else {
            return 2;
        }
    }
    return 0;
}
