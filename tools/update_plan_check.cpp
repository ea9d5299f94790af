// CPU driver of shmr_amd/csrc/update_plan.hpp for tests/test_update_plan.py.
// Reads commands from stdin:
//   "rule"  -> "edges byte-exact" or "edges widened" (the footprint rule of the build),
//              then "chunk C tile T maxpiece M"
//   "plan nblocks k shard_len src_bytes n" + n x "block shard offset len src_offset"
//           -> "invalid", or "ok nrounds npieces", a line of the n rounds, then
//              per piece "update block shard col len src round vec tiles"
//   "chunks nblocks k shard_len src_bytes n" + the n updates as for "plan"
//           -> "invalid", or "ok" and the sizes of the table chunks the pieces
//              travel in (piece::chunk_pieces), in order
//   "fuzz seed n nblocks k shard_len"
//           -> a seeded list of n updates valid by construction (distinct
//              (block, shard, 64-column slot), random sub-range of the slot),
//              planned and checked here: "ok nrounds npieces", or "bad <what>"
//   "find n t0 .. t(n-1) tile" -> the index find_piece gives
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "plan_check.hpp"
#include "update_plan.hpp"

namespace up = shmr::update;

// What every plan must satisfy: the pieces of an update tile it exactly
// (plan_check.hpp), they come in round order, and no round holds two pieces of
// a block whose footprints (column ranges) intersect.
static const char* check(const std::vector<shmr_ec_update>& u, const up::Plan& pl) {
    for (size_t i = 1; i < pl.pieces.size(); ++i)
        if (pl.pieces[i - 1].round > pl.pieces[i].round) return "pieces not in round order";
    for (size_t i = 0; i < u.size(); ++i)
        if (pl.round_of[i] >= pl.nrounds) return "round out of range";
    if (const char* bad = plan_check::check_tiling(u, &shmr_ec_update::src_offset, pl.pieces, pl.round_of.data()))
        return bad;
    // per (block, round): ranges sorted by first column must not intersect
    std::map<std::pair<uint32_t, uint32_t>, std::vector<std::pair<uint64_t, uint64_t>>> fp;
    for (const up::Piece& p : pl.pieces) fp[{p.block, p.round}].push_back({p.col, p.col + p.len});
    for (auto& kv : fp) {
        std::sort(kv.second.begin(), kv.second.end());
        for (size_t i = 1; i < kv.second.size(); ++i)
            if (kv.second[i - 1].second > kv.second[i].first) return "footprints intersect in a round";
    }
    return nullptr;
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "rule")) {
            std::printf("edges %s\nchunk %u tile %u maxpiece %" PRIu64 "\n", up::kByteExactEdges ? "byte-exact" : "widened",
                        up::kChunk, up::kTileBytes, up::kMaxPieceBytes);
        } else if (!std::strcmp(cmd, "plan") || !std::strcmp(cmd, "chunks")) {
            uint64_t nblocks, shard_len, src_bytes, n;
            unsigned k;
            if (std::scanf("%" SCNu64 " %u %" SCNu64 " %" SCNu64 " %" SCNu64, &nblocks, &k, &shard_len, &src_bytes, &n) != 5)
                return 2;
            std::vector<shmr_ec_update> u(n);
            if (!plan_check::scan_requests(&u, &shmr_ec_update::src_offset)) return 2;
            up::Plan pl;
            if (!up::plan(u.data(), u.size(), nblocks, k, shard_len, src_bytes, &pl)) {
                std::printf("invalid\n");
                continue;
            }
            if (const char* bad = check(u, pl)) {
                std::printf("bad %s\n", bad);
                continue;
            }
            if (!std::strcmp(cmd, "chunks")) {
                std::printf("ok");
                for (size_t c : plan_check::chunk_sizes<up::DevPiece>(pl.pieces)) std::printf(" %zu", c);
                std::printf("\n");
                continue;
            }
            std::printf("ok %u %zu\n", pl.nrounds, pl.pieces.size());
            for (size_t i = 0; i < n; ++i) std::printf("%u%c", pl.round_of[i], i + 1 == n ? '\n' : ' ');
            if (!n) std::printf("\n");
            for (const up::Piece& p : pl.pieces)
                std::printf("%" PRIu64 " %u %u %" PRIu64 " %u %" PRIu64 " %u %d %u\n", p.request, p.block, p.shard, p.col,
                            p.len, p.flat, p.round, int(p.vec), up::piece_tiles(p.len));
        } else if (!std::strcmp(cmd, "fuzz")) {
            uint64_t seed, n, nblocks, shard_len;
            unsigned k;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %u %" SCNu64, &seed, &n, &nblocks, &k, &shard_len) != 5)
                return 2;
            const uint64_t slot = 64, slots = shard_len / slot;
            if (!slots || n > nblocks * k * slots) return 2;
            std::mt19937_64 rng(seed);
            std::set<std::tuple<uint32_t, uint32_t, uint64_t>> taken;
            std::vector<shmr_ec_update> u;
            uint64_t src = 0;
            while (u.size() < n) {
                const uint32_t b = uint32_t(rng() % nblocks), s = uint32_t(rng() % k);
                const uint64_t sl = rng() % slots;
                if (!taken.insert(std::make_tuple(b, s, sl)).second) continue;
                const uint64_t a = rng() % slot, len = 1 + rng() % (slot - a);
                u.push_back(shmr_ec_update{b, s, sl * slot + a, len, src});
                src += len;
            }
            up::Plan pl;
            if (!up::plan(u.data(), u.size(), nblocks, k, shard_len, src, &pl)) {
                std::printf("bad refused\n");
                continue;
            }
            if (const char* bad = check(u, pl)) std::printf("bad %s\n", bad);
            else std::printf("ok %u %zu\n", pl.nrounds, pl.pieces.size());
        } else if (!std::strcmp(cmd, "find")) {
            if (!plan_check::run_find()) return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
