// CPU driver of shmr_amd/csrc/read_plan.hpp for tests/test_read_plan.py.
// Reads commands from stdin:
//   "rule"  -> "chunk C tile T maxpiece M entry E table N" (bytes of a vector
//              access, of a tile, of the largest piece, of a table entry; the
//              entries of one table chunk)
//   "plan nblocks k shard_len dst_bytes n" + n x "block shard offset len dst_offset"
//           -> "invalid", or "ok npieces nchunks", then per piece
//              "read block shard col len dst vec tiles tile0" (tile0: the tile
//              prefix within the piece's table chunk), pieces in list order
//   "fuzz seed n nblocks k shard_len"
//           -> a seeded list of n requests valid by construction (random source
//              ranges, destinations packed back to back in a shuffled order),
//              planned and checked here: "ok npieces nchunks", or "bad <what>"
//   "find n t0 .. t(n-1) tile" -> the index find_piece gives
#include <algorithm>
#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <random>
#include <vector>

#include "plan_check.hpp"
#include "read_plan.hpp"

namespace rd = shmr::read;

// The tile prefix of every piece within its table chunk, as the driver fills it.
static std::vector<uint32_t> tile_prefixes(const std::vector<rd::Piece>& ps) {
    std::vector<uint32_t> t0(ps.size());
    for (size_t c0 = 0; c0 < ps.size();) {
        const size_t cnt = rd::chunk_pieces<rd::DevPiece>(ps, c0);
        uint32_t tiles = 0;
        for (size_t i = 0; i < cnt; ++i) {
            t0[c0 + i] = tiles;
            tiles += rd::piece_tiles(ps[c0 + i].len);
        }
        c0 += cnt;
    }
    return t0;
}

// What every plan must satisfy: the pieces of a request tile it exactly, source
// and destination alike (plan_check.hpp), in list order; every tile of a chunk
// is found in its own piece.
static const char* check(const std::vector<shmr_ec_read>& r, const std::vector<rd::Piece>& ps) {
    if (const char* bad = plan_check::check_tiling(r, &shmr_ec_read::dst_offset, ps, nullptr)) return bad;
    for (size_t i = 1; i < ps.size(); ++i)
        if (ps[i - 1].request > ps[i].request) return "pieces not in list order";
    const std::vector<uint32_t> t0 = tile_prefixes(ps);
    for (size_t c0 = 0; c0 < ps.size();) {
        const size_t cnt = rd::chunk_pieces<rd::DevPiece>(ps, c0);
        if (cnt == 0 || cnt > rd::kTablePieces) return "chunk size";
        for (size_t i = 0; i < cnt; ++i) {
            const uint32_t first = t0[c0 + i], last = first + rd::piece_tiles(ps[c0 + i].len) - 1;
            for (uint32_t tile : {first, last})
                if (rd::find_piece([&](uint32_t j) { return t0[c0 + j]; }, uint32_t(cnt), tile) != i)
                    return "tile found in another piece";
        }
        c0 += cnt;
    }
    return nullptr;
}

int main() {
    char cmd[16];
    while (std::scanf("%15s", cmd) == 1) {
        if (!std::strcmp(cmd, "rule")) {
            std::printf("chunk %u tile %u maxpiece %" PRIu64 " entry %zu table %zu\n", rd::kChunk, rd::kTileBytes,
                        rd::kMaxPieceBytes, sizeof(rd::DevPiece), rd::kTablePieces);
        } else if (!std::strcmp(cmd, "plan")) {
            uint64_t nblocks, shard_len, dst_bytes, n;
            unsigned k;
            if (std::scanf("%" SCNu64 " %u %" SCNu64 " %" SCNu64 " %" SCNu64, &nblocks, &k, &shard_len, &dst_bytes, &n) != 5)
                return 2;
            std::vector<shmr_ec_read> r(n);
            if (!plan_check::scan_requests(&r, &shmr_ec_read::dst_offset)) return 2;
            std::vector<rd::Piece> ps;
            if (!rd::plan(r.data(), r.size(), nblocks, k, shard_len, dst_bytes, &ps)) {
                std::printf("invalid\n");
                continue;
            }
            if (const char* bad = check(r, ps)) {
                std::printf("bad %s\n", bad);
                continue;
            }
            std::printf("ok %zu %u\n", ps.size(), rd::count_chunks(ps));
            const std::vector<uint32_t> t0 = tile_prefixes(ps);
            for (size_t i = 0; i < ps.size(); ++i) {
                const rd::Piece& p = ps[i];
                std::printf("%" PRIu64 " %u %u %" PRIu64 " %u %" PRIu64 " %d %u %u\n", p.request, p.block, p.shard, p.col,
                            p.len, p.flat, int(p.vec), rd::piece_tiles(p.len), t0[i]);
            }
        } else if (!std::strcmp(cmd, "fuzz")) {
            uint64_t seed, n, nblocks, shard_len;
            unsigned k;
            if (std::scanf("%" SCNu64 " %" SCNu64 " %" SCNu64 " %u %" SCNu64, &seed, &n, &nblocks, &k, &shard_len) != 5)
                return 2;
            if (!nblocks || !k || !shard_len) return 2;
            std::mt19937_64 rng(seed);
            std::vector<shmr_ec_read> r(n);
            for (auto& x : r) {
                x.block = uint32_t(rng() % nblocks);
                x.shard = uint32_t(rng() % k);
                x.offset = rng() % shard_len;
                x.len = 1 + rng() % std::min<uint64_t>(shard_len - x.offset, 9000);
            }
            // destinations back to back, in another order than the list's
            std::vector<size_t> order(n);
            for (size_t i = 0; i < n; ++i) order[i] = i;
            std::shuffle(order.begin(), order.end(), rng);
            uint64_t dst = 3;
            for (size_t i : order) {
                r[i].dst_offset = dst;
                dst += r[i].len;
            }
            std::vector<rd::Piece> ps;
            if (!rd::plan(r.data(), r.size(), nblocks, k, shard_len, dst, &ps)) {
                std::printf("bad refused\n");
                continue;
            }
            if (const char* bad = check(r, ps)) std::printf("bad %s\n", bad);
            else std::printf("ok %zu %u\n", ps.size(), rd::count_chunks(ps));
        } else if (!std::strcmp(cmd, "find")) {
            if (!plan_check::run_find()) return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
