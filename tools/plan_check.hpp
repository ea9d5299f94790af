// What tools/update_plan_check.cpp and tools/read_plan_check.cpp share: the
// scan of a request list, the check that the pieces tile their requests, the
// chunks of the shared rule and the "find" command (shmr_amd/csrc/piece_plan.hpp).
#pragma once

#include <cinttypes>
#include <cstdint>
#include <cstdio>
#include <vector>

#include "piece_plan.hpp"

namespace plan_check {

namespace pc = shmr::piece;

// n x "block shard offset len flat_offset" into v (T: shmr_ec_update / shmr_ec_read).
template <class T>
bool scan_requests(std::vector<T>* v, uint64_t T::*flat) {
    for (T& x : *v)
        if (std::scanf("%" SCNu32 " %" SCNu32 " %" SCNu64 " %" SCNu64 " %" SCNu64, &x.block, &x.shard, &x.offset, &x.len,
                       &(x.*flat)) != 5)
            return false;
    return true;
}

// What every plan must satisfy: the pieces of a request tile it exactly, in
// order, in the shard and in the flat buffer alike, and carry its fields and its
// round (round_of null: 0); vector pieces are whole chunks on chunk columns.
template <class T>
const char* check_tiling(const std::vector<T>& r, uint64_t T::*flat0, const std::vector<pc::Piece>& ps,
                         const uint32_t* round_of) {
    std::vector<std::vector<const pc::Piece*>> of(r.size());
    for (const pc::Piece& p : ps) {
        if (p.request >= r.size()) return "piece of no request";
        of[p.request].push_back(&p);
    }
    for (size_t i = 0; i < r.size(); ++i) {
        uint64_t col = r[i].offset, flat = r[i].*flat0;
        for (const pc::Piece* p : of[i]) {
            if (p->col != col || p->flat != flat || p->len == 0) return "pieces do not tile the request";
            if (p->block != r[i].block || p->shard != r[i].shard || p->round != (round_of ? round_of[i] : 0))
                return "piece fields";
            if (p->vec ? (p->col % pc::kChunk || p->len % pc::kChunk || p->len > pc::kMaxPieceBytes)
                       : p->len >= pc::kChunk || p->col / pc::kChunk != (p->col + p->len - 1) / pc::kChunk)
                return "piece shape";
            col += p->len;
            flat += p->len;
        }
        if (col != r[i].offset + r[i].len) return "pieces do not cover the request";
    }
    return nullptr;
}

// The sizes of the table chunks of `Entry`s the pieces travel in.
template <class Entry>
std::vector<size_t> chunk_sizes(const std::vector<pc::Piece>& ps) {
    std::vector<size_t> out;
    for (size_t c0 = 0; c0 < ps.size(); c0 += out.back()) out.push_back(pc::chunk_pieces<Entry>(ps, c0));
    return out;
}

// "find n t0 .. t(n-1) tile" -> the index find_piece gives.
inline bool run_find() {
    unsigned n, tile;
    if (std::scanf("%u", &n) != 1 || n == 0) return false;
    std::vector<uint32_t> t0(n);
    for (auto& x : t0)
        if (std::scanf("%" SCNu32, &x) != 1) return false;
    if (std::scanf("%u", &tile) != 1) return false;
    std::printf("%u\n", pc::find_piece([&](uint32_t i) { return t0[i]; }, n, tile));
    return true;
}

}  // namespace plan_check
