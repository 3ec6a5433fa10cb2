// top_extend.h — the extension of a block's LDS copy of the top table (top_table.h).  The scene's table
// holds the first kTopRecords records; a block of the lean one-launch kernels has room for more and fills it from
// `wide` itself, in generations: the candidates of a generation are the child references of the records the generation
// before added (the first one: of the scene's records) that are interior and not tagged yet, in slot order, child 0
// before child 1.  While slots remain the 64 B of wide[ref] go to the next slot and the parent's word becomes
// kTopTag | slot.  Every table so made is parent-closed and holds byte copies, so no result depends on its size.
//
// The slot a candidate gets is computed by TopGroupScan from ballots over groups of 64 (slot, child) pairs, the same
// code in the kernel prologue (bvh_trace.hip: a wave's ballot per group) and on the host (extend_top_table below, which
// tests/cpp/top_extend_check.cpp runs on hand-made trees and the debug entry of bvh_capi.cpp compares with a block's LDS).
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

#include "nnbvh_internal.h"

namespace nnbvh {

// records a block's LDS table holds when it has `block_threads` threads and the CU's 160 KiB are shared by 2048 lanes:
// 64 KiB of stack windows per 1024 lanes, the rest for the tables.  255, 127, 63 (the scene's table alone).
constexpr int top_lds_records(int block_threads) { return block_threads / 4 - 1; }

// a child reference the extension copies: an interior record that is not in the table yet
NNBVH_HD inline bool top_is_candidate(int32_t ref) { return ref >= 0 && (ref & kTopTag) == 0; }

NNBVH_HD inline int top_popcount(unsigned long long m) { return __builtin_popcountll(m); }

// One generation's slot assignment.  The (slot, child) pairs of the scanned records are numbered 2 * (slot - begin) +
// child and taken in groups of 64; add() is called once per group, in order, with the group's candidate mask (bit b =
// pair 64 * g + b is a candidate); `mine` is the group of the caller's own pair.  Then slot(b, next, capacity) is the
// table slot of the candidate at bit b of that group, -1 where the capacity ends before it, and `total` the number of
// candidates of the generation.
struct TopGroupScan {
    int before = 0, total = 0;
    unsigned long long own = 0ull;
    NNBVH_HD void add(int g, int mine, unsigned long long mask) {
        const int n = top_popcount(mask);
        before += g < mine ? n : 0;
        own = g == mine ? mask : own;
        total += n;
    }
    NNBVH_HD int slot(int bit, int next, int capacity) const {
        const int s = next + before + top_popcount(own & ((1ull << bit) - 1ull));
        return s < capacity ? s : -1;
    }
};

// The host's form of the prologue: extends `table` (the scene's table, build_top_table) to at most `capacity` records,
// group by group as a block does.  order[k] = the record of `wide` slot k copies (appended to).  fetch as in
// build_top_table.  An empty table stays empty.
template <class Fetch>
bool extend_top_table(Fetch fetch, int capacity, std::vector<WideNode> *table, std::vector<int32_t> *order) {
    int begin = 0, next = (int)table->size();
    while (next < capacity && begin < next) {
        const int end = next, n_pairs = 2 * (end - begin), n_groups = (n_pairs + 63) >> 6;
        const auto ref_of = [&](int pair) -> int32_t & {
            WideNode &w = (*table)[(size_t)(begin + (pair >> 1))];
            return (pair & 1) ? w.ref1 : w.ref0;
        };
        std::vector<unsigned long long> masks((size_t)n_groups, 0ull);
        for (int pair = 0; pair < n_pairs; ++pair)
            if (top_is_candidate(ref_of(pair))) masks[(size_t)(pair >> 6)] |= 1ull << (pair & 63);
        int total = 0;
        table->resize((size_t)std::min(capacity, next + n_pairs));  // (cut to the records added below)
        for (int mine = 0; mine < n_groups; ++mine) {
            TopGroupScan scan;
            for (int g = 0; g < n_groups; ++g) scan.add(g, mine, masks[(size_t)g]);
            total = scan.total;
            for (int bit = 0; bit < 64; ++bit) {
                if (!((masks[(size_t)mine] >> bit) & 1ull)) continue;
                const int slot = scan.slot(bit, next, capacity);
                if (slot < 0) continue;
                int32_t &ref = ref_of(64 * mine + bit);
                WideNode w;
                if (!fetch(ref, &w)) return false;
                (*table)[(size_t)slot] = w;
                order->push_back(ref);
                ref = kTopTag | slot;
            }
        }
        begin = end;
        next = std::min(capacity, next + total);
        table->resize((size_t)next);
    }
    return true;
}

}  // namespace nnbvh
