// top_table_check.cpp — build_top_table (nn_bvh_amd/csrc/top_table.h) on hand-made trees, host compiler only.
// For each tree: every table record is the byte copy of the record it stands for, up to its tagged references; a tagged
// reference names the slot that holds the copy of the record the original reference names; exactly the references to
// copied records are tagged; the slots are the first records of the breadth-first order; `wide` is unchanged.
// Prints one line per tree and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "../../nn_bvh_amd/csrc/top_table.h"

using namespace nnbvh;

static int g_failed = 0;
#define CHECK(cond, ...)                   \
    do {                                   \
        if (!(cond)) {                     \
            std::printf("FAILED: ");       \
            std::printf(__VA_ARGS__);      \
            std::printf("\n");             \
            g_failed = 1;                  \
            return;                        \
        }                                  \
    } while (0)

static unsigned g_rng = 12345u;
static unsigned rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// a record with recognisable box bytes; the references are filled in by the tree makers
static WideNode record(int k) {
    WideNode w;
    for (int j = 0; j < 12; ++j) w.q[j] = (float)(1000 * k + j) + 0.25f;
    w.ref0 = w.ref1 = ~(3 * k);
    w.axis = k % 3;
    w.pad = 0;
    return w;
}

// n interior records in the DFS numbering the bake uses (first child = record + 1 where it is interior); `pick` chooses
// how many of a subtree's records go to the first child
template <class Pick>
static void make_tree(std::vector<WideNode> &wide, int first, int n, Pick pick) {
    wide[(size_t)first] = record(first);
    const int rest = n - 1;
    if (rest == 0) return;
    const int left = pick(rest);  // 0 .. rest
    if (left > 0) {
        wide[(size_t)first].ref0 = first + 1;
        make_tree(wide, first + 1, left, pick);
    }
    if (rest - left > 0) {
        wide[(size_t)first].ref1 = first + 1 + left;
        make_tree(wide, first + 1 + left, rest - left, pick);
    }
}

static void check_tree(const char *name, const std::vector<WideNode> &wide, int32_t root_ref, int capacity) {
    const std::vector<WideNode> before = wide;
    const int n = (int)wide.size();
    std::vector<WideNode> table;
    std::vector<int32_t> order;
    int fetched = 0;
    const bool ok = build_top_table(
        [&](int32_t r, WideNode *out) {
            ++fetched;
            if (r < 0 || r >= n) return false;
            *out = wide[(size_t)r];
            return true;
        },
        root_ref, root_ref < 0 ? 0 : n, capacity, &table, &order);
    CHECK(ok, "%s: a fetch was out of range", name);
    CHECK(before.size() == wide.size() &&
              (before.empty() || std::memcmp(before.data(), wide.data(), before.size() * sizeof(WideNode)) == 0),
          "%s: wide changed", name);
    CHECK(table.size() == order.size() && fetched == (int)table.size(), "%s: sizes", name);
    // the expected order: plain breadth-first from the root, cut at the capacity
    std::vector<int32_t> bfs;
    if (root_ref >= 0) {
        std::deque<int32_t> q{root_ref};
        while (!q.empty()) {
            const int32_t r = q.front();
            q.pop_front();
            bfs.push_back(r);
            for (int32_t c : {wide[(size_t)r].ref0, wide[(size_t)r].ref1})
                if (c >= 0) q.push_back(c);
        }
        if ((int)bfs.size() > capacity) bfs.resize((size_t)capacity);
    }
    CHECK(bfs == order, "%s: the slots are not the first %d records breadth-first", name, capacity);
    std::vector<int> slot_of((size_t)n, -1);
    for (size_t k = 0; k < order.size(); ++k) slot_of[(size_t)order[k]] = (int)k;
    int tagged = 0, leaf = 0, outside = 0;
    for (size_t k = 0; k < table.size(); ++k) {
        const WideNode &o = wide[(size_t)order[k]], &t = table[k];
        CHECK(std::memcmp(o.q, t.q, sizeof o.q) == 0 && o.axis == t.axis && o.pad == t.pad, "%s: slot %zu is no copy", name, k);
        const int32_t orefs[2] = {o.ref0, o.ref1}, trefs[2] = {t.ref0, t.ref1};
        for (int c = 0; c < 2; ++c) {
            if (orefs[c] >= 0 && slot_of[(size_t)orefs[c]] >= 0) {
                CHECK(trefs[c] == (kTopTag | slot_of[(size_t)orefs[c]]), "%s: slot %zu child %d is not tagged with its slot", name, k, c);
                const WideNode &copy = table[(size_t)(trefs[c] & (kTopTag - 1))], &orig = wide[(size_t)orefs[c]];
                CHECK(std::memcmp(copy.q, orig.q, sizeof orig.q) == 0 && copy.axis == orig.axis,
                      "%s: the tagged slot does not hold the record it replaces", name);
                ++tagged;
            } else {
                CHECK(trefs[c] == orefs[c], "%s: slot %zu child %d changed", name, k, c);
                (orefs[c] < 0 ? leaf : outside) += 1;
            }
        }
    }
    CHECK(table.empty() || tagged == (int)table.size() - 1, "%s: every slot but the root has one tagged reference to it", name);
    std::printf("%s: records %d slots %zu tagged %d leaf %d outside %d\n", name, n, table.size(), tagged, leaf, outside);
}

int main() {
    static_assert(kTopRecords == 63 && kTopTag == (1 << 30), "the table the kernels are compiled for");
    std::vector<WideNode> w;
    // a root that is a leaf: no table
    check_tree("leaf root", w, ~0, kTopRecords);
    // one record, two leaves: a table of one
    w.assign(1, record(0));
    check_tree("one record", w, 0, kTopRecords);
    // a full tree below the capacity: the whole tree
    w.assign(31, WideNode{});
    make_tree(w, 0, 31, [](int rest) { return rest / 2; });
    check_tree("full 31", w, 0, kTopRecords);
    // exactly the capacity, and one more
    w.assign(63, WideNode{});
    make_tree(w, 0, 63, [](int rest) { return rest / 2; });
    check_tree("full 63", w, 0, kTopRecords);
    w.assign(64, WideNode{});
    make_tree(w, 0, 64, [](int rest) { return (rest + 1) / 2; });
    check_tree("64", w, 0, kTopRecords);
    // a chain (each record one interior child, first or second in turn) longer than the capacity
    w.assign(200, WideNode{});
    make_tree(w, 0, 200, [](int rest) { return (rest & 1) ? rest : 0; });
    check_tree("chain 200", w, 0, kTopRecords);
    // random shapes well above the capacity: copied records with leaf, copied and not-copied children
    for (int k = 0; k < 4; ++k) {
        w.assign(500, WideNode{});
        make_tree(w, 0, 500, [](int rest) { return (int)(rnd() % (unsigned)(rest + 1)); });
        check_tree("random 500", w, 0, kTopRecords);
    }
    // small capacities
    check_tree("random 500, capacity 1", w, 0, 1);
    check_tree("random 500, capacity 2", w, 0, 2);
    return g_failed;
}
