// top_extend_check.cpp — extend_top_table (nn_bvh_amd/csrc/top_extend.h: the slot assignment the kernel prologue runs,
// TopGroupScan over ballot groups) on hand-made trees, host compiler only.  For each tree and capacity the scene's table
// (build_top_table, 63 records) is extended and checked: the table is parent-closed (every slot but the root is named by
// exactly one tagged reference, in a lower slot); a tagged reference names the slot that holds the byte copy of the
// record the original reference names; exactly the references to copied records are tagged; nothing is fetched through a
// tagged or foreign reference, so no tagged word comes out of `wide`; the slots are the first records of the
// breadth-first order, as many as the capacity and the tree allow; `wide` is unchanged.
// Prints one line per case and returns 0, or says what failed and returns 1.
#include <cstdio>
#include <cstring>
#include <deque>
#include <vector>

#include "../../nn_bvh_amd/csrc/top_extend.h"
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

static unsigned g_rng = 2024u;
static unsigned rnd() {
    g_rng = g_rng * 1664525u + 1013904223u;
    return g_rng >> 8;
}

// a record with recognisable box bytes and two leaves; the tree makers fill in interior references
static WideNode record(int k) {
    WideNode w;
    for (int j = 0; j < 12; ++j) w.q[j] = (float)(1000 * k + j) + 0.25f;
    w.ref0 = w.ref1 = ~(3 * k);
    w.axis = k % 3;
    w.pad = 0;
    return w;
}

// n interior records in the depth-first numbering the bake uses; pick(rest, depth) = how many of a subtree's other
// records go to the first child
template <class Pick>
static void make_tree(std::vector<WideNode> &wide, int first, int n, int depth, Pick pick) {
    wide[(size_t)first] = record(first);
    const int rest = n - 1;
    if (rest == 0) return;
    const int left = pick(rest, depth);  // 0 .. rest
    if (left > 0) {
        wide[(size_t)first].ref0 = first + 1;
        make_tree(wide, first + 1, left, depth + 1, pick);
    }
    if (rest - left > 0) {
        wide[(size_t)first].ref1 = first + 1 + left;
        make_tree(wide, first + 1 + left, rest - left, depth + 1, pick);
    }
}

static void check_tree(const char *name, const std::vector<WideNode> &wide, int capacity) {
    const std::vector<WideNode> before = wide;
    const int n = (int)wide.size();
    std::vector<WideNode> table;
    std::vector<int32_t> order;
    int bad_fetches = 0;
    const auto fetch = [&](int32_t r, WideNode *out) {
        if (r < 0 || r >= n) {  // a tagged reference is far above n
            ++bad_fetches;
            return false;
        }
        *out = wide[(size_t)r];
        return true;
    };
    CHECK(build_top_table(fetch, 0, n, kTopRecords, &table, &order), "%s: the scene's table", name);
    const size_t n_scene = table.size();
    CHECK(extend_top_table(fetch, capacity, &table, &order) && bad_fetches == 0, "%s: a fetch through a tagged or foreign reference", name);
    CHECK(std::memcmp(before.data(), wide.data(), before.size() * sizeof(WideNode)) == 0, "%s: wide changed", name);
    CHECK(table.size() == order.size() && table.size() >= n_scene, "%s: sizes", name);
    // the expected slots: plain breadth-first order, as far as the capacity (at least the scene's table) reaches
    std::vector<int32_t> bfs;
    std::deque<int32_t> queue{0};
    while (!queue.empty()) {
        const int32_t r = queue.front();
        queue.pop_front();
        bfs.push_back(r);
        for (int32_t c : {wide[(size_t)r].ref0, wide[(size_t)r].ref1}) {
            CHECK(c < 0 || (c & kTopTag) == 0, "%s: a tagged word in wide", name);
            if (c >= 0) queue.push_back(c);
        }
    }
    CHECK((int)bfs.size() == n, "%s: the tree maker lost records", name);
    if (bfs.size() > std::max((size_t)capacity, n_scene)) bfs.resize(std::max((size_t)capacity, n_scene));
    CHECK(bfs == order, "%s: %zu slots, not the first %zu records breadth-first", name, order.size(), bfs.size());
    std::vector<int> slot_of((size_t)n, -1), named((size_t)table.size(), 0);
    for (size_t k = 0; k < order.size(); ++k) slot_of[(size_t)order[k]] = (int)k;
    int tagged = 0, leaf = 0, outside = 0;
    for (size_t k = 0; k < table.size(); ++k) {
        const WideNode &o = wide[(size_t)order[k]], &t = table[k];
        CHECK(std::memcmp(o.q, t.q, sizeof o.q) == 0 && o.axis == t.axis && o.pad == t.pad, "%s: slot %zu is no copy", name, k);
        const int32_t orefs[2] = {o.ref0, o.ref1}, trefs[2] = {t.ref0, t.ref1};
        for (int c = 0; c < 2; ++c) {
            if (orefs[c] >= 0 && slot_of[(size_t)orefs[c]] >= 0) {
                const int s = slot_of[(size_t)orefs[c]];
                CHECK(trefs[c] == (kTopTag | s), "%s: slot %zu child %d is not tagged with its slot", name, k, c);
                CHECK(s > (int)k, "%s: slot %zu child %d names a lower slot", name, k, c);
                const WideNode &copy = table[(size_t)s], &orig = wide[(size_t)orefs[c]];
                CHECK(std::memcmp(copy.q, orig.q, sizeof orig.q) == 0 && copy.axis == orig.axis,
                      "%s: the tagged slot does not hold the record it replaces", name);
                named[(size_t)s] += 1;
                ++tagged;
            } else {
                CHECK(trefs[c] == orefs[c], "%s: slot %zu child %d changed", name, k, c);
                (orefs[c] < 0 ? leaf : outside) += 1;
            }
        }
    }
    for (size_t k = 0; k < table.size(); ++k)
        CHECK(named[k] == (k == 0 ? 0 : 1), "%s: slot %zu is named by %d tagged references", name, k, named[k]);
    std::printf("%s, capacity %d: records %d slots %zu tagged %d leaf %d outside %d\n", name, capacity, n, table.size(),
                tagged, leaf, outside);
}

int main() {
    static_assert(top_lds_records(1024) == 255 && top_lds_records(512) == 127 && top_lds_records(256) == kTopRecords,
                  "the tables the kernels are compiled for");
    const auto half = [](int rest, int) { return rest / 2; };
    const auto random = [](int rest, int) { return (int)(rnd() % (unsigned)(rest + 1)); };
    std::vector<WideNode> w;
    const auto balanced = [&](int n) {
        w.assign((size_t)n, WideNode{});
        make_tree(w, 0, n, 0, half);
    };
    // fewer records than the scene's table holds: nothing to add
    w.assign(1, record(0));
    check_tree("one record", w, 255);
    balanced(31);
    check_tree("balanced 31", w, 255);
    w.assign(50, WideNode{});
    make_tree(w, 0, 50, 0, random);
    check_tree("random 50", w, 255);
    balanced(63);
    check_tree("balanced 63", w, 255);
    // a few more: one generation of 1 .. 12 records
    for (int n = 64; n <= 75; ++n) {
        balanced(n);
        check_tree("balanced 64..75", w, 255);
    }
    // one generation partly filled; two generations, the second partly filled
    balanced(100);
    check_tree("balanced 100", w, 255);
    balanced(150);
    check_tree("balanced 150", w, 255);
    // the capacity is reached inside the second generation (255), inside the first (127) and at a generation's end
    balanced(300);
    check_tree("balanced 300", w, 255);
    check_tree("balanced 300", w, 127);
    check_tree("balanced 300", w, 100);
    check_tree("balanced 300", w, 200);
    for (int k = 0; k < 4; ++k) {
        w.assign(300 + 100 * (size_t)k, WideNode{});
        make_tree(w, 0, (int)w.size(), 0, random);
        check_tree("random 300..600", w, 255);
        check_tree("random 300..600", w, 127);
    }
    // a capacity no larger than the scene's table: the table stays as it is
    check_tree("random 600", w, 63);
    check_tree("random 600", w, 10);
    // a chain (each record one interior child, first or second in turn): one record per generation
    w.assign(200, WideNode{});
    make_tree(w, 0, 200, 0, [](int rest, int) { return (rest & 1) ? rest : 0; });
    check_tree("chain 200", w, 255);
    check_tree("chain 200", w, 127);
    w.assign(300, WideNode{});
    make_tree(w, 0, 300, 0, [](int rest, int) { return (rest & 1) ? rest : 0; });
    check_tree("chain 300", w, 255);
    // a record of level 5 with a leaf child (its other subtree takes all its records), and one with two leaves, in an
    // otherwise balanced tree: the generations below them have gaps
    w.assign(400, WideNode{});
    {
        int at5 = 0;
        make_tree(w, 0, 400, 0, [&](int rest, int depth) {
            if (depth == 5 && ++at5 == 3) return 0;
            if (depth == 4 && at5 > 8 && rest > 1) return 1;  // its first child: a level-5 record with two leaves
            return rest / 2;
        });
    }
    check_tree("leaf children at level 5", w, 255);
    check_tree("leaf children at level 5", w, 127);
    return g_failed;
}
