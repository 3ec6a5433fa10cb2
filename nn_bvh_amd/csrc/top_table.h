// top_table.h — the top table of a flat scene: the first records of the baked tree, breadth-first from the root, as the
// lean one-launch kernels keep them in LDS (bvh_trace.hip).  Host code without HIP:
// tests/cpp/top_table_check.cpp builds tables of hand-made trees with the host compiler alone.
#pragma once
#include <cstdint>
#include <vector>

#include "nnbvh_internal.h"

namespace nnbvh {

// Walks the records breadth-first from root_ref and copies the first `capacity` of them: table[k] is the byte copy of
// record order[k], except that a child reference to a record that is copied too reads kTopTag | its slot.  The root is
// slot 0.  fetch(record, &out) hands out one record of `wide` (which is only read) and returns false on failure, which
// the function passes on.  A root that is a leaf, or a scene without interior records, gives an empty table.  A
// reference outside [0, n_interior) is left as it is and not followed.
template <class Fetch>
bool build_top_table(Fetch fetch, int32_t root_ref, int n_interior, int capacity, std::vector<WideNode> *table,
                     std::vector<int32_t> *order) {
    table->clear();
    order->clear();
    if (root_ref < 0 || root_ref >= n_interior || capacity < 1) return true;
    order->push_back(root_ref);
    for (size_t k = 0; k < order->size(); ++k) {
        WideNode w;
        if (!fetch((*order)[k], &w)) return false;
        for (int32_t *ref : {&w.ref0, &w.ref1}) {
            if (*ref < 0 || *ref >= n_interior || (int)order->size() >= capacity) continue;
            const int32_t slot = (int32_t)order->size();
            order->push_back(*ref);
            *ref = kTopTag | slot;
        }
        table->push_back(w);
    }
    return true;
}

}  // namespace nnbvh
