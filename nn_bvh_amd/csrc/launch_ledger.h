// launch_ledger.h — the launch ledger of one kernel family (nnbvh_instance_launches): how often each of the N instances
// of its table has been enqueued in this process.  Host memory, process-wide; no device is touched.
#pragma once
#include <stdint.h>

#include <array>
#include <atomic>

namespace nnbvh {

template <int N>
struct LaunchLedger {
    std::atomic<uint64_t> launches[N];  // one count per row of the family's table, in its order

    void count(int row) { launches[row].fetch_add(1, std::memory_order_relaxed); }

    // Up to `capacity` rows: desc gets 7 ints per instance (describe(row): the instance's fields, zero-padded), counts its
    // count; either may be null.  reset: the counts are zeroed after they are read.  Returns the number of instances.
    template <class Describe>
    int read(int32_t *desc, uint64_t *counts, int capacity, int reset, Describe describe) {
        for (int i = 0; i < N; ++i) {
            const uint64_t c = reset ? launches[i].exchange(0, std::memory_order_relaxed)
                                     : launches[i].load(std::memory_order_relaxed);
            if (i >= capacity) continue;
            if (counts) counts[i] = c;
            const std::array<int32_t, 7> row = describe(i);
            for (int j = 0; desc && j < 7; ++j) desc[7 * i + j] = row[j];
        }
        return N;
    }
};

}  // namespace nnbvh
