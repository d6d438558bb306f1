// deliver_group.hpp — the host side of the receive ring's grouping
// (deliver_host.cpp): plain C++17 with no HIP, so that
// tests/cpp/ring_group_host.cpp runs it stand-alone under sanitizers.
#pragma once
#include <cstdint>
#include "../../include/lneto_amd.h"

namespace lnxd {

constexpr uint32_t kGroupBuckets = LNX_H_COUNT + 1u;  // handler ids, then the frames not delivered

// The call's grouping from its internal batches'.  Batch b holds frames
// [first[b], first[b] + n[b]) of the call; batch_order + first[b] is its order
// (n[b] batch-local indices, grouped by bucket) and batch_count + kGroupBuckets b
// its bucket sizes.  order (the sum of n[b] entries) becomes the stable
// concatenation: for every bucket in ascending order, and for the batches in
// arrival order, the batch's run of that bucket with first[b] added;
// count[h] the bucket's size over the call.  order may alias nothing.
void merge_groups(const uint32_t* batch_order, const uint32_t* batch_count, const uint32_t* first, const uint32_t* n,
                  uint32_t nbatches, uint32_t* order, uint32_t* count);

// The same from the records themselves (the ring's host path): a stable
// counting sort of the n frames by bucket (the handler id, LNX_H_COUNT for a
// frame not delivered).
void group_records(const lnx_rx_delivery* rec, uint64_t n, uint32_t* order, uint32_t* count);

}  // namespace lnxd
