// batch_plan.h -- how the mains of the misc programs cut their staged records into device batches: a pure function, so that
// tests/batch_plan_main.cpp can run it with caps of a few units where the programs use 64 MiB.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <utility>
#include <vector>

struct BatchPlan {
    std::vector<std::pair<size_t, size_t>> ranges;     // [j0, j1) of the items, in order
    int64_t max_recs = 0;                              // the most items of a batch
    std::vector<int64_t> max_cost;                     // per cost, the largest sum over a batch
};

constexpr int64_t BATCH_NO_CAP = INT64_MAX;            // a cost that is summed and closes no batch

// Items 0 .. n_items stay in order.  A batch always takes one item; it closes before the item that would make it more than max_recs
// items or carry the sum of cost(i, c) past caps[c] for any c.  Costs are not negative.
template <typename Cost> BatchPlan plan_batches(const size_t n_items, const int64_t max_recs, const std::vector<int64_t>& caps, Cost cost) {
    BatchPlan p;
    p.max_cost.assign(caps.size(), 0);
    std::vector<int64_t> sum(caps.size());
    for (size_t j = 0; j < n_items;) {
        size_t j1 = j;
        sum.assign(caps.size(), 0);
        while (j1 < n_items && (int64_t)(j1 - j) < max_recs) {
            bool fits = true;
            for (size_t c = 0; c < caps.size() && j1 > j; c++) if (cost(j1, c) > caps[c] - sum[c]) fits = false;
            if (!fits) break;
            for (size_t c = 0; c < caps.size(); c++) sum[c] += cost(j1, c);
            j1++;
        }
        if (j1 == j) { for (size_t c = 0; c < caps.size(); c++) sum[c] += cost(j1, c); j1++; }      // (max_recs < 1: one item all the same)
        p.ranges.emplace_back(j, j1);
        if ((int64_t)(j1 - j) > p.max_recs) p.max_recs = (int64_t)(j1 - j);
        for (size_t c = 0; c < caps.size(); c++) if (sum[c] > p.max_cost[c]) p.max_cost[c] = sum[c];
        j = j1;
    }
    return p;
}
