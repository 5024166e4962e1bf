// batch_plan_main.cpp -- plan_batches (vcfgl_amd/csrc/misc/batch_plan.h) on random item lists with zero, one and two caps of 1 .. 64:
// the ranges partition the items in order, none is empty or larger than max_recs, a batch of several items is within every cap, no
// batch could have taken its successor's first item, the reported maxima are the batches' maxima, and the ranges are those of the two
// loops the programs carried before (fetchgl_main.cpp: one cap; setal_main.cpp: two caps, the second on values x 4), written out below.
// Built with -fsanitize=address,undefined by tests/test_batch_plan_cpu.py; prints "checks <n>".
#include <stdio.h>
#include <stdlib.h>

#include <algorithm>

#include "misc/batch_plan.h"

static long n_checks = 0;
#define CHECK(x) do { ++n_checks; if (!(x)) { fprintf(stderr, "%s:%d: CHECK(%s) failed (case %ld)\n", __FILE__, __LINE__, #x, n_case); exit(1); } } while (0)
static long n_case = 0;

static uint64_t rng_state = 0x9E3779B97F4A7C15ull;
static uint64_t rnd() { rng_state ^= rng_state << 13; rng_state ^= rng_state >> 7; rng_state ^= rng_state << 17; return rng_state; }
static int64_t rnd_in(int64_t lo, int64_t hi) { return lo + (int64_t)(rnd() % (uint64_t)(hi - lo + 1)); }

typedef std::vector<std::pair<size_t, size_t>> Ranges;

// fetchgl_main.cpp's loop: B records, one cap on the bytes
static Ranges loop_one_cap(const std::vector<int64_t>& bytes, const int64_t B, const int64_t TEXT_MOST, int64_t& max_text, int64_t& max_recs) {
    Ranges batches;
    max_text = 1; max_recs = 1;
    for (size_t j = 0; j < bytes.size();) {
        size_t j1 = j; int64_t t = 0;
        while (j1 < bytes.size() && (int64_t)(j1 - j) < B && (j1 == j || t + bytes[j1] <= TEXT_MOST)) t += bytes[j1++];
        batches.emplace_back(j, j1);
        max_text = std::max(max_text, t); max_recs = std::max<int64_t>(max_recs, (int64_t)(j1 - j));
        j = j1;
    }
    return batches;
}
// setal_main.cpp's loop: `batch` records, a cap on the staged bytes and the same cap on the plane values x 4
static Ranges loop_two_caps(const std::vector<int64_t>& up, const std::vector<int64_t>& vals, const int64_t batch, const int64_t MOST,
                            int64_t& max_text, int64_t& max_vals, int64_t& max_recs) {
    Ranges batches;
    max_text = 4; max_vals = 1; max_recs = 1;
    for (size_t j = 0; j < up.size();) {
        size_t j1 = j; int64_t t = 0, v = 0;
        while (j1 < up.size() && (int64_t)(j1 - j) < batch) {
            const int64_t tb = up[j1], vb = vals[j1];
            if (j1 > j && (t + tb > MOST || (v + vb) * 4 > MOST)) break;
            t += tb; v += vb; j1++;
        }
        batches.emplace_back(j, j1);
        max_text = std::max(max_text, t); max_vals = std::max(max_vals, v); max_recs = std::max<int64_t>(max_recs, (int64_t)(j1 - j));
        j = j1;
    }
    return batches;
}

// the properties every plan has; cost[c][i], caps[c]
static void check_plan(const BatchPlan& p, const size_t n, const int64_t max_recs, const std::vector<int64_t>& caps, const std::vector<std::vector<int64_t>>& cost) {
    const size_t C = caps.size();
    CHECK(p.max_cost.size() == C);
    CHECK((n == 0) == p.ranges.empty());
    size_t at = 0; int64_t most_recs = 0; std::vector<int64_t> most(C, 0);
    for (size_t b = 0; b < p.ranges.size(); b++) {
        const size_t j0 = p.ranges[b].first, j1 = p.ranges[b].second;
        CHECK(j0 == at && j1 > j0 && j1 <= n);                           // in order, none empty
        CHECK((int64_t)(j1 - j0) <= max_recs);
        at = j1;
        most_recs = std::max(most_recs, (int64_t)(j1 - j0));
        bool next_fits = j1 < n && (int64_t)(j1 - j0) < max_recs;
        for (size_t c = 0; c < C; c++) {
            int64_t sum = 0;
            for (size_t j = j0; j < j1; j++) sum += cost[c][j];
            if (j1 - j0 > 1) CHECK(sum <= caps[c]);
            most[c] = std::max(most[c], sum);
            if (j1 < n && sum + cost[c][j1] > caps[c]) next_fits = false;
        }
        CHECK(!next_fits);                                               // the batch could not have taken its successor's first item
    }
    CHECK(at == n);
    CHECK(p.max_recs == most_recs);
    for (size_t c = 0; c < C; c++) CHECK(p.max_cost[c] == most[c]);
}

static void one_case(const size_t n, const int n_caps, const bool with_giant) {
    ++n_case;
    const int64_t max_recs = rnd_in(1, 9);
    std::vector<int64_t> caps;
    for (int c = 0; c < n_caps; c++) caps.push_back(rnd_in(1, 64));
    std::vector<std::vector<int64_t>> cost(2, std::vector<int64_t>(n));
    const int64_t top = rnd_in(1, 40);
    for (size_t i = 0; i < n; i++) { cost[0][i] = rnd_in(0, top); cost[1][i] = 4 * rnd_in(0, top / 4 + 1); }
    if (with_giant && n > 0) {                                          // an item that alone exceeds a cap
        const size_t g = (size_t)rnd_in(0, (int64_t)n - 1);
        cost[0][g] = 65 + rnd_in(0, 100); cost[1][g] = 4 * (17 + rnd_in(0, 100));
    }
    const BatchPlan p = plan_batches(n, max_recs, caps, [&](size_t i, size_t c) { return cost[c][i]; });
    check_plan(p, n, max_recs, caps, cost);
    int64_t mt, mv, mr;
    if (n_caps == 0) {                                                  // blocks of max_recs items
        for (size_t b = 0; b < p.ranges.size(); b++)
            CHECK(p.ranges[b].first == b * (size_t)max_recs && p.ranges[b].second == std::min(n, (b + 1) * (size_t)max_recs));
    } else if (n_caps == 1) {
        const Ranges want = loop_one_cap(cost[0], max_recs, caps[0], mt, mr);
        CHECK(p.ranges == want);
        CHECK(std::max<int64_t>(1, p.max_cost[0]) == mt && std::max<int64_t>(1, p.max_recs) == mr);
    } else {                                                            // the programs give both costs one cap; the second is values x 4
        std::vector<int64_t> vals(n);
        for (size_t i = 0; i < n; i++) vals[i] = cost[1][i] / 4;
        const std::vector<int64_t> same{caps[0], caps[0]};
        const BatchPlan q = plan_batches(n, max_recs, same, [&](size_t i, size_t c) { return cost[c][i]; });
        check_plan(q, n, max_recs, same, cost);
        const Ranges want = loop_two_caps(cost[0], vals, max_recs, caps[0], mt, mv, mr);
        CHECK(q.ranges == want);
        CHECK(std::max<int64_t>(4, q.max_cost[0]) == mt && std::max<int64_t>(1, q.max_cost[1] / 4) == mv && std::max<int64_t>(1, q.max_recs) == mr);
    }
}

int main() {
    for (int n_caps = 0; n_caps <= 2; n_caps++) {
        one_case(0, n_caps, false);                                     // n_items = 0
        one_case(1, n_caps, true);                                      // one item, larger than every cap
        for (int k = 0; k < 1500; k++) one_case((size_t)rnd_in(0, 40), n_caps, k % 3 == 0);
    }
    // a cost that closes no batch is still summed (gtdiscordance_hip's text)
    {
        ++n_case;
        const BatchPlan p = plan_batches(10, 4, {BATCH_NO_CAP}, [](size_t i, size_t) { return (int64_t)1 << (40 + (int)i % 2); });
        CHECK(p.ranges.size() == 3 && p.ranges[2] == std::make_pair((size_t)8, (size_t)10) && p.max_recs == 4);
        CHECK(p.max_cost[0] == 2 * (((int64_t)1 << 40) + ((int64_t)1 << 41)));
    }
    printf("checks %ld cases %ld\n", n_checks, n_case);
    return 0;
}
