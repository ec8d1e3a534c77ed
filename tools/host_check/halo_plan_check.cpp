// Host-side check of the halo merge's plan rule - hv_halo_run_rule and the host plan hv_halo_plan_host (hv_halo_plan.h, what
// hv_merge_halo_plan_held and hv_merge_halo_plan call after their argument checks) - without a GPU and without HIP.
// Meant for the address and undefined-behaviour sanitizers:
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Ipyslam_amd/csrc \
//         tools/host_check/halo_plan_check.cpp -o /tmp/halo_plan_check && /tmp/halo_plan_check
// (a plain C++ compiler will do as well: the header needs the standard library only).
// It checks (a) the host plan against a brute-force plan built from sets, on seeded random lists for worlds 1 - 8 with empty ranks,
// keys dirty where they are not held and holders that list a key twice; (b) the run rule under all_dirty_kept; (c) that the plan
// from the dirty lists alone (the held plan with the one list given twice) is "listed by two ranks or more, the lowest lister keeps".
// It prints "halo_plan_check ok" and exits 0, or names the first expectation that failed.
#include <cstdio>
#include <cstdlib>
#include <map>
#include <random>
#include <set>

#include "hv_halo_plan.h"

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

using Key = std::array<int32_t, 3>;
struct Lists { // the ranks' lists back to back, as the host plan takes them
    std::vector<int32_t> keys;
    std::vector<int64_t> counts;
    std::vector<std::set<Key>> by_rank;
    void add_rank(const std::vector<Key> &list) {
        for (const Key &k : list) keys.insert(keys.end(), k.begin(), k.end());
        counts.push_back((int64_t)list.size());
        by_rank.emplace_back(list.begin(), list.end());
    }
};
struct Plan {
    std::vector<Key> keys;
    std::vector<uint8_t> action;
    bool operator==(const Plan &o) const { return keys == o.keys && action == o.action; }
};

static Plan host_plan(const Lists &dirty, const Lists &held, int world, int rank) {
    // the size query first, then a buffer of exactly that size and a sentinel behind it
    const int64_t n = hv_halo_plan_host(dirty.keys.data(), dirty.counts.data(), held.keys.data(), held.counts.data(), world, rank, nullptr, nullptr, 0);
    std::vector<int32_t> keys((size_t)n * 3);
    std::vector<uint8_t> action((size_t)n);
    EXPECT(hv_halo_plan_host(dirty.keys.data(), dirty.counts.data(), held.keys.data(), held.counts.data(), world, rank, keys.data(), action.data(), n) == n);
    Plan p;
    for (int64_t i = 0; i < n; ++i) p.keys.push_back({keys[i * 3], keys[i * 3 + 1], keys[i * 3 + 2]});
    p.action = action;
    return p;
}
// sets instead of a sort: a key is shared when some rank lists it dirty and two ranks or more hold it; the lowest holder keeps
static Plan brute_plan(const Lists &dirty, const Lists &held, int world, int rank) {
    std::set<Key> every;
    for (int r = 0; r < world; ++r) every.insert(dirty.by_rank[r].begin(), dirty.by_rank[r].end());
    Plan p;
    for (const Key &k : every) { // (std::set: ascending (x, y, z))
        int holders = 0, keeper = -1;
        for (int r = world - 1; r >= 0; --r)
            if (held.by_rank[r].count(k)) {
                ++holders;
                keeper = r;
            }
        if (holders < 2) continue;
        p.keys.push_back(k);
        p.action.push_back(keeper == rank ? 1 : 2);
    }
    return p;
}

static void check_random_lists() {
    std::mt19937 rng(20240607);
    auto chance = [&](double p) { return std::uniform_real_distribution<double>(0.0, 1.0)(rng) < p; };
    int cases = 0, shared_seen = 0, twice_seen = 0;
    for (int world = 1; world <= 8; ++world)
        for (int round = 0; round < 40; ++round, ++cases) {
            const int n_keys = round % 5 == 0 ? 0 : 1 + (int)(rng() % 40);
            std::vector<Key> pool;
            for (int i = 0; i < n_keys; ++i) pool.push_back({(int32_t)(rng() % 7) - 3, (int32_t)(rng() % 5) - 2, (int32_t)(rng() % 3) - 1});
            const int empty_rank = round % 3 == 0 ? (int)(rng() % (unsigned)world) : -1;
            Lists dirty, held;
            for (int r = 0; r < world; ++r) {
                std::vector<Key> d, h;
                std::set<Key> d_once;
                for (const Key &k : pool) {
                    if (r == empty_rank) break;
                    if (chance(0.3) && d_once.insert(k).second) d.push_back(k); // (the pool may repeat a key: dirty lists never do)
                    if (chance(0.4)) {
                        h.push_back(k);
                        if (chance(0.25)) { // the held-twice form
                            h.push_back(k);
                            ++twice_seen;
                        }
                    }
                }
                std::shuffle(d.begin(), d.end(), rng);
                std::shuffle(h.begin(), h.end(), rng);
                dirty.add_rank(d);
                held.add_rank(h);
            }
            for (int rank = 0; rank < world; ++rank) {
                const Plan got = host_plan(dirty, held, world, rank), want = brute_plan(dirty, held, world, rank);
                EXPECT(got == want);
                shared_seen += (int)got.keys.size();
                // (c) the dirty lists alone: every lister a holder
                EXPECT(host_plan(dirty, dirty, world, rank) == brute_plan(dirty, dirty, world, rank));
            }
        }
    EXPECT(cases == 320 && shared_seen > 1000 && twice_seen > 500);
}

static void check_run_rule() {
    auto e = [](int rank, int held) { return (int32_t)(rank << 1 | held); };
    uint8_t a = 9;
    // dirty on 0, held by 1 twice: one holder, not shared; with rank 2 holding it as well: shared, rank 1 keeps
    const int32_t once[] = {e(0, 0), e(1, 1), e(1, 1)}, both[] = {e(0, 0), e(1, 1), e(1, 1), e(2, 1)};
    EXPECT(!hv_halo_run_rule(once, 3, 1, false, &a) && a == 0);
    EXPECT(hv_halo_run_rule(both, 4, 1, false, &a) && a == 1);
    EXPECT(hv_halo_run_rule(both, 4, 2, false, &a) && a == 2);
    EXPECT(hv_halo_run_rule(both, 4, 0, false, &a) && a == 2); // a rank that does not hold it zeroes too (a no-op there)
    // held by two, dirty nowhere; dirty everywhere, held nowhere
    const int32_t clean[] = {e(0, 1), e(3, 1)}, loose[] = {e(0, 0), e(1, 0), e(2, 0)};
    EXPECT(!hv_halo_run_rule(clean, 2, 0, false, &a) && a == 0);
    EXPECT(!hv_halo_run_rule(loose, 3, 0, false, &a) && a == 0);
    // all_dirty_kept: every dirty key is shared and kept, whoever holds it; a key nobody lists dirty is not
    EXPECT(hv_halo_run_rule(once, 3, 0, true, &a) && a == 1);
    EXPECT(hv_halo_run_rule(loose, 3, 2, true, &a) && a == 1);
    EXPECT(hv_halo_run_rule(both, 4, 2, true, &a) && a == 1);
    EXPECT(!hv_halo_run_rule(clean, 2, 0, true, &a) && a == 0);
    const int32_t lone[] = {e(0, 0)};
    EXPECT(hv_halo_run_rule(lone, 1, 0, true, &a) && a == 1);
    EXPECT(!hv_halo_run_rule(lone, 1, 0, false, &a) && a == 0);
}

// (x, y, z) order, a cap below the number of shared keys, and no lists at all
static void check_order_and_cap() {
    Lists dirty, held;
    dirty.add_rank({{1, 0, -1}, {0, 0, 1}, {-2, 5, 5}});
    dirty.add_rank({});
    held.add_rank({{0, 0, 1}, {-2, 5, 5}, {1, 0, -1}});
    held.add_rank({{1, 0, -1}, {-2, 5, 5}, {0, 0, 1}});
    const Plan p = host_plan(dirty, held, 2, 1);
    EXPECT((p.keys == std::vector<Key>{{-2, 5, 5}, {0, 0, 1}, {1, 0, -1}}) && (p.action == std::vector<uint8_t>{2, 2, 2}));
    int32_t keys[2 * 3 + 1] = {0, 0, 0, 0, 0, 0, 77};
    uint8_t action[3] = {0, 0, 77};
    EXPECT(hv_halo_plan_host(dirty.keys.data(), dirty.counts.data(), held.keys.data(), held.counts.data(), 2, 0, keys, action, 2) == 3);
    EXPECT(keys[0] == -2 && keys[3] == 0 && keys[5] == 1 && keys[6] == 77 && action[0] == 1 && action[1] == 1 && action[2] == 77);
    const int64_t none[3] = {0, 0, 0};
    EXPECT(hv_halo_plan_host(nullptr, none, nullptr, none, 3, 2, nullptr, nullptr, 0) == 0);
}

int main() {
    check_run_rule();
    check_order_and_cap();
    check_random_lists();
    puts("halo_plan_check ok");
    return 0;
}
