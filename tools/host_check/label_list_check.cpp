// Host-side check of the label list of the two map payloads - HvProbVoxel's (object, class) pairs and HvProb2Voxel's two marginal
// maps in one list of inline slots and overflow nodes (hv_semantic.h, compiled into this program as it stands: sem_observe,
// prob_fold, prob2_fold, prob_append_t, prob_find, prob_node_grab, the set_object_id functions and the accessors) - without a GPU.
// Meant for the address and undefined-behaviour sanitizers:
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Iinclude -Ipyslam_amd/csrc \
//         tools/host_check/label_list_check.cpp -o /tmp/label_list_check && /tmp/label_list_check
// Seeded observation streams go into ONE voxel and a small node array, and into a std::map model written here after the reference's
// rules (voxel_data_semantic.h:311-417, 562-648; voxel_data_semantic2.h:311-452, 579-691).  Compared after every observation: the
// number of entries, the entries as a set (log-probabilities by their bits), the most likely ids, the log-normalisation and the
// confidence (by their bits: the model adds in the map's key order with the header's exp / log) and `confidence >= 0`.
// Cases: 0, 1, 6, 7, 16, 17 and 254 + 1 entries (the inline and node boundaries and the limit), a pool of two nodes that runs out,
// set_object_id and then growth into the chain that was left behind, a reset that keeps `next` (sem_reset's rule, restated: that
// function belongs to the kernels' unit), a list holding a NaN and one holding -inf.
// It prints "label_list_check ok" and exits 0, or names the first expectation that failed.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <random>
#include <set>
#include <tuple>
#include <vector>

#include "hv_semantic.h"

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

void hv_set_error(const char *, ...) {}

static uint32_t bits(float x) {
    uint32_t u;
    memcpy(&u, &x, 4);
    return u;
}
static bool same(float a, float b) { return bits(a) == bits(b) || (a != a && b != b); }

// one voxel, its node pool and the counters the pool counts in
template <typename VOX> struct Rig {
    VOX v;
    std::vector<HvProbNode> nodes;
    int32_t counters[HV_CNT_COUNT] = {};
    HvTable table;
    HvSemParams G;
    int32_t count = 0; // observations so far (the voxel's `count` is the fold kernel's to keep)
    explicit Rig(int n_nodes) : nodes((size_t)n_nodes) {
        memset(&v, 0, sizeof(v));
        memset(&table, 0, sizeof(table));
        memset(&G, 0, sizeof(G));
        for (HvProbNode &nd : nodes) memset(&nd, 0xff, sizeof(nd)); // (a node's `next` must be cleared by whoever hands it out)
        table.prob_nodes = nodes.empty() ? nullptr : nodes.data();
        table.prob_node_cap = n_nodes;
        table.counters = counters;
        G.depth_threshold = 1.0f;
        G.depth_decay_rate = 0.5f;
    }
    HvNodePool pool() const { return hv_node_pool(table); }
    const HvProbNode *nd() const { return (const HvProbNode *)table.prob_nodes; }
    int used() const { return counters[HV_CNT_PROB_NODES]; }
    int observe(int32_t obj, int32_t cls, bool with_depth, float depth) {
        const int lost = sem_observe(&v, pool(), count == 0, obj, cls, with_depth, depth, G);
        v.count = ++count;
        return lost;
    }
    void reset() { // sem_reset: the record is zeroed, the chain stays
        const uint32_t chain = v.next;
        memset(&v, 0, sizeof(v));
        v.next = chain;
        count = 0;
    }
    std::set<std::tuple<int32_t, int32_t, uint32_t>> entries() const {
        std::set<std::tuple<int32_t, int32_t, uint32_t>> s;
        for (int i = 0; i < prob_nlab(v.meta); ++i) {
            const HvProbPair p = prob_get(&v, nd(), i);
            EXPECT(s.insert({p.obj, p.cls, bits(p.logp)}).second);
        }
        return s;
    }
    // entries this voxel can hold with the nodes it has and the pool can still give
    int room() const {
        int chain = 0;
        for (uint32_t n = v.next; n != 0u; n = nodes[n - 1].next) ++chain;
        const int r = HV_PROB_K + HV_PROB_NK * (chain + ((int)nodes.size() - used()));
        return r < HV_PROB_MAX ? r : HV_PROB_MAX;
    }
};

// ---- VoxelSemanticDataProbabilistic: one map of pairs, the most likely pair cached ----
struct PairModel {
    using Key = std::pair<int32_t, int32_t>;
    std::map<Key, float> m;
    bool cached = false;
    Key best{-1, -1};
    void recompute() { // update_cache(): the first maximum in key order
        cached = false;
        for (const auto &e : m)
            if (!cached || e.second > m[best]) {
                best = e.first;
                cached = true;
            }
    }
    void observe(Key k, float lp, bool first, bool fits) {
        auto it = m.find(k);
        if (it == m.end()) {
            if (!fits) return;
            const float best_lp = cached ? m[best] : 0.f;
            m[k] = lp;
            if (first || (cached && lp > best_lp)) best = k, cached = true;
            else if (!cached) recompute();
        } else if (first) {
            it->second = lp;
            best = k, cached = true;
        } else {
            const float old = it->second, now = old + lp, best_lp = cached ? m[best] : 0.f;
            it->second = now;
            if (!cached) recompute();
            else if (k == best) { if (now < old) recompute(); }
            else if (now > best_lp) best = k;
        }
    }
    float norm() const {
        float acc = -INFINITY;
        for (const auto &e : m) acc = prob_log_add_exp(acc, e.second);
        return acc;
    }
    float confidence() {
        if (m.empty()) return 0.0f;
        if (!cached) recompute();
        if (best.first == -1 || best.second == -1) return 0.0f;
        return hv_expf_cr(m[best] - norm());
    }
    void set_object_id(int32_t id) { // force_label_distribution
        const int32_t cls = m.empty() ? -1 : (cached ? best.second : (recompute(), best.second));
        m.clear();
        cached = false;
        if (id >= 0 && cls >= 0) m[{id, cls}] = 0.0f, best = {id, cls}, cached = true;
    }
};
static void compare(Rig<HvProbVoxel> &r, PairModel &M, bool has_nan) {
    const HvProbNode *nd = r.nd();
    EXPECT(prob_nlab(r.v.meta) == (int)M.m.size());
    std::set<std::tuple<int32_t, int32_t, uint32_t>> want;
    for (const auto &e : M.m) want.insert({e.first.first, e.first.second, bits(e.second)});
    EXPECT(r.entries() == want);
    const float conf = M.confidence(); // (settles the model's cache as the accessors settle theirs: by the argmax)
    EXPECT(sem_object_id(&r.v, nd) == (M.m.empty() ? -1 : M.best.first));
    EXPECT(sem_class_id(&r.v, nd) == (M.m.empty() ? -1 : M.best.second));
    if (!M.m.empty()) EXPECT(same(prob_log_normalization(&r.v, nd, prob_nlab(r.v.meta)), M.norm()));
    EXPECT(same(sem_confidence(&r.v, nd), conf));
    EXPECT(sem_confidence_not_negative(&r.v, nd) == (conf >= 0.0f));
    if (!has_nan && !M.m.empty()) { // the two argmaxes (pointer, register copy) against the map's: larger log-probability, smaller key
        PairModel A = M;
        A.recompute();
        const int n = prob_nlab(r.v.meta);
        const HvProbPair a = prob_get(&r.v, nd, prob_argmax(&r.v, nd, n)), b = prob_get(&r.v, nd, prob_argmax_r<true>(&r.v, nd, n));
        EXPECT(PairModel::Key(a.obj, a.cls) == A.best && PairModel::Key(b.obj, b.cls) == A.best);
    }
}
// n_distinct pairs in a seeded order, every one observed again now and then; -> observations lost
static int run_pairs(Rig<HvProbVoxel> &r, PairModel &M, int n_distinct, uint32_t seed, int id0 = 0) {
    std::mt19937 rng(seed);
    int lost = 0;
    compare(r, M, false);
    for (int k = 0; k < n_distinct; ++k) {
        for (int rep = 0; rep < 1 + (int)(rng() % 2u); ++rep) {
            // a new pair (ids descending and ascending by turns: insertion order is not key order), then an old one
            const int j = rep == 0 ? k : (int)(rng() % (uint32_t)(k + 1));
            const PairModel::Key key{id0 + ((j & 1) ? 1000 - j : j), (j % 7) - 1};
            const bool with_depth = (rng() & 1u) != 0u;
            const float depth = 0.5f + 0.25f * (float)(rng() % 12u); // on both sides of the threshold
            const bool first = r.count == 0, fits = M.m.count(key) != 0 || (int)M.m.size() < r.room();
            const int l = r.observe(key.first, key.second, with_depth, depth);
            EXPECT(l == (fits ? 0 : 1));
            lost += l;
            M.observe(key, prob_observation_log_prob(with_depth, depth, r.G), first, fits);
            compare(r, M, false);
        }
    }
    return lost;
}

// ---- VoxelSemanticDataProbabilistic2: two marginal maps, a most likely id cached per map ----
struct MarginalModel {
    std::map<int32_t, float> m[2];
    bool cached[2] = {false, false};
    int32_t best[2] = {-1, -1};
    struct Best { int32_t id; float lp; bool any; };
    Best most_likely(int w) const {
        if (cached[w]) return {best[w], m[w].at(best[w]), true};
        Best b{-1, -INFINITY, !m[w].empty()};
        for (const auto &e : m[w])
            if (e.second > b.lp) b.id = e.first, b.lp = e.second;
        return b;
    }
    // -> entries lost; room: how many new entries still fit
    int observe(int32_t obj, int32_t cls, float lp, bool first, int room) {
        const float half = lp * 0.5f;
        const int32_t id[2] = {obj, cls};
        int lost = 0;
        bool stored[2];
        for (int w = 0; w < 2; ++w) {
            auto it = m[w].find(id[w]);
            stored[w] = true;
            if (it != m[w].end()) it->second = first ? half : it->second + half;
            else if (room > 0) m[w][id[w]] = half, --room;
            else stored[w] = false, ++lost;
        }
        for (int w = 0; w < 2; ++w) cached[w] = first && stored[w], best[w] = id[w];
        return lost;
    }
    float norm(int w) const {
        if (m[w].empty()) return 0.0f;
        float mx = -INFINITY, sum = 0.0f;
        for (const auto &e : m[w])
            if (e.second > mx) mx = e.second;
        for (const auto &e : m[w]) sum += hv_expf_cr(e.second - mx);
        return mx + hv_logf_cr(sum);
    }
    float confidence() const {
        const Best o = most_likely(0), c = most_likely(1);
        if (o.id == -1 || c.id == -1 || !o.any || !c.any) return 0.0f;
        return hv_expf_cr((o.lp + c.lp) - (norm(0) + norm(1)));
    }
    bool set_object_id(int32_t id, int room) {
        const Best b = most_likely(0);
        const float target = (b.any && b.id != -1 && b.lp != -INFINITY) ? b.lp : 0.0f;
        const bool fits = m[0].count(id) != 0 || room > 0;
        if (fits) m[0][id] = target;
        cached[0] = fits, best[0] = id, cached[1] = false;
        return fits;
    }
    size_t size() const { return m[0].size() + m[1].size(); }
};
static void compare(Rig<HvProb2Voxel> &r, const MarginalModel &M) {
    const HvProbNode *nd = r.nd();
    const int n = prob_nlab(r.v.meta);
    EXPECT(n == (int)M.size());
    std::set<std::tuple<int32_t, int32_t, uint32_t>> want;
    for (int w = 0; w < 2; ++w)
        for (const auto &e : M.m[w]) want.insert({e.first, w, bits(e.second)});
    EXPECT(r.entries() == want);
    EXPECT(sem_object_id(&r.v, nd) == M.most_likely(0).id && sem_class_id(&r.v, nd) == M.most_likely(1).id);
    for (int w = 0; w < 2; ++w) EXPECT(same(prob2_log_normalization(&r.v, nd, n, w), M.norm(w)));
    const float conf = M.confidence();
    EXPECT(same(sem_confidence(&r.v, nd), conf));
    EXPECT(sem_confidence_not_negative(&r.v, nd) == (conf >= 0.0f));
}
// observations until the list holds n_entries or more (or has lost what is missing): a new object with a new class twice, then a new
// object with an old class - the list grows by 2, 2, 1 and crosses every boundary at both parities -, every one followed now and then by
// an observation of ids seen before; -> entries lost
static int run_marginals(Rig<HvProb2Voxel> &r, MarginalModel &M, int n_entries, uint32_t seed, int id0 = 0) {
    std::mt19937 rng(seed);
    int lost = 0;
    compare(r, M);
    for (int k = 0; (int)M.size() + lost < n_entries; ++k) {
        for (int rep = 0; rep < 1 + (int)(rng() % 2u); ++rep) {
            const int j = rep == 0 ? k : (int)(rng() % (uint32_t)(k + 1));
            const int32_t obj = id0 + ((j & 1) ? 500 - j : j), cls = id0 + 100 - (j % 3 == 2 ? j - 1 : j);
            const bool with_depth = (rng() & 1u) != 0u;
            const float depth = 0.5f + 0.25f * (float)(rng() % 12u);
            const bool first = r.count == 0;
            const int room = r.room() - (int)M.size();
            const int l = r.observe(obj, cls, with_depth, depth);
            EXPECT(l == M.observe(obj, cls, prob2_observation_log_prob(with_depth, depth, r.G), first, room));
            lost += l;
            compare(r, M);
        }
    }
    return lost;
}
static int nodes_for(size_t entries) { return entries <= (size_t)HV_PROB_K ? 0 : ((int)entries - HV_PROB_K + HV_PROB_NK - 1) / HV_PROB_NK; }

int main() {
    // the inline and node boundaries and the limit
    for (int n : {0, 1, 6, 7, 16, 17, HV_PROB_MAX + 1}) {
        Rig<HvProbVoxel> r(32);
        PairModel M;
        EXPECT(run_pairs(r, M, n, 100u + (uint32_t)n) == (n > HV_PROB_MAX ? 1 : 0));
        EXPECT(M.m.size() == (size_t)(n < HV_PROB_MAX ? n : HV_PROB_MAX) && r.used() == nodes_for(M.m.size()));
        Rig<HvProb2Voxel> r2(32);
        MarginalModel M2;
        EXPECT(run_marginals(r2, M2, n, 200u + (uint32_t)n) == (n > HV_PROB_MAX ? 1 : 0));
        EXPECT(M2.size() >= (size_t)(n < HV_PROB_MAX ? n : HV_PROB_MAX) && r2.used() == nodes_for(M2.size()));
    }
    { // no pool at all: the inline slots are the list
        Rig<HvProbVoxel> r(0);
        PairModel M;
        EXPECT(run_pairs(r, M, 9, 7u) == 3 && r.used() == 0 && r.v.next == 0u);
    }
    { // a pool of two nodes that runs out: 6 + 20 entries, the counter stays the number of nodes handed out
        Rig<HvProbVoxel> r(2);
        PairModel M;
        EXPECT(run_pairs(r, M, 30, 11u) == 4 && r.used() == 2 && M.m.size() == 26u);
        Rig<HvProb2Voxel> r2(2);
        MarginalModel M2;
        EXPECT(run_marginals(r2, M2, 30, 12u) >= 4 && r2.used() == 2 && M2.size() == 26u);
    }
    { // set_object_id collapses the map; the next one grows into the chain that was left behind.  Then a reset that keeps `next`.
        Rig<HvProbVoxel> r(4);
        PairModel M;
        EXPECT(run_pairs(r, M, 17, 21u) == 0 && r.used() == 2);
        const uint32_t chain = r.v.next;
        sem_set_object_id(&r.v, r.table, 77);
        M.set_object_id(77);
        compare(r, M, false);
        EXPECT(prob_nlab(r.v.meta) <= 1 && r.v.next == chain);
        EXPECT(run_pairs(r, M, 27, 22u, 2000) == 0 && r.used() == 3); // 27 or 28 entries: the two old nodes and one new
        r.reset();
        M = PairModel();
        EXPECT(r.v.next == chain);
        EXPECT(run_pairs(r, M, 36, 23u) == 0 && r.used() == 3 && r.v.next == chain);
        sem_set_object_id(&r.v, r.table, -1); // (no id: the map empties)
        M.set_object_id(-1);
        compare(r, M, false);
    }
    { // the same for the marginal maps: set_object_id adds or moves ONE entry, up to a full list
        Rig<HvProb2Voxel> r(3);
        MarginalModel M;
        EXPECT(run_marginals(r, M, 12, 31u) == 0 && r.used() == 1);
        for (int32_t id : {9000, M.m[0].begin()->first, 9001}) { // new, old, new
            EXPECT(prob2_set_object_id(&r.v, r.pool(), id) == M.set_object_id(id, r.room() - (int)M.size()));
            compare(r, M);
        }
        EXPECT(run_marginals(r, M, 30, 32u, 3000) == 0);
        for (int32_t id = 9100; (int)M.size() < r.room(); ++id) { // one entry at a time up to the last place of the third node
            EXPECT(prob2_set_object_id(&r.v, r.pool(), id) && M.set_object_id(id, 1));
            compare(r, M);
        }
        EXPECT(M.size() == 36u && r.used() == 3);
        EXPECT(!prob2_set_object_id(&r.v, r.pool(), 9002) && !M.set_object_id(9002, 0)); // full: refused, the object cache is dropped
        compare(r, M);
        const uint32_t chain = r.v.next;
        r.reset();
        M = MarginalModel();
        EXPECT(run_marginals(r, M, 30, 33u) == 0 && r.used() == 3 && r.v.next == chain);
    }
    // a list holding a NaN and one holding -inf, inline and in a node
    for (int n : {3, 9})
        for (float bad : {NAN, -INFINITY})
            for (int at : {0, n - 1}) {
                Rig<HvProbVoxel> r(4);
                PairModel M;
                run_pairs(r, M, n, 41u);
                const HvProbPair p = prob_get(&r.v, r.nd(), at);
                prob_set_logp(&r.v, (HvProbNode *)r.table.prob_nodes, at, bad);
                M.m[{p.obj, p.cls}] = bad;
                compare(r, M, bad != bad);
                EXPECT(!prob_all_finite(&r.v, r.nd()));
                Rig<HvProb2Voxel> r2(4);
                MarginalModel M2;
                run_marginals(r2, M2, n, 42u);
                const HvProbPair q = prob_get(&r2.v, r2.nd(), at);
                prob_set_logp(&r2.v, (HvProbNode *)r2.table.prob_nodes, at, bad);
                M2.m[q.cls][q.obj] = bad;
                M2.cached[0] = M2.cached[1] = false; // (the caches of the voxel were dropped by its last update as well)
                compare(r2, M2);
            }
    { // a NaN and an infinite depth through the observation itself
        Rig<HvProb2Voxel> r(4);
        MarginalModel M;
        run_marginals(r, M, 5, 51u);
        for (float depth : {INFINITY, NAN}) {
            EXPECT(r.observe(3, 4, true, depth) == M.observe(3, 4, prob2_observation_log_prob(true, depth, r.G), false, r.room() - (int)M.size()));
            compare(r, M);
        }
    }
    printf("label_list_check ok\n");
    return 0;
}
