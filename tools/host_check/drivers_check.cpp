// Host-side check of the two integrate drivers the grids share - hv_bins_claim / hv_bins_folded / hv_bins_fold_grid (hv_bins.h) and
// hv_sort_path (hv_sort_path.h) - without a GPU: the HIP runtime calls they make, the rocPRIM sort and the library functions they call
// (hv_claims_fit, hv_ensure_buffer ...) are stand-ins defined here that record what was asked of them, the "launches" are lambdas.
// Meant for the address and undefined-behaviour sanitizers:
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Itools/host_check/stub -Iinclude \
//         -Ipyslam_amd/csrc tools/host_check/drivers_check.cpp -o /tmp/drivers_check -pthread && /tmp/drivers_check
// It prints "drivers_check ok" and exits 0, or names the first expectation that failed.
#include <cstdarg>
#include <cstdlib>
#include <string>
#include <thread>
#include <vector>

#include "hv_common.h"
#include "hv_bins.h"
#include "hv_sort_path.h"

namespace host_check {
int size_queries = 0;
std::vector<SortCall> sorts;
std::vector<std::string> trace; // what ran, in order
void note(const char *what) { trace.push_back(what); }
std::vector<int> fit_answers; // what hv_claims_fit returns, call by call (then HV_OK)
size_t fit_calls = 0;
hipError_t launch_error = hipSuccess; // what the next hipGetLastError reports
int mallocs = 0, frees = 0, memsets = 0, occupancy_asks = 0;
bool fail_malloc = false;
} // namespace host_check
using namespace host_check;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

// ---- stand-ins: HIP runtime ----
extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    if (fail_malloc) return hipErrorOutOfMemory;
    ++mallocs;
    *p = malloc(bytes ? bytes : 1);
    return *p ? hipSuccess : hipErrorOutOfMemory;
}
hipError_t hipFree(void *p) {
    ++frees;
    free(p);
    return hipSuccess;
}
hipError_t hipMemsetAsync(void *p, int value, size_t bytes, hipStream_t) {
    ++memsets;
    memset(p, value, bytes); // (the sanitizer checks that the driver clears what it allocated, no more)
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) { return hipSuccess; }
hipError_t hipGetLastError(void) {
    const hipError_t e = launch_error;
    launch_error = hipSuccess;
    return e;
}
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }
hipError_t hipGetDevicePropertiesR0600(hipDeviceProp_tR0600 *prop, int) {
    memset(prop, 0, sizeof(*prop));
    prop->multiProcessorCount = 256;
    return hipSuccess;
}
hipError_t hipOccupancyMaxActiveBlocksPerMultiprocessor(int *n, const void *, int, size_t dyn_lds) {
    ++occupancy_asks;
    *n = dyn_lds > 32768 ? 2 : 8;
    return hipSuccess;
}
}

// ---- stand-ins: the library ----
void hv_set_error(const char *, ...) {}
int hv_ensure_buffer(hv_volume *, void **buf, size_t *cur, size_t want) {
    if (*cur >= want && *buf) return HV_OK;
    if (fail_malloc) return HV_ERR_DEVICE;
    free(*buf);
    *buf = malloc(want);
    *cur = want;
    note("ensure");
    return HV_OK;
}
int hv_claims_fit(hv_volume *v) {
    const int rc = fit_calls < fit_answers.size() ? fit_answers[fit_calls] : HV_OK;
    ++fit_calls;
    if (rc == HV_RETRY_CLAIM && v->table_capacity < (1u << 12)) v->table_capacity *= 2; // the pool grew, the table moved
    return rc;
}
int32_t hv_next_status_seq(hv_volume *v) { return ++v->status_seq_issued; }
void hv_launch_publish_status(hv_volume *) { note("publish"); }

static void fake_kernel_a() {}
static void fake_kernel_b() {}

static hv_volume *make_volume() {
    hv_volume *v = new hv_volume();
    v->cfg.max_points = 1 << 12;
    v->cfg.max_blocks = 1 << 6;
    v->table_capacity = 1 << 7;
    v->local_bits = 9;
    v->table.counters = (int32_t *)calloc(64, sizeof(int32_t));
    return v;
}
static void free_volume(hv_volume *v) {
    for (void *p : {(void *)v->bins.cnt, (void *)v->bins.inl, (void *)v->bins.touched, (void *)v->bins.len, (void *)v->bins.pg_keys, (void *)v->bins.pg_data,
                    (void *)v->sort_tmp, (void *)v->table.counters})
        free(p);
    delete v;
}
static void reset_trace() {
    trace.clear();
    sorts.clear();
    size_queries = 0;
    fit_answers.clear();
    fit_calls = 0;
}

static void check_bins() {
    hv_volume *v = make_volume();
    HvBins B{};
    int32_t seq = 0;
    int launches = 0;
    std::vector<uint32_t> epochs;
    auto bin = [&](const HvBins &b) {
        ++launches;
        epochs.push_back(b.epoch);
        EXPECT(b.cnt != nullptr && b.inl != nullptr && b.touched != nullptr && b.len != nullptr && b.pg_keys != nullptr);
        EXPECT(v->bins_clean);
        b.cnt[v->table_capacity - 1] = 7; // (a bin pass leaves counts behind; the last slot is inside the array)
    };
    // unchecked: one pass, parity flips, a sequence number
    EXPECT(hv_bins_claim(v, 20, false, bin, &B, &seq) == HV_OK);
    EXPECT(launches == 1 && fit_calls == 0 && seq == 1 && v->bins.parity == 1 && B.parity == 0 && B.idx_bits == 20 && B.epoch == 1);
    EXPECT(hv_bins_folded(v) == HV_OK && v->frame_counter == 1 && v->bins_clean);
    // the bins are kept: no allocation in the second call
    const int mallocs_before = mallocs;
    EXPECT(hv_bins_claim(v, 20, false, bin, &B, &seq) == HV_OK && mallocs == mallocs_before && B.parity == 1 && B.epoch == 2 && seq == 2);
    EXPECT(hv_bins_folded(v) == HV_OK);
    // checked, two passes that did not fit: three launches, each from clean arrays made for the table as it is then
    reset_trace();
    launches = 0;
    epochs.clear();
    fit_answers = {HV_RETRY_CLAIM, HV_RETRY_CLAIM};
    const uint64_t cap_before = v->table_capacity;
    EXPECT(hv_bins_claim(v, 20, true, bin, &B, &seq) == HV_OK);
    EXPECT(launches == 3 && fit_calls == 3 && v->table_capacity == 4 * cap_before && v->bins_cap == v->table_capacity && v->bins_clean);
    EXPECT(epochs[0] < epochs[1] && epochs[1] < epochs[2] && B.parity == 0 && v->bins.parity == 1);
    for (uint64_t s = 0; s + 1 < v->table_capacity; ++s) EXPECT(B.cnt[s] == 0);
    EXPECT(hv_bins_folded(v) == HV_OK);
    // checked, never fits: gives up with a capacity error and leaves the bins marked unclean
    reset_trace();
    launches = 0;
    fit_answers.assign(32, HV_RETRY_CLAIM);
    EXPECT(hv_bins_claim(v, 20, true, bin, &B, &seq) == HV_ERR_CAPACITY && launches == 9 && !v->bins_clean);
    // another error from the claims is passed on
    reset_trace();
    fit_answers = {HV_ERR_DEVICE};
    EXPECT(hv_bins_claim(v, 20, true, bin, &B, &seq) == HV_ERR_DEVICE && !v->bins_clean);
    // a launch error after the bin pass: the counts it left are not taken for clean ones by the next call
    reset_trace();
    EXPECT(hv_bins_claim(v, 20, false, bin, &B, &seq) == HV_OK && v->bins_clean);
    launch_error = hipErrorLaunchFailure;
    const int32_t frames = v->frame_counter;
    EXPECT(hv_bins_folded(v) == HV_ERR_DEVICE && !v->bins_clean && v->frame_counter == frames);
    const int memsets_before = memsets;
    EXPECT(hv_bins_claim(v, 20, false, bin, &B, &seq) == HV_OK && memsets > memsets_before && B.parity == 0);
    // an allocation that fails does so BEFORE the bin pass
    hv_volume *w = make_volume();
    launches = 0;
    fail_malloc = true;
    EXPECT(hv_bins_claim(w, 20, false, bin, &B, &seq) == HV_ERR_DEVICE && launches == 0);
    fail_malloc = false;
    free_volume(w);
    free_volume(v);
}

static void check_fold_grid() {
    hv_volume *v = make_volume();
    occupancy_asks = 0;
    EXPECT(hv_bins_fold_grid(v, fake_kernel_a, 0) == 8u * 256u && occupancy_asks == 1);
    EXPECT(hv_bins_fold_grid(v, fake_kernel_a, 0) == 8u * 256u && occupancy_asks == 1);     // cached
    EXPECT(hv_bins_fold_grid(v, fake_kernel_a, 40000) == 2u * 256u && occupancy_asks == 2); // another LDS size: asked again
    EXPECT(hv_bins_fold_grid(v, fake_kernel_b, 0) == 8u * 256u && occupancy_asks == 3);     // another kernel
    v->device = 1;
    EXPECT(hv_bins_fold_grid(v, fake_kernel_a, 0) == 8u * 256u && occupancy_asks == 4);     // another device
    // several threads, each with a volume of its own
    std::vector<std::thread> threads;
    for (int t = 0; t < 8; ++t)
        threads.emplace_back([t]() {
            hv_volume *u = make_volume();
            u->device = 2 + t % 3;
            for (int k = 0; k < 200; ++k) EXPECT(hv_bins_fold_grid(u, k % 2 ? fake_kernel_a : fake_kernel_b, (size_t)(k % 5) * 1024) == 8u * 256u);
            free_volume(u);
        });
    for (auto &t : threads) t.join();
    EXPECT(occupancy_asks == 4 + 3 * 2 * 5);
    free_volume(v);
}

static void check_sort_path() {
    hv_volume *v = make_volume();
    auto keys = []() { note("keys"); };
    auto reduce = []() { note("reduce"); };
    // unchecked: size query, temporary, keys, sort, reduce, status - in that order
    reset_trace();
    EXPECT(hv_sort_path(v, 1000, false, keys, reduce) == HV_OK);
    EXPECT((trace == std::vector<std::string>{"ensure", "keys", "sort", "reduce", "publish"}));
    EXPECT(size_queries == 1 && sorts.size() == 1 && sorts[0].n == 1000 && sorts[0].end_bit == (unsigned)hv_sort_bits(v));
    EXPECT(sorts[0].bytes == v->sort_tmp_bytes && v->frame_counter == 1);
    EXPECT(hv_sort_bits(v) == 7 + 9 + 1);
    // checked, one pass that did not fit: the table doubled, the key is a bit wider, the temporary follows before the keys run again
    reset_trace();
    fit_answers = {HV_RETRY_CLAIM};
    EXPECT(hv_sort_path(v, 1000, true, keys, reduce) == HV_OK);
    EXPECT((trace == std::vector<std::string>{"keys", "ensure", "keys", "sort", "reduce", "publish"}));
    EXPECT(size_queries == 2 && sorts[0].end_bit == 8 + 9 + 1);
    // never fits: nothing is sorted or reduced
    reset_trace();
    fit_answers.assign(32, HV_RETRY_CLAIM);
    EXPECT(hv_sort_path(v, 10, true, keys, reduce) == HV_ERR_CAPACITY && sorts.empty());
    for (const std::string &s : trace) EXPECT(s != "reduce" && s != "publish");
    EXPECT(hv_sort_bits(v) <= 32);
    // a launch error is reported, the frame is not counted
    reset_trace();
    const int32_t frames = v->frame_counter;
    launch_error = hipErrorLaunchFailure;
    v->table_capacity = 1 << 7;
    EXPECT(hv_sort_path(v, 10, false, keys, reduce) == HV_ERR_DEVICE && v->frame_counter == frames);
    free_volume(v);
}

int main() {
    check_bins();
    check_fold_grid();
    check_sort_path();
    puts("drivers_check ok");
    return 0;
}
