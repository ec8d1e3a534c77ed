// Host-side check of the staging layer - HvStage, hv_h2d_lazy / hv_h2d_fence and hv_ensure_buffer (hv_stage.hip, compiled into this
// program as it stands) - without a GPU: the HIP runtime calls it makes are the recording stand-ins of stub/hip_recorder.h.
// Meant for the address and undefined-behaviour sanitizers:
//   hipcc -x hip --offload-host-only -std=c++17 -O1 -g -Xarch_host -fsanitize=address,undefined -Itools/host_check/stub -Iinclude \
//         -Ipyslam_amd/csrc tools/host_check/staging_check.cpp -o /tmp/staging_check -pthread && /tmp/staging_check
// It prints "staging_check ok" and exits 0, or names the first expectation that failed.
#include <cstdarg>
#include <cstdint>
#include <cstdio>
#include <numeric>

#include "hv_common.h"
#include "hip_recorder.h"
#include "hv_stage.hip"

using namespace hip_recorder;

#define EXPECT(cond)                                                                   \
    do {                                                                               \
        if (!(cond)) {                                                                 \
            fprintf(stderr, "%s:%d: expectation failed: %s\n", __FILE__, __LINE__, #cond); \
            exit(1);                                                                   \
        }                                                                              \
    } while (0)

// ---- stand-ins: the library ----
void hv_set_error(const char *, ...) {}
static std::set<const void *> registered; // sources inside a range of hv_host_register
bool hv_host_is_registered(const void *p, size_t) { return registered.count(p) != 0; }

static int count_copies(hipMemcpyKind kind) {
    int n = 0;
    for (const Copy &c : copies) n += c.kind == kind;
    return n;
}
static std::vector<char> pattern(size_t bytes, int seed) {
    std::vector<char> a(bytes);
    for (size_t i = 0; i < bytes; ++i) a[i] = (char)(i * 7 + seed);
    return a;
}

// (a) HV_DEVICE: pointers pass through, no copy, no allocation unless a head was declared, finish without stats does not synchronise
static void check_device() {
    hv_volume *v = new hv_volume();
    char a[100], b[50];
    reset();
    {
        HvStage st(v, HV_DEVICE);
        const int ia = st.in(a, sizeof(a)), ib = st.out(b, sizeof(b)), in = st.in(nullptr, 64), iz = st.out(b, 0);
        EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK);
        EXPECT(st.dev<char>(ia) == a && st.dev<char>(ib) == b && st.dev<char>(in) == nullptr && st.dev<char>(iz) == nullptr);
        EXPECT(st.head_dev == nullptr && mallocs == 0 && copies.empty() && v->stage == nullptr);
        EXPECT(st.finish() == HV_OK && copies.empty() && stream_syncs == 0 && event_records == 0);
    }
    {
        HvStage st(v, HV_DEVICE);
        st.head(40);
        const int ia = st.in(a, sizeof(a));
        EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK);
        EXPECT(st.dev<char>(ia) == a && mallocs == 1 && st.head_dev == v->stage && find(st.head_dev, 40) != nullptr && copies.empty());
        // the stats of a device call: the head bytes asked for, one synchronisation
        memset(st.head_dev, 0x5A, 40);
        char h[40];
        EXPECT(st.finish(h, sizeof(h)) == HV_OK && copies.size() == 1 && copies[0].kind == hipMemcpyDeviceToHost && copies[0].bytes == 40);
        EXPECT(copies[0].src == st.head_dev && h[0] == 0x5A && h[39] == 0x5A && stream_syncs == 1);
    }
    {
        // an argument that is host memory whatever the call's loc (a key list) is staged in a device call too
        HvStage st(v, HV_DEVICE);
        const std::vector<char> keys = pattern(36, 3);
        const int ik = st.in(keys.data(), keys.size(), HV_HOST), ia = st.in(a, sizeof(a));
        reset();
        EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK);
        EXPECT(st.dev<char>(ia) == a && find(st.dev<char>(ik), 36) != nullptr && memcmp(st.dev<char>(ik), keys.data(), 36) == 0);
        EXPECT(copies.size() == 1 && copies[0].kind == hipMemcpyHostToDevice && copies[0].bytes == 36);
    }
    (void)hipFree(v->stage);
    delete v;
}

// (b) (c) (e) HV_HOST with sizes that are no multiples of 256: the layout, the one growth before any copy, the copies back
static void check_host_layout() {
    hv_volume *v = new hv_volume();
    const size_t sizes[5] = {8601, 11468, 1, 0, 4000};
    std::vector<char> in0 = pattern(sizes[0], 1), in1 = pattern(sizes[1], 2), in2 = pattern(sizes[2], 3), in3 = pattern(16, 4);
    std::vector<char> out0(sizes[1]), out1(sizes[4]), out_absent(8);
    // a buffer that is too small already: it has to go, once
    EXPECT(hv_ensure_buffer(v, &v->stage, &v->stage_bytes, 100) == HV_OK);
    reset();
    HvStage st(v, HV_HOST);
    st.head(300);
    const int i0 = st.in(in0.data(), sizes[0]), i1 = st.in(in1.data(), sizes[1]), i2 = st.in(in2.data(), sizes[2]), i3 = st.in(in3.data(), sizes[3]),
              i4 = st.in(nullptr, 512);
    const int o0 = st.out(out0.data(), sizes[1]), o1 = st.out(out1.data(), sizes[4], 40), o2 = st.out(nullptr, 8);
    EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK);
    EXPECT(mallocs == 1 && frees == 1 && copies_at_last_malloc == 0); // grown exactly once, before any copy was queued
    const Alloc *buf = find(v->stage, 1);
    EXPECT(buf != nullptr && st.head_dev == v->stage);
    // absent arguments: null, and no copy in either direction
    EXPECT(st.dev<char>(i3) == nullptr && st.dev<char>(i4) == nullptr && st.dev<char>(o2) == nullptr);
    // present ones: 256-byte aligned from the buffer's start, inside it, behind the head, disjoint
    const int present[5] = {i0, i1, i2, o0, o1};
    const size_t bytes[5] = {sizes[0], sizes[1], sizes[2], sizes[1], sizes[4]};
    for (int a = 0; a < 5; ++a) {
        const char *p = st.dev<char>(present[a]);
        EXPECT(p != nullptr && find(p, bytes[a]) == buf);
        const size_t off = (size_t)(p - (const char *)v->stage);
        EXPECT(off % 256 == 0 && off >= 300);
        for (int b = 0; b < a; ++b) {
            const char *q = st.dev<char>(present[b]);
            EXPECT(p + bytes[a] <= q || q + bytes[b] <= p);
        }
    }
    // the inputs arrived, exactly their bytes each; pageable sources: no fence
    EXPECT(copies.size() == 3 && count_copies(hipMemcpyHostToDevice) == 3);
    EXPECT(copies[0].bytes == sizes[0] && copies[1].bytes == sizes[1] && copies[2].bytes == sizes[2]);
    EXPECT(memcmp(st.dev<char>(i0), in0.data(), sizes[0]) == 0 && memcmp(st.dev<char>(i1), in1.data(), sizes[1]) == 0 && *st.dev<char>(i2) == in2[0]);
    EXPECT(event_records == 0 && event_syncs == 0 && stream_syncs == 1); // (the one synchronisation: the old buffer was drained before it was freed)
    // the "kernel"
    memset(st.head_dev, 0x11, 300);
    memset(st.dev<char>(o0), 0x22, sizes[1]);
    memset(st.dev<char>(o1), 0x33, sizes[4]);
    // finish: the first output whole, 7 rows of 40 bytes of the second, 24 bytes of the head, one synchronisation
    reset();
    st.rows(7);
    char h[24];
    EXPECT(st.finish(h, sizeof(h)) == HV_OK);
    EXPECT(copies.size() == 3 && count_copies(hipMemcpyDeviceToHost) == 3 && stream_syncs == 1 && mallocs == 0);
    EXPECT(copies[0].dst == out0.data() && copies[0].bytes == sizes[1] && copies[1].dst == out1.data() && copies[1].bytes == 7 * 40);
    EXPECT(copies[2].dst == h && copies[2].bytes == 24 && copies[2].src == st.head_dev && h[23] == 0x11);
    EXPECT(out0[0] == 0x22 && out0[sizes[1] - 1] == 0x22 && out1[279] == 0x33 && out1[280] == 0 && out_absent[0] == 0);
    // the same call again: the buffer is large enough, nothing is allocated
    reset();
    HvStage again(v, HV_HOST);
    again.head(300);
    (void)again.in(in0.data(), sizes[0]);
    (void)again.out(out0.data(), sizes[1]);
    EXPECT(again.commit(&v->stage, &v->stage_bytes) == HV_OK && mallocs == 0 && frees == 0);
    // more rows than declared: never more than the declared bytes
    again.rows(1 << 20);
    reset();
    EXPECT(again.finish() == HV_OK && copies.size() == 1 && copies[0].bytes == sizes[1] && stream_syncs == 1);
    // nothing to copy back: nothing waited for
    HvStage none(v, HV_HOST);
    (void)none.in(in2.data(), 1);
    EXPECT(none.commit(&v->stage, &v->stage_bytes) == HV_OK);
    reset();
    EXPECT(none.finish() == HV_OK && copies.empty() && stream_syncs == 0);
    (void)hipFree(v->stage);
    delete v;
}

// (d) three page-locked inputs: one event record + synchronise behind all of them; pageable inputs: none
static void check_fence() {
    hv_volume *v = new hv_volume();
    std::vector<char> a = pattern(700, 1), b = pattern(900, 2), c = pattern(33, 3);
    for (int mode = 0; mode < 3; ++mode) { // 0: pageable, 1: page-locked by the runtime, 2: registered with the library
        page_locked.clear();
        registered.clear();
        if (mode == 1) page_locked = {a.data(), b.data(), c.data()};
        if (mode == 2) registered = {a.data(), b.data(), c.data()};
        reset();
        HvStage st(v, HV_HOST);
        (void)st.in(a.data(), a.size());
        (void)st.in(b.data(), b.size());
        (void)st.in(c.data(), c.size());
        EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK && count_copies(hipMemcpyHostToDevice) == 3);
        EXPECT(event_records == (mode ? 1 : 0) && event_syncs == (mode ? 1 : 0) && stream_syncs == 0);
    }
    // one page-locked source among pageable ones is enough
    page_locked = {b.data()};
    registered.clear();
    reset();
    HvStage st(v, HV_HOST);
    (void)st.in(a.data(), a.size());
    (void)st.in(b.data(), b.size());
    EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_OK && event_records == 1 && event_syncs == 1);
    page_locked.clear();
    (void)hipFree(v->stage);
    delete v;
}

// (f) a failed hipMalloc: the error comes back with nothing queued; more arguments than the helper holds are refused the same way
static void check_errors() {
    hv_volume *v = new hv_volume();
    std::vector<char> a = pattern(5000, 1), o(5000);
    reset();
    fail_malloc = true;
    HvStage st(v, HV_HOST);
    (void)st.in(a.data(), a.size());
    (void)st.out(o.data(), o.size());
    EXPECT(st.commit(&v->stage, &v->stage_bytes) == HV_ERR_DEVICE && copies.empty() && event_records == 0 && v->stage == nullptr);
    fail_malloc = false;
    HvStage many(v, HV_HOST);
    for (int i = 0; i < HvStage::MAX_PIECES + 1; ++i) (void)many.in(a.data(), 8);
    reset();
    EXPECT(many.commit(&v->stage, &v->stage_bytes) == HV_ERR_INVALID && copies.empty() && mallocs == 0);
    delete v;
}

// the frame pair every integrate call stages: one buffer, one growth, colour optional
static void check_frame() {
    hv_volume *v = new hv_volume();
    const size_t npx = 61 * 47;
    std::vector<char> depth = pattern(npx * 2, 1), rgb = pattern(npx * 3, 2);
    const void *d_depth = nullptr;
    const uint8_t *d_rgb = nullptr;
    reset();
    EXPECT(hv_stage_frame(v, depth.data(), HV_DEPTH_U16, (const uint8_t *)rgb.data(), npx, HV_HOST, &d_depth, &d_rgb) == HV_OK);
    EXPECT(mallocs == 1 && copies.size() == 2 && copies[0].bytes == npx * 2 && copies[1].bytes == npx * 3);
    EXPECT(memcmp(d_depth, depth.data(), npx * 2) == 0 && memcmp(d_rgb, rgb.data(), npx * 3) == 0);
    EXPECT(hv_stage_frame(v, depth.data(), HV_DEPTH_U16, nullptr, npx, HV_DEVICE, &d_depth, &d_rgb) == HV_OK && d_depth == depth.data() && d_rgb == nullptr);
    (void)hipFree(v->stage);
    delete v;
}

int main() {
    check_device();
    check_host_layout();
    check_fence();
    check_errors();
    check_frame();
    EXPECT(allocs.empty());
    puts("staging_check ok");
    return 0;
}
