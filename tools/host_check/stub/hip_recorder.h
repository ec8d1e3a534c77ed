// Stand-ins for the HIP runtime calls of the staging layer (hv_stage.hip) that record what was asked of them: "device" memory is
// malloc memory, a copy is a memcpy (so the sanitizers see every byte that moves), events and streams only count.  Include it in
// exactly one translation unit, after <hip/hip_runtime.h>.
#pragma once
#include <cstdlib>
#include <cstring>
#include <set>
#include <vector>

namespace hip_recorder {
struct Copy {
    hipMemcpyKind kind;
    size_t bytes;
    const void *dst, *src;
};
struct Alloc {
    void *p;
    size_t bytes;
};
std::vector<Copy> copies;
std::vector<Alloc> allocs; // live allocations
int mallocs = 0, frees = 0, event_records = 0, event_syncs = 0, stream_syncs = 0;
int copies_at_last_malloc = -1; // how many copies had been queued when the last allocation was made
bool fail_malloc = false;
std::set<const void *> page_locked; // sources hipPointerGetAttributes reports as host memory of the runtime's
void reset() {
    copies.clear();
    mallocs = frees = event_records = event_syncs = stream_syncs = 0;
    copies_at_last_malloc = -1;
}
// the live allocation that holds [p, p + bytes), or null
const Alloc *find(const void *p, size_t bytes) {
    for (const Alloc &a : allocs)
        if ((const char *)p >= (const char *)a.p && (const char *)p + bytes <= (const char *)a.p + a.bytes) return &a;
    return nullptr;
}
} // namespace hip_recorder

extern "C" {
hipError_t hipMalloc(void **p, size_t bytes) {
    using namespace hip_recorder;
    if (fail_malloc) return hipErrorOutOfMemory;
    ++mallocs;
    copies_at_last_malloc = (int)copies.size();
    *p = malloc(bytes ? bytes : 1);
    allocs.push_back({*p, bytes});
    return hipSuccess;
}
hipError_t hipFree(void *p) {
    using namespace hip_recorder;
    ++frees;
    for (size_t i = 0; i < allocs.size(); ++i)
        if (allocs[i].p == p) {
            allocs.erase(allocs.begin() + (long)i);
            break;
        }
    free(p);
    return hipSuccess;
}
hipError_t hipMemcpyAsync(void *dst, const void *src, size_t bytes, hipMemcpyKind kind, hipStream_t) {
    hip_recorder::copies.push_back({kind, bytes, dst, src});
    memcpy(dst, src, bytes);
    return hipSuccess;
}
hipError_t hipPointerGetAttributes(hipPointerAttribute_t *attr, const void *p) {
    if (hip_recorder::page_locked.count(p) == 0) return hipErrorInvalidValue;
    memset(attr, 0, sizeof(*attr));
    attr->type = hipMemoryTypeHost;
    return hipSuccess;
}
hipError_t hipEventCreateWithFlags(hipEvent_t *e, unsigned) {
    static int one_event;
    *e = (hipEvent_t)&one_event;
    return hipSuccess;
}
hipError_t hipEventRecord(hipEvent_t, hipStream_t) {
    ++hip_recorder::event_records;
    return hipSuccess;
}
hipError_t hipEventSynchronize(hipEvent_t) {
    ++hip_recorder::event_syncs;
    return hipSuccess;
}
hipError_t hipStreamSynchronize(hipStream_t) {
    ++hip_recorder::stream_syncs;
    return hipSuccess;
}
hipError_t hipGetLastError(void) { return hipSuccess; }
const char *hipGetErrorString(hipError_t) { return "stand-in error"; }
}
