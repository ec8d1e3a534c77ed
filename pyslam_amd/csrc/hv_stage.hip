// libpyslam_hipvol.so — the layer between the C ABI's `loc` argument and the kernels: HvStage (hv_common.h) and the host -> device
// copies of caller arrays.  Host code only (tools/host_check/staging_check.cpp compiles this file against stand-ins of the runtime).
#include <algorithm>

#include "hv_common.h"

// A buffer of the volume that only grows: freed (after the stream has drained) and reallocated with headroom when `want` exceeds it.
int hv_ensure_buffer(hv_volume *v, void **buf, size_t *cur, size_t want) {
    if (*cur >= want && *buf != nullptr) return HV_OK;
    if (*buf) {
        HV_HIP(hipStreamSynchronize(v->stream));
        HV_HIP(hipFree(*buf));
        *buf = nullptr;
        *cur = 0;
    }
    size_t bytes = want < 4096 ? 4096 : want + want / 4;
    HV_HIP(hipMalloc(buf, bytes));
    *cur = bytes;
    return HV_OK;
}

// Host -> device copy of a caller's array on the volume's stream.  The C ABI borrows HV_HOST arrays "for the duration of the call":
// a pageable source is read by the runtime before hipMemcpyAsync returns, but a PAGE-LOCKED source (the front's shared-memory ring
// after hv_host_register, a torch pinned tensor, hipHostMalloc memory) is read by the DMA engine later, when the stream gets there -
// the caller may have refilled the memory by then (a ring slot released while its copy was still queued).  So the
// host waits for the copy when the source is page-locked; the kernels behind it stay asynchronous.
static bool hv_host_is_pinned(const void *p, size_t bytes) {
    if (hv_host_is_registered(p, bytes)) return true;
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, p) != hipSuccess) {
        (void)hipGetLastError(); // plain malloc / numpy memory: "invalid value", not an error of ours
        return false;
    }
    return attr.type == hipMemoryTypeHost;
}

int hv_h2d_lazy(hv_volume *v, void *dst, const void *src, size_t bytes, bool *pending) {
    if (bytes == 0) return HV_OK;
    HV_HIP(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, v->stream));
    if (hv_host_is_pinned(src, bytes)) *pending = true;
    return HV_OK;
}

// (an event right behind the copies, not the whole stream: a caller whose keyframes sit in page-locked memory would otherwise wait
// for every kernel queued before this call as well - ADVICE r05)
int hv_h2d_fence(hv_volume *v, bool pending) {
    if (!pending) return HV_OK;
    if (v->ev_h2d == nullptr) HV_HIP(hipEventCreateWithFlags(&v->ev_h2d, hipEventDisableTiming));
    HV_HIP(hipEventRecord(v->ev_h2d, v->stream));
    HV_HIP(hipEventSynchronize(v->ev_h2d));
    return HV_OK;
}

int hv_h2d(hv_volume *v, void *dst, const void *src, size_t bytes) {
    bool pending = false;
    const int rc = hv_h2d_lazy(v, dst, src, bytes, &pending);
    return rc != HV_OK ? rc : hv_h2d_fence(v, pending);
}

int HvStage::add(void *user, size_t bytes, size_t row_bytes, bool is_out, int32_t where) {
    if (count == MAX_PIECES) {
        overflow = true;
        return 0;
    }
    const bool present = user != nullptr && bytes > 0;
    piece[count] = Piece{present ? user : nullptr, present ? bytes : 0, row_bytes, is_out, (where < 0 ? loc : where) == HV_HOST, nullptr};
    return count++;
}

int HvStage::commit(void **buf, size_t *cur) {
    HV_REQUIRE(!overflow, HV_ERR_INVALID, "HvStage: more than %d arguments", MAX_PIECES);
    const size_t pad = 255;
    size_t off[MAX_PIECES], total = (head_bytes + pad) & ~pad;
    for (int i = 0; i < count; ++i) {
        off[i] = total;
        if (piece[i].staged) total += (piece[i].bytes + pad) & ~pad;
    }
    // everything is sized before the one growth: a pointer handed out below stays valid for the rest of the call
    if (total > 0) {
        const int rc = hv_ensure_buffer(v, buf, cur, total);
        if (rc != HV_OK) return rc;
    }
    char *base = total > 0 ? (char *)*buf : nullptr;
    head_dev = head_bytes > 0 ? base : nullptr;
    bool pending = false;
    for (int i = 0; i < count; ++i) {
        Piece &p = piece[i];
        p.dev = p.bytes == 0 ? nullptr : (p.staged ? base + off[i] : p.user);
        if (p.staged && !p.out) {
            const int rc = hv_h2d_lazy(v, p.dev, p.user, p.bytes, &pending);
            if (rc != HV_OK) return rc;
        }
    }
    return hv_h2d_fence(v, pending); // one fence behind all the call's copies
}

void HvStage::rows(int64_t m) {
    for (int i = 0; i < count; ++i)
        if (piece[i].out && piece[i].row_bytes > 0) piece[i].bytes = std::min(piece[i].bytes, piece[i].row_bytes * (size_t)std::max<int64_t>(m, 0));
}

int HvStage::finish(void *extra, size_t extra_bytes, const void *extra_dev) {
    bool copied = false;
    for (int i = 0; i < count; ++i) {
        const Piece &p = piece[i];
        if (!p.out || !p.staged || p.bytes == 0) continue;
        HV_HIP(hipMemcpyAsync(p.user, p.dev, p.bytes, hipMemcpyDeviceToHost, v->stream));
        copied = true;
    }
    if (extra != nullptr && extra_bytes > 0) {
        HV_HIP(hipMemcpyAsync(extra, extra_dev != nullptr ? extra_dev : head_dev, extra_bytes, hipMemcpyDeviceToHost, v->stream));
        copied = true;
    }
    if (copied) HV_HIP(hipStreamSynchronize(v->stream));
    return HV_OK;
}

int hv_stage_frame(hv_volume *v, const void *depth, int32_t depth_dtype, const uint8_t *rgb, size_t npx, int32_t loc, const void **d_depth,
                   const uint8_t **d_rgb) {
    HvStage st(v, loc);
    const int i_depth = st.in(depth, npx * (depth_dtype == HV_DEPTH_U16 ? 2 : 4)), i_rgb = st.in(rgb, npx * 3);
    const int rc = st.commit(&v->stage, &v->stage_bytes);
    *d_depth = st.dev<const void>(i_depth);
    *d_rgb = st.dev<const uint8_t>(i_rgb);
    return rc;
}
