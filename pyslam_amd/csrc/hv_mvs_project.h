// Rule M3 of include/hipvol.h, the projection of a reference pixel into a source view through its 3x4 matrix [A | b]: what the plane
// sweep of hv_mvs_sgm (hv_mvs.hip) and the forward step of hv_depth_consistency (hv_depth_consistency.hip, rule C2) share.  One copy
// of the rule: both callers are held bit for bit to numpy restatements that state it once (tests/mvs_reference.py project()).
#pragma once
#include "hv_common.h"

static constexpr int MVS_MAX_VIEWS = 4;

// Rule M3, first line: a = A p for the reference pixel (x, y).  One multiply and one add per term, in this order.
__device__ __forceinline__ void mvs_ray(const float *__restrict__ m, int x, int y, float (&a)[3]) {
    const float fx = (float)x, fy = (float)y;
#pragma unroll
    for (int i = 0; i < 3; ++i) a[i] = (m[4 * i] * fx + m[4 * i + 1] * fy) + m[4 * i + 2];
}

// Rule M3, the rest: the source pixel of the plane with inverse depth w, -1 when the view does not see it.  IEEE division, ties to
// even; every comparison is a float comparison, so a NaN fails.  -> vr W + ur
__device__ __forceinline__ int mvs_source_pixel(const float (&a)[3], const float *__restrict__ m, float w, int H, int W) {
    const float q0 = a[0] + w * m[3], q1 = a[1] + w * m[7], q2 = a[2] + w * m[11];
    const float ur = rintf(q0 / q2), vr = rintf(q1 / q2);
    const bool seen = q2 > 0.0f && ur >= 0.0f && ur <= (float)(W - 1) && vr >= 0.0f && vr <= (float)(H - 1);
    return seen ? (int)vr * W + (int)ur : -1;
}
