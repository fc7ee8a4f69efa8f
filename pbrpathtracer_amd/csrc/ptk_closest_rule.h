// The closest-point rule of include/ptk.h (ptk_closest_points: THE RULE) for one 48-byte record, whole: d2k, the barycentrics v, w and
// the point q.  The one statement of the rule in the library: closest_kernel (ptk_closest.hip) puts its accept behind it,
// nearest_kernel (ptk_knearest.hip) takes the key from it in its leaf arm and v, w and q again in its epilogue, overlap_kernel
// (ptk_overlap.hip) takes a sphere's d2k.  To be compiled with -ffp-contract=off only: every operation is one IEEE float32 operation.
#pragma once

#include "ptk_device_fn.h"

namespace ptk {

struct ClosestRule { float d2k, v, w; v3 q; };

__device__ __forceinline__ ClosestRule closest_rule(const v3 p, const float4 t0, const float4 t1, const float4 t2)
{
    const v3 a = V(t0.x, t0.y, t0.z), e1 = V(t0.w, t1.x, t1.y), e2 = V(t1.z, t1.w, t2.x);
    const v3 ap = sub(p, a), bp = sub(ap, e1), cp = sub(ap, e2);
    const float d1 = dot(e1, ap), d2 = dot(e2, ap), d3 = dot(e1, bp), d4 = dot(e2, bp), d5 = dot(e1, cp), d6 = dot(e2, cp);
    const float vc = d1 * d4 - d3 * d2, vb = d5 * d2 - d1 * d6, va = d3 * d6 - d5 * d4, e43 = d4 - d3, e56 = d5 - d6;
    const bool r0 = (d1 <= 0.0f) & (d2 <= 0.0f);
    const bool r1 = (d3 >= 0.0f) & (d4 <= d3);
    const bool r3 = (vc <= 0.0f) & (d1 >= 0.0f) & (d3 <= 0.0f);
    const bool r2 = (d6 >= 0.0f) & (d5 <= d6);
    const bool r4 = (vb <= 0.0f) & (d2 >= 0.0f) & (d6 <= 0.0f);
    const bool r5 = (va <= 0.0f) & (e43 >= 0.0f) & (e56 >= 0.0f);
    const int reg = r0 ? 0 : (r1 ? 1 : (r3 ? 3 : (r2 ? 2 : (r4 ? 4 : (r5 ? 5 : 7)))));
    // two IEEE divisions serve every region: A = v of the edge 1-2 / the face, B = w of the edges 1-3, 2-3 / the face
    const float den = (va + vb) + vc;
    const bool useA = (reg == 3) | (reg == 7), useB = reg >= 4;
    const float numA = reg == 3 ? d1 : vb, denA = reg == 3 ? d1 - d3 : den;
    const float numB = reg == 4 ? d2 : (reg == 5 ? e43 : vc), denB = reg == 4 ? d2 - d6 : (reg == 5 ? e43 + e56 : den);
    const float A = (useA ? numA : 0.0f) / (useA ? denA : 1.0f), B = (useB ? numB : 0.0f) / (useB ? denB : 1.0f);
    float v = reg == 1 ? 1.0f : (reg == 5 ? 1.0f - B : (useA ? A : 0.0f));
    float w = reg == 2 ? 1.0f : (useB ? B : 0.0f);
    v = v > 0.0f ? v : 0.0f;                 // (a NaN becomes 0)
    v = v < 1.0f ? v : 1.0f;
    w = w > 0.0f ? w : 0.0f;
    const float top = 1.0f - v;
    w = w < top ? w : top;
    ClosestRule r;
    r.v = v; r.w = w;
    r.q = V((a.x + e1.x * v) + e2.x * w, (a.y + e1.y * v) + e2.y * w, (a.z + e1.z * v) + e2.z * w);
    const v3 d = sub(p, r.q);
    r.d2k = dot(d, d);
    return r;
}

}  // namespace ptk
