// The one place a BVH4 record (ptk_device.h) is written on the device: shared by the device builder's collapse
// (bvh_device.hip) and the refit (ptk_refit.hip), so that a refit of unmoved triangles reproduces the builder's record bit
// for bit.  The host builder's emit_node (bvh_build.cpp) states the same rule in host code.
#pragma once

#include <hip/hip_runtime.h>
#include <stdint.h>

#include "ptk_device.h"

namespace ptk {

// cmn / cmx: the padded float boxes of the node's nc children (slots 0 .. nc - 1); link: all four links, NODE_EXIT in the
// empty slots.  Union box -> origin; per-axis scale rounded so that origin + 255 * scale reaches the union's upper bound
// (the nextafter loop); child planes quantised OUTWARD with the indices taken in double arithmetic; empty slots 255 / 0.
// umn / umx return the union (the box a parent takes for this node).
__device__ __forceinline__ void emit_wide_node(const float (*cmn)[3], const float (*cmx)[3], int nc, const int32_t* link,
                                               float4* __restrict__ o4, float* umn, float* umx)
{
    for (int a = 0; a < 3; a++) { umn[a] = INFINITY; umx[a] = -INFINITY; }
    for (int k = 0; k < nc; k++)
        for (int a = 0; a < 3; a++) { umn[a] = fminf(umn[a], cmn[k][a]); umx[a] = fmaxf(umx[a], cmx[k][a]); }
    float scale[3];
    uint32_t lo[3] = { 0, 0, 0 }, hi[3] = { 0, 0, 0 };
    for (int a = 0; a < 3; a++)
    {
        const double ext = (double)umx[a] - (double)umn[a];
        float s = (float)(ext / 255.0 * (1.0 + 1e-6));
        if (!(s > 1e-30f)) s = 1e-30f;
        while ((double)umn[a] + 255.0 * (double)s < (double)umx[a]) s = nextafterf(s, INFINITY);
        scale[a] = s;
        for (int k = 0; k < 4; k++)
        {
            if (k >= nc) { lo[a] |= 255u << (8 * k); continue; }          // empty slot: inverted box
            const double o = umn[a], sd = s;
            int ql = (int)floor(((double)cmn[k][a] - o) / sd), qh = (int)ceil(((double)cmx[k][a] - o) / sd);
            ql = min(max(ql, 0), 255); qh = min(max(qh, 0), 255);
            while (ql > 0 && o + ql * sd > (double)cmn[k][a]) ql--;
            while (qh < 255 && o + qh * sd < (double)cmx[k][a]) qh++;
            lo[a] |= (uint32_t)ql << (8 * k); hi[a] |= (uint32_t)qh << (8 * k);
        }
    }
    o4[0] = make_float4(umn[0], umn[1], umn[2], scale[0]);
    o4[1] = make_float4(scale[1], scale[2], __int_as_float(link[0]), __int_as_float(link[1]));
    o4[2] = make_float4(__int_as_float(link[2]), __int_as_float(link[3]), __uint_as_float(lo[0]), __uint_as_float(lo[1]));
    o4[3] = make_float4(__uint_as_float(lo[2]), __uint_as_float(hi[0]), __uint_as_float(hi[1]), __uint_as_float(hi[2]));
}

}  // namespace ptk
