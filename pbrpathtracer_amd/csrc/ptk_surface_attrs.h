// What is AT a surface point (triangle, u, v): the one statement of the shading quantities shade_interaction computes at an
// interaction, for the two kernels that give them to a caller - features_kernel (ptk_features.hip: the pinhole ray of a pixel) and
// attributes_kernel (ptk_attributes.hip: any (triangle, bary) pair; include/ptk.h ptk_surface_attributes has the rule operation by
// operation).  The same IEEE operations in the same order as the exact trace kernel, on the records of that triangle only; both
// units are compiled with -ffp-contract=off.
#pragma once
#include "ptk_device_fn.h"

namespace ptk {

// which quantities are wanted: bit PTK_ATTR_* of include/ptk.h (POSITION is not the function's: it needs the vertices, not the records)
enum : uint32_t {
    SA_MATERIAL = 1u << 0, SA_UV = 1u << 1, SA_POSITION = 1u << 2, SA_NORMAL_GEOM = 1u << 3, SA_NORMAL = 1u << 4, SA_ALBEDO = 1u << 5,
    SA_EMISSION = 1u << 6, SA_GLOSS = 1u << 7, SA_OPACITY = 1u << 8,
    SA_SHADED = SA_NORMAL | SA_ALBEDO | SA_EMISSION | SA_GLOSS | SA_OPACITY          // what reads the material record
};

// The caller fills in the values of a miss and calls surface_attrs for a hit: only the wanted members are written (and material,
// ng, which cost nothing beyond s0).
struct SurfaceAttrs {
    int material;
    float uvx, uvy;
    v3 ng, n, albedo, emission;
    float roughness, reflectiveness, opacity;
};

// P: anything with shade, mats, texinfo, texels.  tri is a valid triangle index; u, v are used as given.  want is uniform over
// the wave (kernel arguments), so every `want &` below is a scalar branch.  flip: negate the shading normal when dot(n, rd) > 0
// (a NaN does not flip); rd is read only then.  Record reads: s0 always; s1, s2 for the texture coordinate, which is computed when
// it is wanted or some map of the material is bound; the material record and texels only for SA_SHADED.
template <class PT>
__device__ __forceinline__ void surface_attrs(const PT& P, int tri, float u, float v, bool flip, v3 rd, uint32_t want, SurfaceAttrs& A)
{
    const float4* sp4 = P.shade + (size_t)tri * SHADE_F4;
    const float4 s0 = ldg4(sp4);
    const int mbits = __float_as_int(s0.w);
    const int matid = mbits & 0x7fffffff;
    A.material = matid;
    A.ng = V(s0.x, s0.y, s0.z);
    if (!(want & (SA_SHADED | SA_UV))) return;
    const float4* mp = P.mats + (size_t)matid * MAT_F4;
    int tex_diffuse = -1, tex_normal = -1, tex_emiss = -1, tex_rough = -1, tex_metal = -1, tex_opacity = -1;
    bool any_tex = false;
    if (want & SA_SHADED)
    {
        const float4 m4f = ldg4(mp + 4), m5f = ldg4(mp + 5);
        tex_diffuse = __float_as_int(m4f.x); tex_normal = __float_as_int(m4f.y);
        tex_emiss = __float_as_int(m4f.z); tex_rough = __float_as_int(m4f.w);
        tex_metal = __float_as_int(m5f.x); tex_opacity = __float_as_int(m5f.y);
        any_tex = __float_as_int(m5f.z) != 0;       // some map is bound
    }
    float uvx = 0.0f, uvy = 0.0f;
    if ((want & SA_UV) || any_tex)
    {
        const float4 s1 = ldg4(sp4 + 1), s2 = ldg4(sp4 + 2);
        const float w = 1.0f - u - v;               // GetUV :533-536
        uvx = w * s1.x + u * s1.z + v * s2.x;
        uvy = w * s1.y + u * s1.w + v * s2.y;
    }
    A.uvx = uvx; A.uvy = uvy;
    if (want & SA_NORMAL)
    {
        v3 n = A.ng;
        if (mbits < 0)                              // :556, GetSmoothNormal :538-543
        {
            const float4 s2 = ldg4(sp4 + 2), s3 = ldg4(sp4 + 3), s4 = ldg4(sp4 + 4);
            const float w = 1.0f - u - v;
            const v3 n1 = V(s2.z, s2.w, s3.x), n2 = V(s3.y, s3.z, s3.w), n3 = V(s4.x, s4.y, s4.z);
            n = normalize(add(add(muls(n1, w), muls(n2, u)), muls(n3, v)));
        }
        if (tex_normal >= 0)                        // :558-566
        {
            const float4 s4 = ldg4(sp4 + 4), s5 = ldg4(sp4 + 5), s6 = ldg4(sp4 + 6);
            const float4 c = tex2d(P, tex_normal, uvx, uvy);
            v3 nt = V(c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f);
            if (nt.z <= 0.0f) nt = V(nt.x, nt.y, PTK_EPS);
            nt = normalize(nt);
            const v3 tg = V(s4.w, s5.x, s5.y), bt = V(s5.z, s5.w, s6.x);
            const v3 m = V(tg.x * nt.x + bt.x * nt.y + n.x * nt.z,
                           tg.y * nt.x + bt.y * nt.y + n.y * nt.z,
                           tg.z * nt.x + bt.z * nt.y + n.z * nt.z);
            n = normalize(m);
        }
        if (flip && dot(n, rd) > 0.0f) n = neg(n);  // :567-568
        A.n = n;
    }
    if (want & SA_ALBEDO)
    {
        const float4 m0 = ldg4(mp);
        A.albedo = V(m0.x, m0.y, m0.z);
        if (tex_diffuse >= 0) { const float4 c = tex2d(P, tex_diffuse, uvx, uvy); A.albedo = V(c.x, c.y, c.z); }
    }
    if (want & SA_EMISSION)
    {
        const float4 m1 = ldg4(mp + 1), m2 = ldg4(mp + 2);
        v3 emiss = V(m2.x, m2.y, m2.z);
        if (tex_emiss >= 0) { const float4 c = tex2d(P, tex_emiss, uvx, uvy); emiss = V(c.x, c.y, c.z); }
        A.emission = muls(emiss, m1.w);
    }
    if (want & SA_GLOSS)
    {
        A.roughness = ldg4(mp + 2).w;
        if (tex_rough >= 0) A.roughness = tex2d_r(P, tex_rough, uvx, uvy);
        A.reflectiveness = ldg4(mp + 3).x;
        if (tex_metal >= 0) A.reflectiveness = tex2d_r(P, tex_metal, uvx, uvy);
    }
    if (want & SA_OPACITY)
    {
        A.opacity = 1.0f;                           // tri_test's texel: the value its opacity draw is compared with
        if (tex_opacity >= 0) A.opacity = tex2d_r(P, tex_opacity, uvx, uvy);
    }
}

}  // namespace ptk
