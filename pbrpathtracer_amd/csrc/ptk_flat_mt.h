// The arithmetic of the FLAT pass's triangle test (tri_test_pair, ptk_kernels.hip): Moeller-Trumbore for the two rays a lane sends
// from one point, the bounce ray in the x half and the shadow ray in the y half of a pair type F2, written once for the device
// (F2 = the packed f32 pair) and for the host (tests/cpp/flat_mt_fuzz.cpp: a struct of two floats), operation by operation in the
// reference's order.  ZM is a compile-time mask over the record's six edge words (bit 0..5 = e1.x e1.y e1.z e2.x e2.y e2.z): a
// masked word is known to be stored as +0 or -0 and enters as the empty type Zero, whose operators delete the operation instead
// of performing it - a product with it is Zero, a sum or difference with it is the other operand (negated for Zero - x).
// ZM = 0 is the full text.  DESIGN.md 4.1 has the argument that every ZM whose words are zero accepts the same hits with the
// same bits of t (u, v of a hit may differ in the sign of a zero); flat_zero_class picks the mask for a record.
#pragma once

#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTK_MT_HD __host__ __device__ __forceinline__
#else
#define PTK_MT_HD inline
#endif

namespace ptk_mt {

struct Zero {};
// (the non-template Zero-Zero forms win over the templates, which would otherwise tie)
template <class T> PTK_MT_HD Zero operator*(Zero, const T&) { return Zero(); }
template <class T> PTK_MT_HD Zero operator*(const T&, Zero) { return Zero(); }
PTK_MT_HD Zero operator*(Zero, Zero) { return Zero(); }
template <class T> PTK_MT_HD T operator+(Zero, const T& x) { return x; }
template <class T> PTK_MT_HD T operator+(const T& x, Zero) { return x; }
PTK_MT_HD Zero operator+(Zero, Zero) { return Zero(); }
template <class T> PTK_MT_HD T operator-(const T& x, Zero) { return x; }
template <class T> PTK_MT_HD T operator-(Zero, const T& x) { return -x; }
PTK_MT_HD Zero operator-(Zero, Zero) { return Zero(); }

template <bool Z> struct EdgeWord { typedef float type; static PTK_MT_HD float get(float w) { return w; } };
template <> struct EdgeWord<true> { typedef Zero type; static PTK_MT_HD Zero get(float) { return Zero(); } };
template <class A, class B> struct Same { static const bool value = false; };
template <class A> struct Same<A, A> { static const bool value = true; };

// The masks that are built, by class number (4 bits per triangle in the class table, ptk_device.h FLAT_CLASSES_AT):
// 0 general; 1-3 both edges zero on axis x / y / z (a triangle in an axis plane); 4-15 such a triangle one of whose stored edges
// is parallel to an axis as well - plane axis p, the third zero on e1 or on e2 at one of the two other axes.
constexpr int FLAT_ZERO_CLASSES = 16;
constexpr unsigned flat_zero_mask(int cls)
{
    return cls == 0 ? 0u
         : cls < 4 ? 9u << (cls - 1)
         : (9u << ((cls - 4) >> 2)) | 1u << ((((cls - 4) >> 2) + 1 + ((cls - 4) & 1)) % 3 + (((cls - 4) & 2) ? 3 : 0));
}

// The class of a record from its six stored edge words: the built mask with the most bits that is a subset of the words that
// compare equal to 0.0f (-0 too); the first such in class order.  A record one of whose edges is all zero is general.
PTK_MT_HD int flat_zero_class(const float e[6])
{
    unsigned z = 0;
    for (int k = 0; k < 6; k++) z |= (e[k] == 0.0f ? 1u : 0u) << k;
    if ((z & 7u) == 7u || (z & 56u) == 56u) return 0;
    int best = 0, bits = 0;
    for (int c = 1; c < FLAT_ZERO_CLASSES; c++)
    {
        const unsigned m = flat_zero_mask(c);
        const int n = c < 4 ? 2 : 3;
        if ((m & ~z) == 0u && n > bits) { best = c; bits = n; }
    }
    return best;
}

// a, u, v, t of both rays against one record.  d = the directions (pairs), ro = the origin both rays leave, rcp = 1 / x on a
// pair in the build's arithmetic.  The accept tests are mt_accept's; nothing here branches.
template <unsigned ZM, class F2, class Rcp>
PTK_MT_HD void mt_pair(const F2 dx, const F2 dy, const F2 dz, float rox, float roy, float roz, float v0x, float v0y, float v0z,
                       float e1x_, float e1y_, float e1z_, float e2x_, float e2y_, float e2z_, Rcp rcp, F2& a_out, F2& u_out, F2& v_out, F2& t_out)
{
    const typename EdgeWord<(ZM & 1u) != 0>::type e1x = EdgeWord<(ZM & 1u) != 0>::get(e1x_);
    const typename EdgeWord<(ZM & 2u) != 0>::type e1y = EdgeWord<(ZM & 2u) != 0>::get(e1y_);
    const typename EdgeWord<(ZM & 4u) != 0>::type e1z = EdgeWord<(ZM & 4u) != 0>::get(e1z_);
    const typename EdgeWord<(ZM & 8u) != 0>::type e2x = EdgeWord<(ZM & 8u) != 0>::get(e2x_);
    const typename EdgeWord<(ZM & 16u) != 0>::type e2y = EdgeWord<(ZM & 16u) != 0>::get(e2y_);
    const typename EdgeWord<(ZM & 32u) != 0>::type e2z = EdgeWord<(ZM & 32u) != 0>::get(e2z_);
    // h = cross(rd, edge2)
    const auto hx = dy * e2z - dz * e2y;
    const auto hy = dz * e2x - dx * e2z;
    const auto hz = dx * e2y - dy * e2x;
    const auto a = hx * e1x + hy * e1y + hz * e1z;               // dot(edge1, h)
    // (a keeps a direction component under every mask: an all-NaN direction makes a, f and t NaN, and t > EPS rejects)
    static_assert(!Same<decltype(a), const Zero>::value, "this mask deletes the determinant");
    const F2 f = rcp(a);
    // The two rays of a lane leave the SAME point (shade_interaction starts both at p), so everything of Moeller-Trumbore that
    // depends on the origin alone - s = ro - v0, q = cross(s, edge1), dot(edge2, q) - is the same number for both: computed once
    // in scalar f32 (full rate) instead of twice in packed f32 (half rate), 17 of the ~60 operations per ray and triangle.  The
    // same IEEE operations on the same inputs: bit-identical.  (No shadow ray: its half of the packed values is ignored anyway.)
    const float sx = rox - v0x, sy = roy - v0y, sz = roz - v0z;              // s = ro - v0
    const F2 u = f * (sx * hx + sy * hy + sz * hz);
    const auto qx = sy * e1z - sz * e1y;                         // q = cross(s, edge1)
    const auto qy = sz * e1x - sx * e1z;
    const auto qz = sx * e1y - sy * e1x;
    const F2 v = f * (dx * qx + dy * qy + dz * qz);
    const F2 t = f * (qx * e2x + qy * e2y + qz * e2z);
    a_out = a; u_out = u; v_out = v; t_out = t;
}

// the reference's tests in their negated form, AND-ed (u > 1 is implied, see tri_test in ptk_device_fn.h)
PTK_MT_HD bool mt_accept(float a, float u, float v, float uv, float t, float eps)
{
    return !(__builtin_fabsf(a) < eps) & !(u < 0.0f) & !(v < 0.0f) & !(uv > 1.0f) & (t > eps);
}

// ---- fan-split axis-aligned rectangles: records 2k, 2k + 1 tested as one pair (exact PLAIN pass, csrc/ptk_kernels_rect.hip) ------------
// A quad (p0, p1, p2, p3) split as the fan (p0, p1, p2), (p0, p2, p3) stores two records A, B with the same v0 and e1(B) = e2(A).
// When it is a rectangle in an axis plane (normal axis p, in-plane axes i, j) the stored words are
//   A: e1 = alpha x_i, e2 = alpha x_i + beta x_j        B: e1 = alpha x_i + beta x_j, e2 = beta x_j        every other word a zero
// and when the four alphas and the four betas are the same BITS, Moeller-Trumbore's s, its determinant a (hence f = 1 / a), and t
// are the same operations on the same operand bits for A and B (the pair lemma).  The kind of a pair names p and i:
// kind = 1 + 2 p + s, i = (p + 1 + s) % 3, j = (p + 2 - s) % 3; 0 = no pair.
constexpr int FLAT_RECT_KINDS = 6;
constexpr int rect_plane(int kind) { return (kind - 1) >> 1; }
constexpr int rect_axis_i(int kind) { return (rect_plane(kind) + 1 + ((kind - 1) & 1)) % 3; }
constexpr int rect_axis_j(int kind) { return (rect_plane(kind) + 2 - ((kind - 1) & 1)) % 3; }
// the zero masks of the two records of a pair (both are built classes: plane bits and one more word)
constexpr unsigned rect_mask_a(int kind) { return (9u << rect_plane(kind)) | 1u << rect_axis_j(kind); }
constexpr unsigned rect_mask_b(int kind) { return (9u << rect_plane(kind)) | 8u << rect_axis_i(kind); }

PTK_MT_HD uint32_t mt_bits(float f) { uint32_t u; __builtin_memcpy(&u, &f, 4); return u; }
// the same bits and not a NaN
PTK_MT_HD bool mt_same_word(float x, float y) { return mt_bits(x) == mt_bits(y) && x == y; }

// The kind of the pair (recA, recB), each a record's nine stored words v0.xyz, e1.xyz, e2.xyz; 0 when they are not one.  Zeros
// compare equal to 0.0f (-0 counts, as for the classes); everything else is compared bit by bit, so one ulp anywhere, or a NaN,
// means no pair.  The first kind that fits (two fit only when alpha or beta is itself a zero).
PTK_MT_HD int flat_rect_pair(const float recA[9], const float recB[9])
{
    for (int k = 0; k < 3; k++) if (!mt_same_word(recA[k], recB[k])) return 0;
    const float* e1a = recA + 3; const float* e2a = recA + 6; const float* e1b = recB + 3; const float* e2b = recB + 6;
    for (int kind = 1; kind <= FLAT_RECT_KINDS; kind++)
    {
        const int p = rect_plane(kind), i = rect_axis_i(kind), j = rect_axis_j(kind);
        const bool zeros = e1a[p] == 0.0f && e1a[j] == 0.0f && e2a[p] == 0.0f && e1b[p] == 0.0f && e2b[p] == 0.0f && e2b[i] == 0.0f;
        const bool same = mt_same_word(e1a[i], e2a[i]) && mt_same_word(e1b[i], e2a[i]) && mt_same_word(e1b[j], e2a[j]) && mt_same_word(e2b[j], e2a[j]);
        if (zeros && same) return kind;
    }
    return 0;
}

// a, u, v, t of both rays against both records of a pair of kind KIND.  The existing arithmetic twice, under the two records' zero
// masks, with every word of B - and A's alpha - NAMED as the word of e2(A) it is bitwise equal to: nothing is shared by hand, the
// compiler's common-subexpression elimination finds s, two h products, a, f, two q products and t of B among A's values.
template <int KIND, class F2, class Rcp>
PTK_MT_HD void mt_rect_pair(const F2 dx, const F2 dy, const F2 dz, float rox, float roy, float roz, float v0x, float v0y, float v0z,
                            float e2x, float e2y, float e2z, Rcp rcp, F2& aA, F2& uA, F2& vA, F2& tA, F2& aB, F2& uB, F2& vB, F2& tB)
{
    static_assert(KIND >= 1 && KIND <= FLAT_RECT_KINDS, "kinds are 1..6");
    mt_pair<rect_mask_a(KIND)>(dx, dy, dz, rox, roy, roz, v0x, v0y, v0z, e2x, e2y, e2z, e2x, e2y, e2z, rcp, aA, uA, vA, tA);
    mt_pair<rect_mask_b(KIND)>(dx, dy, dz, rox, roy, roz, v0x, v0y, v0z, e2x, e2y, e2z, e2x, e2y, e2z, rcp, aB, uB, vB, tB);
}

// The accept decisions of the pair for one ray, in the pass's sequential order (A, then B against the best A may have left), from
// A's a and t, which are B's: X = |a| >= eps, t > eps, t < best is one value for both; an accepted A makes best.t = t, so B's
// t < best fails, and a rejected A leaves best where it was.  NaN directions make a and t NaN and reject through X.
PTK_MT_HD void mt_rect_accept(float a, float t, float uA, float vA, float uvA, float uB, float vB, float uvB, float best_t, float eps, bool& okA, bool& okB)
{
    const bool X = !(__builtin_fabsf(a) < eps) & (t > eps) & (t < best_t);
    okA = X & !(uA < 0.0f) & !(vA < 0.0f) & !(uvA > 1.0f);
    okB = X & !(uB < 0.0f) & !(vB < 0.0f) & !(uvB > 1.0f) & !okA;
}

// The same rule as one update per ray, the form the pair pass runs (tri_accept_rect, ptk_kernels.hip): hit = the ray's best changes,
// first = the record it changes to is A.  With inA, inB the three barycentric tests of each record, okA = X & inA and
// okB = X & inB & !okA, so hit = okA | okB = X & (inA | inB & !(X & inA)) = X & (inA | inB); and under hit X holds, so the accepted
// record is A exactly when inA (okA = inA, and okB only when !inA).  Both write the same t.  (tests/cpp/flat_rect_accept_fuzz.cpp)
PTK_MT_HD void mt_rect_accept_once(float a, float t, float uA, float vA, float uvA, float uB, float vB, float uvB, float best_t, float eps, bool& hit, bool& first)
{
    const bool X = !(__builtin_fabsf(a) < eps) & (t > eps) & (t < best_t);
    const bool inA = !(uA < 0.0f) & !(vA < 0.0f) & !(uvA > 1.0f);
    const bool inB = !(uB < 0.0f) & !(vB < 0.0f) & !(uvB > 1.0f);
    hit = X & (inA | inB);
    first = inA;
}

}  // namespace ptk_mt
