// Device functions shared by every kernel file of libptk.so, all __forceinline__: the v3 arithmetic in the reference's order, the
// exact 1 / x and sqrt (rcp_ieee, sqrt_ieee), the RNG and its keys, tex2d, the re-entrant BVH walk (Walk, tri_test, walk_step), the
// light sampler, one surface interaction of Trace (shade_interaction), the owned-tile / quadrant pixel mapping and the 8-bit resolve.  PTK_CONTRACT selects namespace and arithmetic:
// 0 (the default: what a file that does not define it gets) namespace ptk, every operation the IEEE operation of the CPU oracle;
// 1 ptk::fma, the same text for -ffp-contract=fast; 2 ptk::fast, 1 / x, sqrt and 1 / sqrt straight from the hardware as well.
// Only ptk_kernels.hip is built at levels 1 and 2 (see there).  The committed counter files are tied to this file's sha256
// (kernel_header_sha256, profiles/README.md) beside that of ptk_kernels.hip + ptk_device.h: the trace kernels' walk is here.
#pragma once

#include "ptk_device.h"
#include "ptk_angle_f32.h"

#ifndef PTK_CONTRACT
#define PTK_CONTRACT 0
#endif
// The cycle unit (ptk_kernels_cycle.hip: the exact PLAIN kernels, nothing else) compiles its shade block's table reads and its
// hemisphere angle in forms that hold for that block alone: ldg_at, sincos_2pi_theta_f32.  Every other unit gets 0 here and the
// text it always had.
#if defined(PTK_CYCLE_UNIT) && !PTK_CONTRACT
#define PTK_SHADE32 1
#else
#define PTK_SHADE32 0
#endif
// ... and its square roots: sqrt_ieee_rsq below.

namespace ptk {
#if PTK_CONTRACT >= 2
namespace fast {
#elif PTK_CONTRACT
namespace fma {
#endif

#define PTK_EPS 0.00001f                        // mesh.h:12
#define PTK_FLT_EPSILON 1.1920928955078125e-7f
#define PTK_PI_D 3.14159265358979323846
#define PTK_BLOCK 256
#define PTK_NOHIT 0x7fffffff
// rows of the per-lane LDS traversal stack: the most entries the tree may defer, plus one row of slack that walk_step's
// branchless pushes write into (every link is stored at the running top, also one that does not stay)
#define PTK_STACK_ROWS (PTK_MAX_BVH_DEPTH + 1)

struct v3 { float x, y, z; };

__device__ __forceinline__ v3 V(float x, float y, float z) { v3 r; r.x = x; r.y = y; r.z = z; return r; }
__device__ __forceinline__ v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
__device__ __forceinline__ v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
__device__ __forceinline__ v3 mulv(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
__device__ __forceinline__ v3 muls(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
__device__ __forceinline__ v3 neg(v3 a) { return V(-a.x, -a.y, -a.z); }
// glm 0.9.3.1 dot / cross / normalize / reflect (include/glm/core/func_geometric.inl:161-283)
__device__ __forceinline__ float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
__device__ __forceinline__ v3 cross(v3 x, v3 y)
{
    return V(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
// 1.0f / a, BIT FOR BIT the IEEE-754 round-to-nearest quotient the oracle and the reference compute, for every float with
// 2^-126 <= |a| <= 2^126: v_rcp_f32 (1 ulp) and one Newton step with an exact residual.  Proven by enumeration - all 2^32
// bit patterns on this GPU, tools/microbench/exact_math.hip, profiles/r02/exact_math.json: 0 mismatches in that range - and
// 13 issue cycles instead of the 43 of the compiler's v_div_scale / v_div_fmas / v_div_fixup expansion (which exists for the
// denormal ranges).  The range cannot be left by a triangle's determinant or a vector's length while scene coordinates stay
// below 2^61 in magnitude, which ptk_upload_scene enforces.
__device__ __forceinline__ float rcp_ieee(float a)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_rcpf(a);
#else
    const float y = __builtin_amdgcn_rcpf(a);
    const float e = __builtin_fmaf(-a, y, 1.0f);
    return __builtin_fmaf(y, e, y);
#endif
}
// ... plus IEEE results for zeros, infinities and NaNs (one v_div_fixup_f32): where a zero length can occur
__device__ __forceinline__ float rcp_ieee_any(float a)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_rcpf(a);
#else
    return __builtin_amdgcn_div_fixupf(rcp_ieee(a), a, 1.0f);
#endif
}
// sqrtf(x), BIT FOR BIT the correctly rounded IEEE-754 root: v_sqrt_f32 (1 ulp) and the exact residuals (fma) of its two
// neighbours - the core of the compiler's own expansion without its range scaling (x < 2^-96 is multiplied by 2^32 first)
// and special-case selects.  Enumerated over all 2^32 bit patterns (tools/microbench/exact_math.hip, profiles/r02/
// exact_math.json): identical to sqrtf for +0, +inf and every x >= 2^-104 (the largest input that differs is 0x0b6e9372,
// where the residuals underflow); anything below - a positive length under 2^-52, which no scene produces, and negative
// or NaN arguments - takes the compiler's expansion behind a branch that is practically never taken.
__device__ __forceinline__ float sqrt_ieee_rsq(float x);
__device__ __forceinline__ float sqrt_ieee(float x)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_sqrtf(x);
#elif PTK_SHADE32
    return sqrt_ieee_rsq(x);                    // the cycle unit's shade block: the same bits from the shorter sequence below
#else
    if (__builtin_expect(!(x >= 0x1p-104f), 0)) return sqrtf(x);          // (zero too: correct either way, and as rare)
    float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x), rp = __builtin_fmaf(-sp, s, x);
    s = rm <= 0.0f ? sm : s;
    return rp > 0.0f ? sp : s;
#endif
}
// The same root from v_rsq_f32 (1 ulp): g = x * rsq(x) ~ sqrt(x), corrected once by its exact residual r = x - g * g (fma) times
// h = rsq(x) / 2 ~ 1 / (2 sqrt(x)) - one transcendental, two multiplies and two fma, no compare and no select.  Enumerated over all
// 2^32 bit patterns on the GPU WITH the range test in front (tools/microbench/exact_math.hip, profiles/r15/exact_math_rsq.json):
// identical to sqrtf everywhere.  That is a fact about this hardware's v_rsq_f32, not about every 1-ulp rsq - a host model that
// moves rsq by an ulp finds a few inputs where only the longer coupled form (g and h refined together by a Newton step first;
// enumerated beside it, exact as well) holds - so the enumeration is the proof, and tests/test_gpu_sqrt_rsq.py holds this library's
// code on every mantissa of eight binades.  The short form is exact for x in [2^-102, +inf) - below, the residual underflows - and
// wrong for zero (rsq = inf) and for +inf (rsq = 0, g = NaN), so ONE test sends everything outside that interval - zeros, smaller
// positives, +inf, negatives, NaNs - to the compiler's expansion behind the never-taken branch: as unsigned numbers the interval's
// bit patterns are consecutive, one subtraction and one compare.  The cycle unit's sqrt_ieee is this function; every other unit
// has it for the probe alone.
__device__ __forceinline__ float sqrt_ieee_rsq(float x)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_sqrtf(x);
#else
    if (__builtin_expect(!(__float_as_uint(x) - 0x0c800000u < 0x7f800000u - 0x0c800000u), 0)) return sqrtf(x);
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y, h = 0.5f * y;
    const float r = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(r, h, g);
#endif
}
// the factor normalize() multiplies by: glm's inversesqrt = 1 / sqrt(x), two IEEE roundings (level 2: v_rsq_f32)
__device__ __forceinline__ float inv_length(float sqr)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_rsqf(sqr);
#else
    return rcp_ieee_any(sqrt_ieee(sqr));
#endif
}
// ... over sqrt_ieee_rsq, as the cycle unit compiles inv_length (the probe's op 7)
__device__ __forceinline__ float inv_length_rsq(float sqr)
{
#if PTK_CONTRACT >= 2
    return __builtin_amdgcn_rsqf(sqr);
#else
    return rcp_ieee_any(sqrt_ieee_rsq(sqr));
#endif
}
__device__ __forceinline__ v3 normalize(v3 a)
{
    float sqr = a.x * a.x + a.y * a.y + a.z * a.z;
    return muls(a, inv_length(sqr));
}
__device__ __forceinline__ v3 reflect(v3 I, v3 N)
{
    float d = dot(N, I);
    return sub(I, muls(muls(N, d), 2.0f));
}

// sin/cos on [0, 2*pi]: fixed polynomial shared (by construction, not by source) with the oracle
__device__ __forceinline__ void sincos_2pi(float a, float& s, float& c)
{
    int k = (int)(a * 0.636619772367581343f + 0.5f);
    float r = (float)((double)a - (double)k * 1.57079632679489661923);
    sincos_reduced(k, r, s, c);                 // (ptk_angle_f32.h: the polynomial and the quadrant selects)
}

// ---- RNG (replaces PathTracer::Rand, pathtracer.cpp:367-371) -----------------------------------
__device__ __forceinline__ uint32_t pcg_out(uint32_t st)
{
    uint32_t w = ((st >> ((st >> 28u) + 4u)) ^ st) * 277803737u;
    return (w >> 22u) ^ w;
}
__device__ __forceinline__ uint32_t hash32(uint32_t x) { return pcg_out(x * 747796405u + 2891336453u); }
__device__ __forceinline__ float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }

struct Rng {
    uint32_t state, inc, key;
    __device__ __forceinline__ float next()
    {
        uint32_t old = state;
        state = old * 747796405u + inc;
        return u01(pcg_out(old));
    }
    __device__ __forceinline__ float opacity(uint32_t ray, uint32_t tri) const
    {
        return u01(hash32(tri + hash32(ray + key)));
    }
};

__device__ __forceinline__ float4 ldg4(const float4* p) { return *p; }
// The record at byte offset `off` of a table whose address is wave-uniform (a launch parameter): the load takes the base from an SGPR
// pair and the offset from ONE 32-bit register (global_load ..., v_off, s[base:base+1] offset:imm - constant parts go into `base`
// and land in the immediate), where table[index] costs a 64-bit multiply-add or shift and copies of the base into a VGPR pair.
// Only for tables below 2^32 bytes: the host launches no kernel that reads through this otherwise (ptk_table_offset.h).
template <class T>
__device__ __forceinline__ T ldg_at(const T* base, uint32_t off) { return *(const T*)((const char*)base + off); }
typedef float f2 __attribute__((ext_vector_type(2)));
// (float)byte / 255.0f, exactly: the double product rounds to the same float for all 256 bytes
// (checked exhaustively in tests/test_host_cpu.py); saves the IEEE division sequence
__device__ __forceinline__ float unorm8(uint32_t b) { return (float)((double)b * (1.0 / 255.0)); }

// ---- Image::tex2D (image.cpp:63-86), nearest + repeat, RGBA8 atlas -----------------------------------
template <class PT>
__device__ __forceinline__ float4 tex2d(const PT& P, int tex, float uvx, float uvy)
{
    int4 ti = P.texinfo[tex];
    float u = uvx - truncf(uvx);              // == fmodf(uvx, 1.0f), exact
    float v = uvy - truncf(uvy);
    if (u < 0.0f) u += 1.0f;
    if (v < 0.0f) v += 1.0f;
    int cx = (int)((float)ti.x * u);
    int cy = (int)((float)ti.y * v);
    cx = min(cx, ti.x - 1); cy = min(cy, ti.y - 1);
    cx = max(cx, 0); cy = max(cy, 0);
    uint32_t w = P.texels[(size_t)ti.z + (size_t)cy * (size_t)ti.x + (size_t)cx];
    float4 r;
    r.x = unorm8(w & 255u);
    r.y = unorm8((w >> 8) & 255u);
    r.z = unorm8((w >> 16) & 255u);
    r.w = unorm8(w >> 24);
    return r;
}
template <class PT>
__device__ __forceinline__ float tex2d_r(const PT& P, int tex, float uvx, float uvy)
{
    int4 ti = P.texinfo[tex];
    float u = uvx - truncf(uvx);
    float v = uvy - truncf(uvy);
    if (u < 0.0f) u += 1.0f;
    if (v < 0.0f) v += 1.0f;
    int cx = (int)((float)ti.x * u);
    int cy = (int)((float)ti.y * v);
    cx = min(cx, ti.x - 1); cy = min(cy, ti.y - 1);
    cx = max(cx, 0); cy = max(cy, 0);
    uint32_t w = P.texels[(size_t)ti.z + (size_t)cy * (size_t)ti.x + (size_t)cx];
    return unorm8(w & 255u);
}

struct Hit { int tri; float t, u, v; };

struct Counters { uint32_t rays, shadow, nodes, tris, shaded, tex, walk_iters, walk_lanes, shade_execs, shade_lanes, gen_execs, gen_lanes, tri_execs, tri_lanes, cur_nodes, max_nodes, started; };

// ---- closest hit (replaces the recursive PathTracer::Hit, pathtracer.cpp:411-492) ---------------------
// The walk is re-entrant: all of its state lives in this struct so a wave can interleave BVH steps
// with shading of other lanes.  stack: this thread's column of the block's LDS stack, element k at
// stack[k * PTK_BLOCK].
struct Walk {
    v3 ro, rd, inv;
    v3 cn, cf;                   // per axis: -(ro * inv + slack) and slack - ro * inv, the constant terms of a node's near / far slab
                                 // distances for this ray; slack = what the slab arithmetic can be off by for any node (walk_step)
    uint32_t sgnx, sgny, sgnz;   // per axis: all ones when the ray travels towards -axis (selects the near / far plane bytes with one v_bfi each)
    int node;
    int* top;                    // this lane's stack top in LDS (== its column's base when empty); unused by the FLAT kernel
    int tri_next, tri_left;      // pending leaf: records [tri_next, tri_next + tri_left) still to test
    Hit best;
    // occl_tri >= 0 marks a shadow ray towards light triangle occl_tri.  DirectIllumimation's test (pathtracer.cpp:522-526) is
    // "the closest hit along the ray is the light triangle (or nothing)".  The light triangle is tested FIRST, before the walk
    // (its record comes with the light sample), so `best` already holds its hit - if the ray hits it at all - and any other
    // triangle the walk then accepts is, by the closest-hit rule, nearer: it decides the test and ends the walk.  Order
    // independent by construction.  (Round 1 ended the walk on any hit nearer than 0.9999 x the distance to the light SAMPLE:
    // wrong when Moeller-Trumbore places a grazing hit on the light triangle itself nearer than that - found by
    // tools/soak_random_scenes.py, one pixel-sample in 19 of 3000 random scenes.)
    int occl_tri;

    // node: >= 0 interior node to test next; NODE_EXIT nothing left on the node side; any other negative
    // value = a leaf waiting for the triangle queue (tri_next, tri_left) to drain
    __device__ __forceinline__ void begin(v3 o, v3 d, int num_nodes, int* stack, float scene_bound)
    {
        ro = o; rd = d;
        // acceleration only: 1-ulp reciprocals are fine for conservative slab tests.  Clamped to +-1e18 so that a ray
        // parallel to an axis (a zero component: a hemisphere sample with w == 0 about an axis-aligned normal, one path in
        // 2^24) keeps FINITE slab distances of the right sign - with +-inf the quantised form q * (scale * inv) + (origin -
        // ro) * inv turns into NaNs on that axis, the axis stops culling and such a ray walks the whole tree (measured:
        // 228 153 node visits for one ray of the 1 M-triangle scene, a 0.5 s tail per launch)
        inv = V(__builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.x), -1e18f, 1e18f), __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.y), -1e18f, 1e18f),
                __builtin_amdgcn_fmed3f(__builtin_amdgcn_rcpf(d.z), -1e18f, 1e18f));
        // The slab arithmetic of walk_step, t = fma(q, A, B) with A = scale * inv and B = (origin - ro) * inv, is off by at most
        // 2^-21 (|B| + 256 |A|) (see there).  Every node origin lies inside the scene's padded bounds and a node's 255 grid
        // steps span at most the scene, so per axis that is at most 2^-21 (max |ro| + 3.1 scene_bound) |inv| - a property of the RAY,
        // computed here once instead of twelve instructions per node visited.  (In position units 5e-7 x the scene's size:
        // nothing next to a node's own extent until rays come from ~10^5 scene sizes away, where it is exactly what is needed.)
        const float r21 = (fmaxf(fmaxf(fabsf(o.x), fabsf(o.y)), fabsf(o.z)) + scene_bound) * 0x1p-21f;      // (one bound for the three axes)
        const v3 slack = V(r21 * fabsf(inv.x), r21 * fabsf(inv.y), r21 * fabsf(inv.z));
        // ... and folded, with the ray's own share of B, into the constant of ONE fma per plane family and axis:
        //   B -+ slack = origin * inv - ro * inv -+ slack = fma(origin, inv, cn | cf),   cn = fma(-ro, inv, -slack), cf = fma(-ro, inv, slack)
        // (origin * inv - ro * inv instead of (origin - ro) * inv: the cancellation costs 2^-24 (|origin| + |ro|) |inv| at most,
        // which the bound above was derived with - |origin - ro| <= |origin| + |ro| - so it is covered)
        cn = V(__builtin_fmaf(-o.x, inv.x, -slack.x), __builtin_fmaf(-o.y, inv.y, -slack.y), __builtin_fmaf(-o.z, inv.z, -slack.z));
        cf = V(__builtin_fmaf(-o.x, inv.x, slack.x), __builtin_fmaf(-o.y, inv.y, slack.y), __builtin_fmaf(-o.z, inv.z, slack.z));
        sgnx = (uint32_t)(__float_as_int(inv.x) >> 31); sgny = (uint32_t)(__float_as_int(inv.y) >> 31); sgnz = (uint32_t)(__float_as_int(inv.z) >> 31);
        node = num_nodes > 0 ? 0 : NODE_EXIT;
        top = stack;
        tri_next = 0; tri_left = 0;
        best.tri = PTK_NOHIT; best.t = __builtin_inff(); best.u = 0.0f; best.v = 0.0f;
    }
    __device__ __forceinline__ bool done() const { return node == NODE_EXIT && tri_left == 0; }
    template <int STRIDE>
    __device__ __forceinline__ int pop(const int* stack)
    {
        if (top == stack) return NODE_EXIT;
        top -= STRIDE;
        return *top;
    }
};

// Moeller-Trumbore's a, u, v, t of the ray (ro, rd) for one 48-byte triangle record: the one place these float32 operations are
// written, in this order, for every triangle arm of the BVH walk (tri_test, the crossing counts, the multi-hit list and its
// epilogue) - so what one of them decides on is bit for bit what the others compute.
__device__ __forceinline__ void mt_auvt(const v3 ro, const v3 rd, const float4 t0, const float4 t1, const float4 t2, float& a, float& u, float& v,
                                        float& t)
{
    v3 v0 = V(t0.x, t0.y, t0.z);
    v3 edge1 = V(t0.w, t1.x, t1.y);
    v3 edge2 = V(t1.z, t1.w, t2.x);
    v3 h = cross(rd, edge2);
    a = dot(edge1, h);
    float f = rcp_ieee(a);                      // (|a| < EPS, a NaN or infinite: rejected below whatever f is)
    v3 s = sub(ro, v0);
    u = f * dot(s, h);
    v3 q = cross(s, edge1);
    v = f * dot(rd, q);
    t = f * dot(edge2, q);
}

// Candidate test of one triangle record: Hit's leaf branch (pathtracer.cpp:463-489) = Moeller-Trumbore
// + order-independent closest rule + stochastic opacity.  Returns true when the walk can stop (an
// occluder decided a shadow ray).
template <bool STATS, class PT>
__device__ __forceinline__ bool tri_test(const PT& P, Walk& W, float4 t0, float4 t1, float4 t2, const Rng& rng,
                                         uint32_t ray, Counters& cnt)
{
    if (STATS) cnt.tris++;
    // Moeller-Trumbore, PathTracer::IntersectTriangle pathtracer.cpp:373-409.  The reference returns
    // early after each rejection test; here every quantity is computed and the SAME tests (in their
    // negated form, so NaNs fall through exactly as they do there) are AND-ed: identical results for
    // every accepted hit, no divergent branches in the hot loop.
    float a, u, v, t;
    mt_auvt(W.ro, W.rd, t0, t1, t2, a, u, v, t);
    int tri = __float_as_int(t2.y);
    // (the reference also returns on u > 1, pathtracer.cpp:393: implied here - v >= 0 makes fl(u + v) >= u, rounding being
    // monotone, so u > 1 fails the u + v test, and a NaN u passes both forms alike)
    bool ok = !(fabsf(a) < PTK_EPS) & !(u < 0.0f) & !(v < 0.0f) & !(u + v > 1.0f) & (t > PTK_EPS);
    // (t < inf: with a ray origin ~1e30 away q overflows, v is NaN, t +inf - the reference rejects that on u > 1 or on a NaN
    // of its own; without the test the tie rule below would take t == best.t == inf for a hit.  ptk_set_camera bounds the
    // camera position, so only a path that has already left every float range could get here)
    ok = ok & (t < __builtin_inff()) & ((t < W.best.t) | ((t == W.best.t) & (tri < W.best.tri)));
    int otex = __float_as_int(t2.z);
    if (ok && otex >= 0)
    {
        // stochastic opacity, pathtracer.cpp:469-476 (GetUV :533-536); rare: skipped with s_cbranch_execz
        const float4* sp4 = P.shade + (size_t)tri * SHADE_F4;
        float4 s1 = ldg4(sp4 + 1), s2 = ldg4(sp4 + 2);
        float w = 1.0f - u - v;
        float ux = w * s1.x + u * s1.z + v * s2.x;
        float uy = w * s1.y + u * s1.w + v * s2.y;
        float op = tex2d_r(P, otex, ux, uy);
        if (STATS) cnt.tex++;
        ok = rng.opacity(ray, (uint32_t)tri) < op;
    }
    W.best.tri = ok ? tri : W.best.tri;
    W.best.t = ok ? t : W.best.t;
    W.best.u = ok ? u : W.best.u;
    W.best.v = ok ? v : W.best.v;
    return ok & (W.occl_tri >= 0) & (tri != W.occl_tri);
}

// What the walk loop reads of the launch parameters, held in SGPRs for the length of the loop.  The parameters themselves
// live in the constant address space (trace_kernel), where a field is an s_load at its point of use - right for the hundreds of
// fields-times-places outside the hot loop, wrong inside it: the compiler re-issued the loads of the node and triangle pointers
// in EVERY walk iteration and waited for them before the node record could even be requested.  readfirstlane makes the
// values opaque (not re-materialisable as loads).
// (The pointers keep the GLOBAL address space through the integer round trip: a generic pointer would turn every record fetch
// into a flat_load, which is slower and counts against the LDS counter as well.)
#define PTK_GLOBAL __attribute__((address_space(1)))
struct WalkParams {
    const float4* nodes; const float4* tris; const float4* shade;
    const int4* texinfo; const uint32_t* texels;
    int tri_thr, shade_thr, gen_thr;
};
template <class T>
__device__ __forceinline__ T* uniform_ptr(T* p)
{
    const uint64_t v = (uint64_t)(uintptr_t)p;
    const uint32_t lo = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)v), hi = (uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(v >> 32));
    return (T*)(PTK_GLOBAL T*)(uintptr_t)(((uint64_t)hi << 32) | lo);        // integer -> GLOBAL pointer -> generic: the loads stay global_load
}
template <class PT>
__device__ __forceinline__ WalkParams walk_params(const PT& P)
{
    WalkParams w;
    w.nodes = uniform_ptr(P.nodes); w.tris = uniform_ptr(P.tris); w.shade = uniform_ptr(P.shade);
    w.texinfo = uniform_ptr(P.texinfo); w.texels = uniform_ptr(P.texels);
    w.tri_thr = __builtin_amdgcn_readfirstlane(P.tri_thr); w.shade_thr = __builtin_amdgcn_readfirstlane(P.shade_thr);
    w.gen_thr = __builtin_amdgcn_readfirstlane(P.gen_thr);
    return w;
}

// One BVH step of a lane: up to two triangles of the pending leaf (arm A) AND one interior node (arm B).  A leaf
// reached by arm B is parked in the lane's one-entry triangle queue and the descent continues with the next node
// from the stack, so the two arms overlap instead of alternating (the wave executes both arms every iteration anyway).
// The price is slightly later t-max tightening; the result is unaffected (closest hit is order-independent).
struct NodeRec { float4 q0, q1, q2, q3; };      // one 64-byte node record in flight / in registers
// the record of the node a lane will test next (a lane without a node reads the root - every such lane the same 64 bytes - which
// costs less than a branch around the loads and zeroing sixteen registers for the lanes that skip them)
template <class PT>
__device__ __forceinline__ void request_node(const PT& P, const Walk& W, NodeRec& r)
{
    // (a 32-bit byte offset from the wave-uniform base: the load takes its base from an SGPR pair, no 64-bit address arithmetic)
    const float4* np = (const float4*)((const char*)P.nodes + (uint32_t)max(W.node, 0) * (uint32_t)(NODE_F4 * 16));
    r.q0 = ldg4(np); r.q1 = ldg4(np + 1); r.q2 = ldg4(np + 2); r.q3 = ldg4(np + 3);
}
// PIPELINED: the caller's loop keeps a node record in flight ACROSS iterations - `rec` was requested (request_node) before the
// loop or at the end of the lane's previous step, and the record of the node this step ends on is requested before the step
// returns, so its round trip also covers the loop's wave-uniform bookkeeping (ballots, debts, ~30 dependent scalar instructions)
// instead of starting behind it.
// tri: the triangle arm, tri(t0, t1, t2, pos) for the 48-byte record at position `pos` of the triangle table; returns whether the
// walk may stop.  Every record of a leaf is queued exactly once and arm A tests what is queued once each - unless a test stops the
// walk - so an arm that never stops is called exactly once for every record of every leaf the walk reaches: what counting and
// listing crossings need.  Arm B culls against W.best.t, whatever the triangle arm keeps there.
template <bool STATS, int STRIDE, bool PIPELINED, class PT, class TRI>
__device__ __forceinline__ void walk_step_with(const PT& P, Walk& W, int* stack, Counters& cnt, const bool run_tri_arm, NodeRec* rec, TRI tri)
{
    // the node record of arm B is requested BEFORE arm A runs, so that its round trip overlaps arm A's loads and arithmetic
    // (one memory latency per iteration instead of two; the compiler would otherwise issue it after arm A's join)
    NodeRec here;
    if (PIPELINED) here = *rec; else request_node(P, W, here);
    const float4 q0 = here.q0, q1 = here.q1, q2 = here.q2, q3 = here.q3;
    asm volatile("" ::: "memory");
    const bool node_was = W.node >= 0;
    if (run_tri_arm && W.tri_left > 0)                    // ---- arm A: up to TWO triangles
    {
        // The second triangle: the pending leaf's next one, or - the pending leaf has only this one left and the lane is BLOCKED
        // on a second leaf (W.node holds it: the one-leaf queue was busy) - the first triangle of that leaf, whose remainder then
        // becomes the pending leaf while the lane pops its next node.  Both records are requested together and tested one after
        // the other: the same tri_test calls in the same order as one per execution, so results cannot differ.  Leaves hold
        // 1.1-1.5 triangles on average, so what this buys is mostly the blocked leaf - its lane walks on an iteration earlier -
        // and a triangle arm that is voted 44 % less often (round 4: C4 +2 %, C5 +4 %, C3 +4 %; three or four per execution,
        // and the pair in packed f32, measured slower: DESIGN 12).
        const bool two = W.tri_left >= 2;
        const bool blocked = !two & (W.node < 0) & (W.node != NODE_EXIT);
        const int code = ~W.node;
        const int iA = W.tri_next, iB = two ? iA + 1 : (blocked ? (code >> 3) : iA);
        const float4* tpa = (const float4*)((const char*)P.tris + (uint32_t)iA * (uint32_t)(TRI_F4 * 16));
        const float4* tpb = (const float4*)((const char*)P.tris + (uint32_t)iB * (uint32_t)(TRI_F4 * 16));
        float4 a0 = ldg4(tpa), a1 = ldg4(tpa + 1), a2 = ldg4(tpa + 2);
        float4 b0 = ldg4(tpb), b1 = ldg4(tpb + 1), b2 = ldg4(tpb + 2);
        bool stop = tri(a0, a1, a2, (uint32_t)iA);
        if ((two | blocked) && !stop) stop = tri(b0, b1, b2, (uint32_t)iB);
        if (blocked)
        {
            W.tri_next = (code >> 3) + 1; W.tri_left = code & 7;
            W.node = W.template pop<STRIDE>(stack);
        }
        else { W.tri_next = iA + (two ? 2 : 1); W.tri_left -= two ? 2 : 1; }
        W.top = stop ? stack : W.top;                     // an occluder decides a shadow ray: drop everything
        W.tri_left = stop ? 0 : W.tri_left;
        W.node = stop ? NODE_EXIT : W.node;
    }
    if (node_was && W.node >= 0)                          // ---- arm B: one 4-wide interior node (its record is `here`; a node popped by arm A waits a step)
    {
        if (STATS) { cnt.nodes++; cnt.cur_nodes++; }
        // child planes live on the node's 8-bit grid: plane = origin + q * scale, so along the ray
        //   t = (plane - ro) * inv = q * (scale * inv) + (origin - ro) * inv = fma(q, A, B)
        // (box tests are acceleration only - any conservative test gives the same closest hit - so fused
        // multiply-adds and approximate reciprocals are fine here; the grid boxes enclose the padded boxes)
        const float Ax = q0.w * W.inv.x, Ay = q1.x * W.inv.y, Az = q1.y * W.inv.z;
        // CONSERVATIVE for every ray, however far its origin: t = fma(q, A, B) is the sum of two possibly large terms, so its
        // error is absolute - at most 2^-22 (|B| + 255 |A|) from the roundings of the products, the 1-ulp reciprocal and the
        // fmas - i.e. a position error of ~6e-8 x the distance between the ray's origin and the node, which exceeds an 8-bit
        // grid step once that distance is > 65 000 node extents (and Moeller-Trumbore's own decisions carry the same
        // uncertainty, so no padding of the tree can stand in for it).  Near planes are taken that much (x 2) too early and far
        // planes too late; found by tools/soak_bvh.py: two clusters of 1e-3 at +-1e3 gave tree-dependent hits.  The bound is
        // taken per RAY (Walk::begin: |B| <= (|ro| + scene bound) |inv|, 256 |A| <= 2.01 scene bound |inv|) and folded into the
        // ray's constants: six fused multiply-adds per node here (round 2: fifteen instructions).
        const float Bnx = __builtin_fmaf(q0.x, W.inv.x, W.cn.x), Bny = __builtin_fmaf(q0.y, W.inv.y, W.cn.y), Bnz = __builtin_fmaf(q0.z, W.inv.z, W.cn.z);
        const float Bfx = __builtin_fmaf(q0.x, W.inv.x, W.cf.x), Bfy = __builtin_fmaf(q0.y, W.inv.y, W.cf.y), Bfz = __builtin_fmaf(q0.z, W.inv.z, W.cf.z);
        // the ray enters a slab through the low plane when it travels in +axis, through the high plane otherwise:
        // pick the near / far plane bytes of all four children at once by the sign of the direction
        const uint32_t mx = W.sgnx, my = W.sgny, mz = W.sgnz;
        const uint32_t lox = __float_as_uint(q2.z), loy = __float_as_uint(q2.w), loz = __float_as_uint(q3.x);
        const uint32_t hix = __float_as_uint(q3.y), hiy = __float_as_uint(q3.z), hiz = __float_as_uint(q3.w);
        const uint32_t nx = (hix & mx) | (lox & ~mx), fx = (lox & mx) | (hix & ~mx);
        const uint32_t ny = (hiy & my) | (loy & ~my), fy = (loy & my) | (hiy & ~my);
        const uint32_t nz = (hiz & mz) | (loz & ~mz), fz = (loz & mz) | (hiz & ~mz);
        const int link0 = __float_as_int(q1.z), link1 = __float_as_int(q1.w), link2 = __float_as_int(q2.x), link3 = __float_as_int(q2.y);
        // ... and a node is only culled against the closest hit so far when it lies beyond it by more than Moeller-Trumbore's
        // own error in t (relative ~1e-7 / cos of the incidence angle: which of two triangles 1e-6 apart is "closest" is
        // decided by that arithmetic, not by geometry - the second half of the same soak finding)
        const float tmax = W.best.t * 1.0000153f;
        int key[4];
        bool hit[4];
#pragma unroll
        for (int k = 0; k < 4; k++)
        {
            const float tnx = __builtin_fmaf((float)((nx >> (8 * k)) & 255u), Ax, Bnx), tfx = __builtin_fmaf((float)((fx >> (8 * k)) & 255u), Ax, Bfx);
            const float tny = __builtin_fmaf((float)((ny >> (8 * k)) & 255u), Ay, Bny), tfy = __builtin_fmaf((float)((fy >> (8 * k)) & 255u), Ay, Bfy);
            const float tnz = __builtin_fmaf((float)((nz >> (8 * k)) & 255u), Az, Bnz), tfz = __builtin_fmaf((float)((fz >> (8 * k)) & 255u), Az, Bfz);
            // NaNs (0 * inf for axis-parallel rays) drop out of min3 / max3: that axis then does not constrain - conservative
            const float tn = fmaxf(fmaxf(tnx, tny), tnz), tf = fminf(fminf(tfx, tfy), tfz);
            // entry no earlier than the ray's start, exit no later than the closest hit: ONE compare instead of three (and no
            // scalar ands of three lane masks per child; round 4: C4 +1.5 %)
            hit[k] = fmaxf(tn, 0.0f) <= fminf(tf, tmax);
            // order key: the entry distance with the slot in its low bits (negative distances - origin inside - sort first)
            key[k] = hit[k] ? ((__float_as_int(tn) & ~3) | k) : 0x7fffffff;
        }
        const int kmin = min(min(key[0], key[1]), min(key[2], key[3]));
        // the nearest child is the one whose key is the minimum (keys of hit children differ in their slot bits); the same
        // four compares decide which of the others wait on the stack (two hits: exactly far-after-near; more: slot order)
        const bool o0 = key[0] != kmin, o1 = key[1] != kmin, o2 = key[2] != kmin;
        int next = !o0 ? link0 : (!o1 ? link1 : (!o2 ? link2 : link3));
        // every link is written at the running top and the top moves on only behind a link that stays: no exec-mask juggling around
        // four conditional stores (round 4: C4 +2 %; with the clamped compare above: 28 -> 11 scalar instructions per node).  A link
        // that does not stay is still stored, one row above a stack that may be full: hence the slack row of PTK_STACK_ROWS
        *W.top = link0; W.top += (hit[0] & o0) ? STRIDE : 0;
        *W.top = link1; W.top += (hit[1] & o1) ? STRIDE : 0;
        *W.top = link2; W.top += (hit[2] & o2) ? STRIDE : 0;
        *W.top = link3; W.top += (hit[3] & (key[3] != kmin)) ? STRIDE : 0;
        if (kmin == 0x7fffffff) next = W.template pop<STRIDE>(stack);
        W.node = next;
    }
    if (W.node < 0 && W.node != NODE_EXIT && W.tri_left == 0)   // a leaf and the triangle queue is free
    {
        const int code = ~W.node;
        W.tri_next = code >> 3;
        W.tri_left = (code & 7) + 1;
        W.node = W.template pop<STRIDE>(stack);
    }
    if (PIPELINED) request_node(P, W, *rec);                    // for this lane's next step (a finished walk asks for the root: where its next ray starts)
}
// ... with the closest-hit rule in arm A: the step of the trace kernels and of every walk that keeps one hit per ray
template <bool STATS, int STRIDE, bool PIPELINED = false, class PT>
__device__ __forceinline__ void walk_step(const PT& P, Walk& W, const Rng& rng, uint32_t ray, int* stack, Counters& cnt,
                                          const bool run_tri_arm = true, NodeRec* rec = nullptr)
{
    walk_step_with<STATS, STRIDE, PIPELINED>(P, W, stack, cnt, run_tri_arm, rec, [&](const float4 t0, const float4 t1, const float4 t2, uint32_t) {
        return tri_test<STATS>(P, W, t0, t1, t2, rng, ray, cnt);
    });
}

// hemisphere / lobe sampler, pathtracer.cpp:606-611 (:618-623 lobe form): see oracle sample_about()
// its tangent frame: depends on the axis the sampler turns about only, not on the draws (for the hemisphere about an unsmoothed,
// unmapped triangle's normal: one of two values per triangle - fill_flat_frames_kernel tabulates them for the PLAIN kernel)
__device__ __forceinline__ void sample_basis(v3 n_for_test, float thr, v3 basis_from, v3& u, v3& v)
{
    u = fabsf(n_for_test.x) < thr ? cross(V(1.0f, 0.0f, 0.0f), basis_from) : cross(V(1.0f, 1.0f, 1.0f), basis_from);
    u = normalize(u);
    v = normalize(cross(u, basis_from));
}
// ... and the direction drawn in that frame.  theta is a u01 draw at every call
__device__ __forceinline__ v3 sample_in_basis(v3 u, v3 v, v3 pole, float w, float theta)
{
    float sn, cs;
    if (PTK_SHADE32) sincos_2pi_theta_f32(theta, sn, cs);   // the same bits for each of the 2^24 draws, without a double (ptk_angle_f32.h)
    else
    {
        float ang = (float)(2.0f * PTK_PI_D * theta);
        sincos_2pi(ang, sn, cs);
    }
    v3 d = add(add(muls(u, w * cs), muls(v, w * sn)), muls(pole, sqrt_ieee(1.0f - w * w)));
    return normalize(d);
}
__device__ __forceinline__ v3 sample_about(v3 n_for_test, float thr, v3 basis_from, v3 pole, float w, float theta)
{
    v3 u, v;
    sample_basis(n_for_test, thr, basis_from, u, v);
    return sample_in_basis(u, v, pole, w, theta);
}

__device__ __forceinline__ uint32_t pixel_key(uint32_t seed_lo, uint32_t seed_hi, uint32_t pixel)
{
    uint32_t a = hash32(seed_hi);
    uint32_t b = hash32(seed_lo + a);
    return hash32(pixel + b);
}

// DirectIllumimation's sampling half (pathtracer.cpp:494-521, 527-530; SampleTriangle :494-503): picks a light triangle and a
// point on it from three draws, in the reference's order, and returns false when the surface faces away (:518-520).  Its
// visibility half (:522-526, closest hit along l is the light) is the shadow walk the caller starts: towards `l`, with
// occl_tri = light_tri, after testing the light triangle itself (lt0..lt2, its record) first.  di is the value DirectIllumimation returns when that walk finds the
// light (:530).
template <class PT>
__device__ __forceinline__ bool sample_direct_light(const PT& P, v3 p, v3 n, v3 diffuse, float u_light, float u_su, float u_sv,
                                                    v3& l, v3& di, int& light_tri, float4& lt0, float4& lt1, float4& lt2)
{
    int lightId = (int)floorf(u_light * (float)P.num_lights);
    if (lightId == P.num_lights && lightId > 0) lightId--;
    float4 l0, l1, l2, l3;
    if constexpr (PTK_SHADE32)
    {
        const uint32_t lo = (uint32_t)lightId * (uint32_t)(LIGHT_F4 * 16);
        l0 = ldg_at(P.lights, lo); l1 = ldg_at(P.lights + 1, lo); l2 = ldg_at(P.lights + 2, lo); l3 = ldg_at(P.lights + 3, lo);
    }
    else
    {
        const float4* lp = P.lights + (size_t)lightId * LIGHT_F4;
        l0 = ldg4(lp); l1 = ldg4(lp + 1); l2 = ldg4(lp + 2); l3 = ldg4(lp + 3);
    }
    float su = sqrt_ieee(u_su);
    float sv = u_sv;
    float w0 = 1.0f - su, w1 = su * (1.0f - sv), w2 = su * sv;
    v3 vLight = add(add(muls(V(l0.x, l0.y, l0.z), w0), muls(V(l1.x, l1.y, l1.z), w1)),
                    muls(V(l2.x, l2.y, l2.z), w2));
    const v3 dl = sub(vLight, p);
    l = normalize(dl);
    float ndl = dot(neg(n), neg(l));
    light_tri = __float_as_int(l0.w);
    // the light triangle's own record, as the walk would fetch it: v0, e1 = v2 - v1, e2 = v3 - v1 (the same subtractions the
    // record packers perform), its index and opacity texture
    lt0 = make_float4(l0.x, l0.y, l0.z, l1.x - l0.x);
    lt1 = make_float4(l1.y - l0.y, l1.z - l0.z, l2.x - l0.x, l2.y - l0.y);
    lt2 = make_float4(l2.z - l0.z, l0.w, l3.y, 0.0f);
    if (ndl <= 0.0f) return false;              // (:519 in its own form: a NaN normal - a normal map on a mesh without uvs - goes ON, as there)
    v3 lColor = V(l1.w, l2.w, l3.x);
    di = muls(mulv(lColor, diffuse), ndl);      // :530
    return true;
}

// a triangle's entry of the frame table (see FLAT_FRAMES_AT): both sides; nothing in the kernels that compute the frame
template <bool ON> struct FlatFrames { float4 u0, v0, u1, v1; };
template <> struct FlatFrames<false> {};

// One surface interaction of PathTracer::Trace (pathtracer.cpp:551-727) for the hit W.best of the ray (W.ro, W.rd): emission,
// Russian roulette, material branch, direction sampling, the light sample of DirectIllumimation.  Returns true when the path
// ends here; otherwise W holds the next ray to walk (BVH kernels: the shadow ray towards the sampled light - W.occl_tri >= 0,
// W.best = its light triangle's own hit, Tdi its contribution, nextDir the bounce direction that follows - or the bounce
// ray itself; FLAT kernel: W the bounce ray and WS the shadow ray, tested in one pass).  Shared by every trace kernel.
// PLAIN (trace_kernel): every material is opaque and untextured and no triangle is smoothed, so the texture lookups, the UVs,
// the smoothed and normal-mapped normals and the glass branch are dead code; what remains is the mtype == 0 route, operation
// for operation and draw for draw.
// LAMBERT (a PLAIN scene none of whose materials has reflectiveness > 0, ptk.h ptk_scene_is_lambert): the specular draw
// `rng.next() < reflectiveness` (:601) is false for every draw - u01 is never negative, and no x >= 0 is below a zero of either
// sign, a negative or a NaN - so only the stream's advance is left of it and the route is known at compile time: the hemisphere
// sampler about n, weight = diffuse, a light sample.  No bounce is specular, so `iter` equals `depth` and is neither read nor
// written; reflect(), the mirror and lobe samplers, roughness and specular are gone.  Every operation that is left is the PLAIN
// kernel's, in its order.
template <bool STATS, bool FLAT, bool PLAIN, bool LAMBERT, class PT>
__device__ __forceinline__ bool shade_interaction(const PT& P, Walk& W, Walk& WS, int* stack, Rng& rng, v3& L, v3& T, v3& Tdi, v3& nextDir,
                                                  int& depth, int& iter, bool& inside, const uint32_t ray, Counters& cnt)
{
    const Hit h = W.best;
    const v3 ro = W.ro, rd = W.rd;
    if (STATS) cnt.shaded++;
    // (the cycle unit's PLAIN kernels read the three tables by 32-bit byte offsets: ldg_at)
    constexpr bool OFF32 = PTK_SHADE32 && PLAIN;
    const float4* sp4 = P.shade + (size_t)h.tri * SHADE_F4;
    float4 s0;
    if constexpr (OFF32) s0 = ldg_at(P.shade, (uint32_t)h.tri * (uint32_t)(SHADE_F4 * 16)); else s0 = ldg4(sp4);
    int mbits = __float_as_int(s0.w);
    int matid = PLAIN ? mbits : mbits & 0x7fffffff;
    bool smoothing = !PLAIN && mbits < 0;
    const float4* mp = P.mats + (size_t)matid * MAT_F4;
    // the whole 96-byte material in one batch (two of its words are only needed further down: asked for there,
    // they cost the block another memory round trip), and the vertex normals of a smoothed triangle with it
    float4 m0, m1, m2, m3;
    if constexpr (OFF32)
    {
        const uint32_t mo = (uint32_t)matid * (uint32_t)(MAT_F4 * 16);
        m0 = ldg_at(P.mats, mo); m1 = ldg_at(P.mats + 1, mo); m2 = ldg_at(P.mats + 2, mo); m3 = ldg_at(P.mats + 3, mo);
    }
    else { m0 = ldg4(mp); m1 = ldg4(mp + 1); m2 = ldg4(mp + 2); m3 = ldg4(mp + 3); }
    const float4 notex = make_float4(__int_as_float(-1), __int_as_float(-1), __int_as_float(-1), __int_as_float(-1));
    float4 m4f = PLAIN ? notex : ldg4(mp + 4), m5f = PLAIN ? notex : ldg4(mp + 5);
    float4 sn2 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), sn3 = sn2, sn4 = sn2;
    if (smoothing) { sn2 = ldg4(sp4 + 2); sn3 = ldg4(sp4 + 3); sn4 = ldg4(sp4 + 4); }
    // PLAIN, exact build: the hemisphere sampler's frames about the triangle's two possible normals ride in the same batch (the
    // table fill_flat_frames_kernel computed with the same operations); asked for by index after the flip test instead - two
    // loads, not four - they cost the block a memory round trip of its own and half of the gain
    FlatFrames<PLAIN && !PTK_CONTRACT> frames;
    if constexpr (PLAIN && !PTK_CONTRACT)
    {
        if constexpr (OFF32)
        {
            const float4* ft = P.flat_tris + FLAT_FRAMES_AT;
            const uint32_t fo = (uint32_t)h.tri * (uint32_t)(FLAT_FRAME_F4 * 16);
            frames.u0 = ldg_at(ft, fo); frames.v0 = ldg_at(ft + 1, fo); frames.u1 = ldg_at(ft + 2, fo); frames.v1 = ldg_at(ft + 3, fo);
        }
        else
        {
            const float4* fp = P.flat_tris + FLAT_FRAMES_AT + h.tri * FLAT_FRAME_F4;
            frames.u0 = ldg4(fp); frames.v0 = ldg4(fp + 1); frames.u1 = ldg4(fp + 2); frames.v1 = ldg4(fp + 3);
        }
    }
    asm volatile("" ::: "memory");
    int tex_diffuse = __float_as_int(m4f.x), tex_normal = __float_as_int(m4f.y);
    int tex_emiss = __float_as_int(m4f.z), tex_rough = __float_as_int(m4f.w);
    int tex_metal = __float_as_int(m5f.x);
    bool any_tex = !PLAIN && __float_as_int(m5f.z) != 0;

    v3 p = add(ro, muls(rd, h.t));                  // :553
    float uvx = 0.0f, uvy = 0.0f;
    if (any_tex)
    {
        float4 s1 = ldg4(sp4 + 1), s2 = ldg4(sp4 + 2);
        float w = 1.0f - h.u - h.v;                 // GetUV :533-536
        uvx = w * s1.x + h.u * s1.z + h.v * s2.x;
        uvy = w * s1.y + h.u * s1.w + h.v * s2.y;
    }
    v3 n = V(s0.x, s0.y, s0.z);
    if (smoothing)                                  // :556, GetSmoothNormal :538-543
    {
        const float4 s2 = sn2, s3 = sn3, s4 = sn4;
        float w = 1.0f - h.u - h.v;
        v3 n1 = V(s2.z, s2.w, s3.x), n2 = V(s3.y, s3.z, s3.w), n3 = V(s4.x, s4.y, s4.z);
        v3 sn = add(add(muls(n1, w), muls(n2, h.u)), muls(n3, h.v));
        n = normalize(sn);
    }
    if (tex_normal >= 0)                            // :558-566
    {
        float4 s4 = ldg4(sp4 + 4), s5 = ldg4(sp4 + 5), s6 = ldg4(sp4 + 6);
        float4 c = tex2d(P, tex_normal, uvx, uvy);
        if (STATS) cnt.tex++;
        v3 nt = V(c.x * 2.0f - 1.0f, c.y * 2.0f - 1.0f, c.z * 2.0f - 1.0f);
        if (nt.z <= 0.0f) nt = V(nt.x, nt.y, PTK_EPS);
        nt = normalize(nt);
        v3 tg = V(s4.w, s5.x, s5.y), bt = V(s5.z, s5.w, s6.x);
        v3 m = V(tg.x * nt.x + bt.x * nt.y + n.x * nt.z,
                 tg.y * nt.x + bt.y * nt.y + n.y * nt.z,
                 tg.z * nt.x + bt.z * nt.y + n.z * nt.z);
        n = normalize(m);
    }
    v3 frame_u = V(0.0f, 0.0f, 0.0f), frame_v = frame_u;
    if constexpr (PLAIN && !PTK_CONTRACT)           // n becomes one of the triangle's two possible normals: its frame
    {
        const bool flip = dot(n, rd) > 0.0f;
        frame_u = V(flip ? frames.u1.x : frames.u0.x, flip ? frames.u1.y : frames.u0.y, flip ? frames.u1.z : frames.u0.z);
        frame_v = V(flip ? frames.v1.x : frames.v0.x, flip ? frames.v1.y : frames.v0.y, flip ? frames.v1.z : frames.v0.z);
    }
    if (dot(n, rd) > 0.0f) n = neg(n);              // :567-568
    p = add(p, muls(n, PTK_EPS));                   // :569

    static_assert(PLAIN || !LAMBERT, "LAMBERT is a level of the PLAIN kernel");
    bool ended = false;
    if (!((LAMBERT ? depth : iter) < P.max_depth)) ended = true;        // :571 terminal bounce: no emission
    else
    {
        v3 diffuse = V(m0.x, m0.y, m0.z);
        if (tex_diffuse >= 0) { float4 c = tex2d(P, tex_diffuse, uvx, uvy); diffuse = V(c.x, c.y, c.z); if (STATS) cnt.tex++; }
        v3 emiss = V(m2.x, m2.y, m2.z);
        if (tex_emiss >= 0) { float4 c = tex2d(P, tex_emiss, uvx, uvy); emiss = V(c.x, c.y, c.z); if (STATS) cnt.tex++; }
        float roughness = m2.w;
        if (tex_rough >= 0) { roughness = tex2d_r(P, tex_rough, uvx, uvy); if (STATS) cnt.tex++; }
        float reflectiveness = m3.x;
        if (tex_metal >= 0) { reflectiveness = tex2d_r(P, tex_metal, uvx, uvy); if (STATS) cnt.tex++; }
        const int mtype = PLAIN ? 0 : __float_as_int(m0.w);
        const v3 specular = V(m1.x, m1.y, m1.z);
        const float emissI = m1.w;

        depth++;                                    // :586-587
        if (!LAMBERT) iter++;
        const float prob = m3.w;                    // min(0.95, max(diffuse)) of the constant colour
        if (depth >= P.max_depth)
        {
            if (fabsf(rng.next()) > prob) ended = true;     // :590-594, no 1/prob compensation
        }
        if (!ended)
        {
            const v3 r = LAMBERT ? rd : reflect(rd, n);     // :596 (read by the mirror and lobe samplers only)
            v3 dir;
            v3 weight;
            bool diffuse_bounce = false;
            // the reference spells the same three-way roughness sampler out three times
            // (:603-624, :679-700) and the hemisphere sampler twice more (:631-636, :717-722);
            // here the branch only picks the sampler's arguments and ONE call does the work
            int sampler = 0;                        // 0: mirror direction r, 1: hemisphere about n, 2: lobe about r
            if (LAMBERT)
            {
                rng.state = rng.state * 747796405u + rng.inc;      // :601's draw, whose comparison is false whatever it gives
                sampler = 1;                        // :631-636
                diffuse_bounce = true;
                weight = diffuse;                   // :638
            }
            else if (mtype == 0)
            {
                if (rng.next() < reflectiveness)    // :601
                {
                    sampler = roughness == 1.0f ? 1 : (roughness == 0.0f ? 0 : 2);
                    iter--;
                    weight = specular;              // :626
                }
                else
                {
                    sampler = 1;                    // :631-636
                    diffuse_bounce = true;
                    weight = diffuse;               // :638
                }
            }
            else
            {
                bool refract = false;
                v3 refractN = n;
                if (roughness != 0.0f)              // :645-654
                {
                    float w = rng.next() * roughness, th = rng.next();
                    refractN = sample_about(n, 1.0f - PTK_FLT_EPSILON, r, n, w, th);
                }
                float nc = 1.0f, ng = m3.z;
                float eta = inside ? ng / nc : nc / ng;     // :658
                float r0 = (nc - ng) / (nc + ng);
                r0 = r0 * r0;
                float c = fabsf(dot(rd, refractN));
                float k = 1.0f - eta * eta * (1.0f - c * c);
                if (k < 0.0f) refract = false;
                else
                {
                    float re = r0 + (1.0f - r0) * (1.0f - c) * (1.0f - c);    // :668
                    if (fabsf(rng.next()) < re) refract = false;
                    else if (rng.next() < reflectiveness) refract = false;
                    else refract = true;
                }
                if (!refract)
                {
                    sampler = roughness == 1.0f ? 1 : (roughness == 0.0f ? 0 : 2);
                    iter--;
                    weight = specular;              // :702
                }
                else if (rng.next() < m3.y)         // :706 translucency
                {
                    float a = eta * dot(n, rd) + sqrt_ieee(k);
                    dir = normalize(sub(muls(rd, eta), muls(refractN, a)));   // :708
                    p = sub(p, muls(muls(n, PTK_EPS), 2.0f));                  // :709
                    inside = !inside;
                    iter--;
                    weight = diffuse;               // :712
                    sampler = 3;                    // direction already set
                }
                else
                {
                    sampler = 1;                    // :717-722
                    diffuse_bounce = true;
                    weight = diffuse;               // :724
                }
            }
            if (sampler == 0) dir = r;
            else if (sampler != 3)
            {
                const bool lobe = sampler == 2;
                float w = rng.next();
                if (lobe) w = w * roughness;
                float th = rng.next();
                if constexpr (PLAIN && !PTK_CONTRACT)
                {
                    v3 u = frame_u, v = frame_v;
                    if (lobe) sample_basis(n, 1.0f - PTK_FLT_EPSILON, r, u, v);
                    dir = sample_in_basis(u, v, lobe ? r : n, w, th);
                }
                else
                    dir = sample_about(n, lobe ? 1.0f - PTK_FLT_EPSILON : 1.0f - PTK_EPS, lobe ? r : n, lobe ? r : n, w, th);
            }

            L = add(L, mulv(T, muls(emiss, emissI)));      // emiss * emissiveIntensity term
            v3 next_ro = p, next_rd = dir;
            float4 lt0 = make_float4(0.0f, 0.0f, 0.0f, 0.0f), lt1 = lt0, lt2 = lt0;
            if (diffuse_bounce && P.num_lights > 0)
            {
                // DirectIllumimation + SampleTriangle, pathtracer.cpp:494-531
                const float u_light = rng.next(), u_su = rng.next(), u_sv = rng.next();
                v3 l, di;
                int light_tri;
                if (sample_direct_light(P, p, n, diffuse, u_light, u_su, u_sv, l, di, light_tri, lt0, lt1, lt2))
                {
                    Tdi = mulv(T, di);
                    if (FLAT)
                    {
                        // the shadow ray rides along with the bounce ray in the next flat pass, which finds its
                        // closest hit over ALL triangles (no early end: the pass runs for the bounce ray anyway)
                        WS.begin(p, l, P.num_nodes, stack, P.scene_bound);
                        WS.occl_tri = light_tri;
                    }
                    else
                    {
                        W.occl_tri = light_tri;
                        nextDir = dir;
                        next_rd = l;
                    }
                }
            }
            T = mulv(T, weight);
            W.begin(next_ro, next_rd, P.num_nodes, stack, P.scene_bound);
            // a shadow ray meets its light triangle before anything else (see Walk::occl_tri)
            if (!FLAT && W.occl_tri >= 0) (void)tri_test<STATS>(P, W, lt0, lt1, lt2, rng, ray, cnt);
        }
    }
    return ended;
}

// ---- owned tiles -> pixels ------------------------------------------------------------------------------------------------
// Tile column and row of tile index `tile` (rank r of `world` owns tiles r, r + world, ...): rows are rotated by 3 tiles each so
// that a rank's tiles form diagonals, not columns (load balance).  Also what the host's loops over owned tiles use (ptk_api.hip).
__host__ __device__ __forceinline__ void tile_origin(int tile, int tiles_x, int& tx, int& ty)
{
    ty = tile / tiles_x; tx = (tile % tiles_x + tiles_x - (3 * ty) % tiles_x) % tiles_x;
}
// the pixel of `lane` of the wave that holds 8x8 quadrant `quad` of tile (tx, ty): one wave per quadrant, rows of eight lanes
__device__ __forceinline__ void quadrant_pixel(int tx, int ty, int quad, int lane, int& px, int& py)
{
    px = tx * PTK_TILE + (quad & 1) * 8 + (lane & 7);
    py = ty * PTK_TILE + (quad >> 1) * 8 + (lane >> 3);
}

// one channel of the 8-bit resolve (pathtracer.cpp:802-812): clamped to [0, 1], NaN to 0, x * 255 truncated
__device__ __forceinline__ uint8_t resolve8(float x)
{
    x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);
    if (!(x == x)) x = 0.0f;
    return (uint8_t)(x * 255);
}

#if PTK_CONTRACT
}  // namespace fma / fast
#endif
}  // namespace ptk
