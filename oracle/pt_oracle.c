/* TEST INFRASTRUCTURE ONLY — see pt_oracle.h.  Plain C99 restatement of the reference's render loop.
 * Every function cites the reference file:line it follows (paths relative to
 * /root/reference/PathTracing/src/).  Compile with -ffp-contract=off and WITHOUT -ffast-math: the
 * float expression order below is the parity contract with the HIP kernel. */
#include "pt_oracle.h"

#include <math.h>
#include <stdlib.h>
#include <string.h>
#ifdef _OPENMP
#include <omp.h>
#endif

#define ORC_EPS 0.00001f           /* mesh.h:12 */
#define ORC_PI_D 3.14159265358979323846
#define ORC_FLT_EPSILON 1.1920928955078125e-7f
#define ORC_TILE 16

typedef struct { float x, y, z; } v3;

static inline v3 V(float x, float y, float z) { v3 r = { x, y, z }; return r; }
static inline v3 ld3(const float* p) { return V(p[0], p[1], p[2]); }
static inline v3 add(v3 a, v3 b) { return V(a.x + b.x, a.y + b.y, a.z + b.z); }
static inline v3 sub(v3 a, v3 b) { return V(a.x - b.x, a.y - b.y, a.z - b.z); }
static inline v3 mulv(v3 a, v3 b) { return V(a.x * b.x, a.y * b.y, a.z * b.z); }
static inline v3 muls(v3 a, float s) { return V(a.x * s, a.y * s, a.z * s); }
static inline v3 neg(v3 a) { return V(-a.x, -a.y, -a.z); }
/* glm 0.9.3.1 core/func_geometric.inl:161-171 */
static inline float dot(v3 a, v3 b) { return a.x * b.x + a.y * b.y + a.z * b.z; }
/* glm core/func_geometric.inl:200-211 */
static inline v3 cross(v3 x, v3 y)
{
    return V(x.y * y.z - y.y * x.z, x.z * y.x - y.z * x.x, x.x * y.y - y.x * x.y);
}
/* glm normalize = x * inversesqrt(dot(x,x)), inversesqrt = 1/sqrt (func_geometric.inl:239-248,
 * func_exponential.inl:145-153) */
static inline v3 normalize(v3 a)
{
    float sqr = a.x * a.x + a.y * a.y + a.z * a.z;
    float inv = 1.0f / sqrtf(sqr);
    return muls(a, inv);
}
/* glm reflect = I - N * dot(N, I) * 2 (func_geometric.inl:276-283) */
static inline v3 reflect(v3 I, v3 N)
{
    float d = dot(N, I);
    return sub(I, muls(muls(N, d), 2.0f));
}

/* ---- sin/cos on [0, 2*pi] -------------------------------------------------------------------
 * Replaces libm cosf/sinf (pathtracer.cpp:610, :738) by a fixed polynomial so that CPU and GPU
 * agree bit for bit.  Reduction in double, cephes single-precision kernels on [-pi/4, pi/4]. */
#ifdef ORC_LIBM_SINCOS
/* (tools/fuzz_trace_vs_reference.py --libm: libm's own sinf / cosf, as the reference calls them - with these the recursion below
 * reproduces the reference's radiance BIT FOR BIT; the polynomial is what the product computes with, DESIGN.md section 2, difference 6) */
void orc_sincos(float a, float* s, float* c) { *s = sinf(a); *c = cosf(a); }
#else
void orc_sincos(float a, float* s, float* c)
{
    int k = (int)(a * 0.636619772367581343f + 0.5f);
    float r = (float)((double)a - (double)k * 1.57079632679489661923);
    float z = r * r;
    float sp = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
    float cp = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z
               - 0.5f * z + 1.0f;
    switch (k & 3)
    {
    case 0: *s = sp; *c = cp; break;
    case 1: *s = cp; *c = -sp; break;
    case 2: *s = -sp; *c = -cp; break;
    default: *s = -cp; *c = sp; break;
    }
}
#endif

/* orc_sincos on n angles (the exhaustive tests pass 2^24 of them) */
void orc_sincos_n(const float* a, int n, float* s, float* c)
{
    for (int i = 0; i < n; ++i) orc_sincos(a[i], &s[i], &c[i]);
}

/* ---- RNG -------------------------------------------------------------------------------------
 * Replaces PathTracer::Rand (pathtracer.cpp:367-371; one std::mt19937 raced by all workers) by a
 * counter-based PCG-RXS-M-XS-32 stream per (seed, pixel, sample).  Tape mode replays recorded
 * reference draws. */
static inline uint32_t pcg_out(uint32_t st)
{
    uint32_t w = ((st >> ((st >> 28u) + 4u)) ^ st) * 277803737u;
    return (w >> 22u) ^ w;
}
static inline uint32_t hash32(uint32_t x) { return pcg_out(x * 747796405u + 2891336453u); }

typedef struct {
    uint32_t state, inc, key;      /* counter mode */
    const float* tape; int tape_len, tape_pos;   /* tape mode when tape != NULL */
} rng_t;

static inline uint32_t pixel_key(uint64_t seed, uint32_t pixel)
{
    uint32_t a = hash32((uint32_t)(seed >> 32));
    uint32_t b = hash32((uint32_t)seed + a);
    return hash32(pixel + b);
}
static inline void rng_init(rng_t* r, uint32_t pkey, uint32_t sample)
{
    r->state = hash32(sample + pkey);
    r->inc = (hash32(pkey ^ 0x9E3779B9u) << 1) | 1u;
    r->key = r->state;
    r->tape = 0; r->tape_len = 0; r->tape_pos = 0;
}
static inline float u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }
static inline float rnd(rng_t* r)
{
    if (r->tape)
    {
        float v = r->tape_pos < r->tape_len ? r->tape[r->tape_pos] : 0.5f;
        r->tape_pos++;
        return v;
    }
    uint32_t old = r->state;
    r->state = old * 747796405u + r->inc;
    return u01(pcg_out(old));
}
/* independent draw for the stochastic-opacity test of triangle `tri` on ray number `ray` of this
 * path: order-independent replacement for the Rand() at pathtracer.cpp:475 */
static inline float rnd_opacity(rng_t* r, uint32_t ray, uint32_t tri)
{
    if (r->tape) return rnd(r);
    return u01(hash32(tri + hash32(ray + r->key)));
}
float orc_rand_u01(uint64_t seed, uint32_t pixel, uint32_t sample, int n)
{
    rng_t r; float v = 0.0f;
    rng_init(&r, pixel_key(seed, pixel), sample);
    for (int i = 0; i <= n; i++) v = rnd(&r);
    return v;
}

/* ---- scene ------------------------------------------------------------------------------------*/
typedef struct { float bmin[3], bmax[3]; int32_t left, right, first, count; } node_t;

struct orc_scene {
    int32_t nt;
    float *verts, *normals, *uvs, *tbn;
    uint8_t* smoothing;
    int32_t* material;
    int32_t nm; orc_material* mats;
    int32_t ntex; orc_texture* tex; uint8_t* texels; int64_t texel_bytes;
    int32_t nl; int32_t* lights;
    /* own BVH */
    node_t* nodes; int32_t nnodes, cap; int32_t* order; int32_t depth;
};

static void* dup(const void* p, size_t n)
{
    void* q = malloc(n ? n : 1);
    if (n && p) memcpy(q, p, n);
    return q;
}

/* ---- Moeller-Trumbore, PathTracer::IntersectTriangle pathtracer.cpp:373-409 -----------------*/
static inline int intersect_triangle(v3 ro, v3 rd, v3 v0, v3 v1, v3 v2, float* t, float* u, float* v)
{
    v3 edge1 = sub(v1, v0);
    v3 edge2 = sub(v2, v0);
    v3 h = cross(rd, edge2);
    float a = dot(edge1, h);
    if (fabsf(a) < ORC_EPS) return 0;
    float f = 1.0f / a;
    v3 s = sub(ro, v0);
    float uu = f * dot(s, h);
    if (uu < 0.0f || uu > 1.0f) return 0;
    v3 q = cross(s, edge1);
    float vv = f * dot(rd, q);
    if (vv < 0.0f || uu + vv > 1.0f) return 0;
    float tt = f * dot(edge2, q);
    if (tt > ORC_EPS) { *t = tt; *u = uu; *v = vv; return 1; }
    return 0;
}
void orc_intersect_triangle(const float* ro, const float* rd, const float* v0, const float* v1,
                            const float* v2, float* out3)
{
    float t, u, v;
    if (intersect_triangle(ld3(ro), ld3(rd), ld3(v0), ld3(v1), ld3(v2), &t, &u, &v)) { out3[0] = t; out3[1] = u; out3[2] = v; }
    else out3[0] = out3[1] = out3[2] = 0.0f;
}

/* ---- census (test infrastructure: orc_render_census) ---------------------------------------------
 * Every function below that decides something takes `cz`, the census' counters (ORC_ARM_N of them) or NULL.  The functions
 * orc_render, trace and the probes call are thin wrappers that pass a literal NULL into the always-inlined body, so the
 * compiler drops every ARM() from them: their code is what it was without the census. */
#define ORC_INLINE static inline __attribute__((always_inline))
#define ARM(cz, id) do { if (cz) (cz)[id]++; } while (0)

/* ---- Image::tex2D image.cpp:63-86 -----------------------------------------------------------*/
ORC_INLINE void tex2d_impl(const orc_scene* s, int tex, float uvx, float uvy, float* out4, int64_t* cz, int slot)
{
    if (tex < 0 || tex >= s->ntex || s->tex[tex].width <= 0 || s->tex[tex].height <= 0)
    { ARM(cz, ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_MISSING); out4[0] = out4[1] = out4[2] = out4[3] = 0.0f; return; }
    const orc_texture* T = &s->tex[tex];
    float u = fmodf(uvx, 1.0f);
    float v = fmodf(uvy, 1.0f);
    if (u < 0.0f) u += 1.0f;
    if (v < 0.0f) v += 1.0f;
    int cx = (int)((float)T->width * u);
    int cy = (int)((float)T->height * v);
    if (cz)
    {
        int64_t* a = cz + ORC_ARM_TEX + slot * ORC_TEX_ARMS;
        const int hx = cx > T->width - 1, hy = cy > T->height - 1, lx = cx < 0, ly = cy < 0;
        a[ORC_TEX_HI_X] += hx; a[ORC_TEX_HI_Y] += hy; a[ORC_TEX_LO_X] += lx; a[ORC_TEX_LO_Y] += ly;
        a[ORC_TEX_PLAIN] += !(hx | hy | lx | ly);
    }
    if (cx > T->width - 1) cx = T->width - 1;     /* clamp: see header (reference over-reads) */
    if (cy > T->height - 1) cy = T->height - 1;
    if (cx < 0) cx = 0;                            /* NaN uv */
    if (cy < 0) cy = 0;
    const uint8_t* p = s->texels + T->offset + 4 * ((int64_t)cy * T->width + cx);
    out4[0] = (float)p[0] / 255.0f;
    out4[1] = (float)p[1] / 255.0f;
    out4[2] = (float)p[2] / 255.0f;
    out4[3] = (float)p[3] / 255.0f;
}
static inline void tex2d(const orc_scene* s, int tex, float uvx, float uvy, float* out4) { tex2d_impl(s, tex, uvx, uvy, out4, NULL, 0); }
void orc_tex2d(const orc_scene* s, int tex, float u, float v, float* out4) { tex2d(s, tex, u, v, out4); }

/* PathTracer::GetUV pathtracer.cpp:533-536 */
static inline void get_uv(const orc_scene* s, int tri, float cx, float cy, float* ux, float* uy)
{
    const float* uv = s->uvs + (size_t)tri * 6;
    float w = 1.0f - cx - cy;
    *ux = w * uv[0] + cx * uv[2] + cy * uv[4];
    *uy = w * uv[1] + cx * uv[3] + cy * uv[5];
}

/* ---- Triangle::Init mesh.cpp:61-83 ------------------------------------------------------------*/
void orc_triangle_init(const float* in, float* out9)
{
    v3 v1 = ld3(in), v2 = ld3(in + 3), v3_ = ld3(in + 6);
    v3 e1 = sub(v2, v1), e2 = sub(v3_, v1);
    float d1x = in[11] - in[9], d1y = in[12] - in[10];
    float d2x = in[13] - in[9], d2y = in[14] - in[10];
    float f = 1.0f / (d1x * d2y - d2x * d1y);
    v3 tangent = V(f * (d2y * e1.x - d1y * e2.x), f * (d2y * e1.y - d1y * e2.y), f * (d2y * e1.z - d1y * e2.z));
    v3 bitangent = V(f * (-d2x * e1.x + d1x * e2.x), f * (-d2x * e1.y + d1x * e2.y), f * (-d2x * e1.z + d1x * e2.z));
    v3 normal = cross(e1, e2);
    tangent = normalize(tangent);
    bitangent = normalize(bitangent);
    normal = normalize(normal);
    out9[0] = normal.x; out9[1] = normal.y; out9[2] = normal.z;
    out9[3] = tangent.x; out9[4] = tangent.y; out9[5] = tangent.z;
    out9[6] = bitangent.x; out9[7] = bitangent.y; out9[8] = bitangent.z;
}

/* ---- own BVH (acceleration only; closest hit is tree-independent) ------------
 * The reference builds a random-axis median-split pointer tree (mesh.cpp:169-211) and walks both
 * children unconditionally (pathtracer.cpp:411-492).  Here: longest-axis object-median split,
 * leaves <= 2 triangles, boxes padded so culling is conservative, ordered traversal with t-max. */
static void tri_bounds(const orc_scene* s, int tri, float* mn, float* mx)
{
    const float* p = s->verts + (size_t)tri * 9;
    for (int a = 0; a < 3; a++)
    {
        float lo = p[a], hi = p[a];
        for (int k = 1; k < 3; k++) { float x = p[k * 3 + a]; if (x < lo) lo = x; if (x > hi) hi = x; }
        mn[a] = lo; mx[a] = hi;
    }
}
typedef struct { const orc_scene* s; int axis; } cmp_ctx;
static cmp_ctx g_cmp;   /* build is single-threaded */
static int cmp_centroid(const void* a, const void* b)
{
    int ia = *(const int32_t*)a, ib = *(const int32_t*)b;
    const float* pa = g_cmp.s->verts + (size_t)ia * 9 + g_cmp.axis;
    const float* pb = g_cmp.s->verts + (size_t)ib * 9 + g_cmp.axis;
    float ca = pa[0] + pa[3] + pa[6], cb = pb[0] + pb[3] + pb[6];
    if (ca < cb) return -1;
    if (ca > cb) return 1;
    return ia < ib ? -1 : (ia > ib ? 1 : 0);
}
static int32_t build(orc_scene* s, int first, int count, int depth, float pad)
{
    int32_t id = s->nnodes++;
    node_t* n = &s->nodes[id];
    float mn[3] = { INFINITY, INFINITY, INFINITY }, mx[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (int i = 0; i < count; i++)
    {
        float a[3], b[3];
        tri_bounds(s, s->order[first + i], a, b);
        for (int k = 0; k < 3; k++) { if (a[k] < mn[k]) mn[k] = a[k]; if (b[k] > mx[k]) mx[k] = b[k]; }
    }
    for (int k = 0; k < 3; k++) { n->bmin[k] = mn[k] - pad; n->bmax[k] = mx[k] + pad; }
    if (depth > s->depth) s->depth = depth;
    if (count <= 2) { n->left = n->right = -1; n->first = first; n->count = count; return id; }
    int axis = 0;
    float e0 = mx[0] - mn[0], e1 = mx[1] - mn[1], e2 = mx[2] - mn[2];
    if (e1 > e0 && e1 >= e2) axis = 1; else if (e2 > e0 && e2 > e1) axis = 2;
    g_cmp.s = s; g_cmp.axis = axis;
    qsort(s->order + first, (size_t)count, sizeof(int32_t), cmp_centroid);
    int half = count / 2;
    n->first = 0; n->count = 0;
    int32_t l = build(s, first, half, depth + 1, pad);
    int32_t r = build(s, first + half, count - half, depth + 1, pad);
    n = &s->nodes[id];
    n->left = l; n->right = r;
    return id;
}

orc_scene* orc_create(const orc_scene_desc* d)
{
    orc_scene* s = (orc_scene*)calloc(1, sizeof(orc_scene));
    s->nt = d->num_triangles;
    size_t n = (size_t)s->nt;
    s->verts = (float*)dup(d->verts, n * 9 * sizeof(float));
    s->normals = (float*)dup(d->normals, n * 9 * sizeof(float));
    s->uvs = (float*)dup(d->uvs, n * 6 * sizeof(float));
    s->tbn = (float*)dup(d->tbn, n * 9 * sizeof(float));
    s->smoothing = (uint8_t*)dup(d->smoothing, n);
    s->material = (int32_t*)dup(d->material, n * sizeof(int32_t));
    s->nm = d->num_materials;
    s->mats = (orc_material*)dup(d->materials, (size_t)s->nm * sizeof(orc_material));
    s->ntex = d->num_textures;
    s->tex = (orc_texture*)dup(d->textures, (size_t)s->ntex * sizeof(orc_texture));
    s->texel_bytes = d->texel_bytes;
    s->texels = (uint8_t*)dup(d->texels, (size_t)d->texel_bytes);
    s->nl = d->num_lights;
    s->lights = (int32_t*)dup(d->lights, (size_t)s->nl * sizeof(int32_t));
    s->cap = (int32_t)(2 * n + 2);
    s->nodes = (node_t*)calloc((size_t)s->cap, sizeof(node_t));
    s->order = (int32_t*)malloc((n ? n : 1) * sizeof(int32_t));
    for (size_t i = 0; i < n; i++) s->order[i] = (int32_t)i;
    float ext = 1.0f;
    for (size_t i = 0; i < n * 9; i++) { float a = fabsf(s->verts[i]); if (a > ext) ext = a; }
    if (n > 0) build(s, 0, (int)n, 1, 1e-5f * ext);
    return s;
}
void orc_destroy(orc_scene* s)
{
    if (!s) return;
    free(s->verts); free(s->normals); free(s->uvs); free(s->tbn); free(s->smoothing); free(s->material);
    free(s->mats); free(s->tex); free(s->texels); free(s->lights); free(s->nodes); free(s->order);
    free(s);
}
void orc_bvh_info(const orc_scene* s, int32_t* nodes, int32_t* depth) { *nodes = s->nnodes; *depth = s->depth; }

typedef struct { int32_t tri; float t, u, v; } hit_t;

/* candidate test of one triangle: Hit leaf branch, pathtracer.cpp:463-489 */
/* returns 1 when it looked up an opacity texel (the candidate hits and is nearer than the best so far), for the counting
 * render below; the others ignore it */
ORC_INLINE int test_triangle_impl(const orc_scene* s, int tri, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* best, int64_t* cz)
{
    const float* p = s->verts + (size_t)tri * 9;
    float t, u, v;
    if (!intersect_triangle(ro, rd, ld3(p), ld3(p + 3), ld3(p + 6), &t, &u, &v)) return 0;
    /* (an infinite t - an overflowed determinant of a ray far outside every scene - is no hit: with best->t starting at
       infinity the tie rule would otherwise accept it; the kernels test the same) */
    if (cz && t < INFINITY)
        ARM(cz, t < best->t ? ORC_ARM_TRI_NEARER : (t == best->t ? (tri < best->tri ? ORC_ARM_TRI_TIE_ACCEPTED : ORC_ARM_TRI_TIE_REJECTED)
                                                                 : ORC_ARM_TRI_FARTHER));
    if (!(t < INFINITY) || !(t < best->t || (t == best->t && tri < best->tri))) return 0;
    int otex = s->mats[s->material[tri]].tex[5];
    if (otex >= 0)
    {
        float ux, uy, c[4];
        get_uv(s, tri, u, v, &ux, &uy);
        tex2d_impl(s, otex, ux, uy, c, cz, 5);
        if (!(rnd_opacity(rng, ray, (uint32_t)tri) < c[0])) { ARM(cz, ORC_ARM_TRI_OPACITY_DROPPED); return 1; }
        ARM(cz, ORC_ARM_TRI_OPACITY_KEPT);
    }
    best->tri = tri; best->t = t; best->u = u; best->v = v;
    return otex >= 0;
}
static inline int test_triangle(const orc_scene* s, int tri, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* best)
{
    return test_triangle_impl(s, tri, ro, rd, rng, ray, best, NULL);
}

ORC_INLINE int closest_hit_impl(const orc_scene* s, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* out, int64_t* cz)
{
    hit_t best; best.tri = 0x7fffffff; best.t = INFINITY; best.u = best.v = 0.0f;
    if (s->nt == 0) return 0;
    v3 inv = V(1.0f / rd.x, 1.0f / rd.y, 1.0f / rd.z);
    int32_t stack[128]; int sp = 0;
    stack[sp++] = 0;
    while (sp)
    {
        const node_t* n = &s->nodes[stack[--sp]];
        float t0x = (n->bmin[0] - ro.x) * inv.x, t1x = (n->bmax[0] - ro.x) * inv.x;
        float t0y = (n->bmin[1] - ro.y) * inv.y, t1y = (n->bmax[1] - ro.y) * inv.y;
        float t0z = (n->bmin[2] - ro.z) * inv.z, t1z = (n->bmax[2] - ro.z) * inv.z;
        float tn = fmaxf(fmaxf(fminf(t0x, t1x), fminf(t0y, t1y)), fminf(t0z, t1z));
        float tf = fminf(fminf(fmaxf(t0x, t1x), fmaxf(t0y, t1y)), fmaxf(t0z, t1z));
        if (!(tn <= tf * 1.0000004f) || tf < 0.0f || tn > best.t) continue;
        if (n->left < 0)
        {
            for (int i = 0; i < n->count; i++) test_triangle_impl(s, s->order[n->first + i], ro, rd, rng, ray, &best, cz);
        }
        else if (sp + 2 <= 128)
        {
            stack[sp++] = n->right;
            stack[sp++] = n->left;
        }
        else ARM(cz, ORC_ARM_WALK_STACK_FULL);
    }
    if (best.tri == 0x7fffffff) return 0;
    *out = best;
    return 1;
}
static int closest_hit(const orc_scene* s, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* out)
{
    return closest_hit_impl(s, ro, rd, rng, ray, out, NULL);
}
/* the census' closest hit: the tree walk above, or (brute) the candidates in ascending index order, the FLAT pass's */
static int closest_hit_census(const orc_scene* s, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* out, int64_t* cz, int brute)
{
    if (!brute) return closest_hit_impl(s, ro, rd, rng, ray, out, cz);
    hit_t best; best.tri = 0x7fffffff; best.t = INFINITY; best.u = best.v = 0.0f;
    for (int i = 0; i < s->nt; i++) test_triangle_impl(s, i, ro, rd, rng, ray, &best, cz);
    if (best.tri == 0x7fffffff) return 0;
    *out = best;
    return 1;
}
static int closest_hit_brute(const orc_scene* s, v3 ro, v3 rd, rng_t* rng, uint32_t ray, hit_t* out)
{
    hit_t best; best.tri = 0x7fffffff; best.t = INFINITY; best.u = best.v = 0.0f;
    for (int i = 0; i < s->nt; i++) test_triangle(s, i, ro, rd, rng, ray, &best);
    if (best.tri == 0x7fffffff) return 0;
    *out = best;
    return 1;
}
int orc_hit(const orc_scene* s, const float* ro, const float* rd, float* tuv, int32_t* tri)
{
    rng_t r; rng_init(&r, 0, 0); hit_t h;
    if (!closest_hit(s, ld3(ro), ld3(rd), &r, 0, &h)) { *tri = -1; tuv[0] = tuv[1] = tuv[2] = 0.0f; return 0; }
    *tri = h.tri; tuv[0] = h.t; tuv[1] = h.u; tuv[2] = h.v; return 1;
}
int orc_hit_brute(const orc_scene* s, const float* ro, const float* rd, float* tuv, int32_t* tri)
{
    rng_t r; rng_init(&r, 0, 0); hit_t h;
    if (!closest_hit_brute(s, ld3(ro), ld3(rd), &r, 0, &h)) { *tri = -1; tuv[0] = tuv[1] = tuv[2] = 0.0f; return 0; }
    *tri = h.tri; tuv[0] = h.t; tuv[1] = h.u; tuv[2] = h.v; return 1;
}

/* ---- counting (test infrastructure for the trace kernels' counters, include/ptk.h ptk_stats) ----------------------------
 * orc_render_counted traces exactly what orc_render traces and counts, per pixel, what the kernels' STATS build counts. */
typedef struct {
    int64_t* px;          /* this pixel's ORC_CNT_N counters */
    orc_ray_rec* rec;     /* where this pixel's next ray record goes; NULL: no dump */
    orc_ray_rec* rec_end;
    int overflow;
    uint32_t pixel, sample;
    int brute;            /* the scene has opacity textures: candidates in ascending index order, the FLAT pass's */
} count_t;

static int closest_hit_counted(const orc_scene* s, v3 ro, v3 rd, rng_t* rng, uint32_t ray, int kind, int light, count_t* cc,
                               hit_t* out)
{
    int hit;
    cc->px[ORC_CNT_CAMERA + kind]++;
    if (cc->brute)
    {
        /* closest_hit_brute, counting the opacity texels its candidate order reads (its closest hit is the tree walk's) */
        hit_t best; best.tri = 0x7fffffff; best.t = INFINITY; best.u = best.v = 0.0f;
        for (int i = 0; i < s->nt; i++) cc->px[ORC_CNT_TEX_OPACITY] += test_triangle(s, i, ro, rd, rng, ray, &best);
        hit = best.tri != 0x7fffffff;
        if (hit) *out = best;
    }
    else hit = closest_hit(s, ro, rd, rng, ray, out);
    if (cc->rec)
    {
        if (cc->rec < cc->rec_end)
        {
            orc_ray_rec* r = cc->rec++;
            r->pixel = cc->pixel; r->sample = cc->sample; r->ray = ray; r->kind = kind;
            r->ro[0] = ro.x; r->ro[1] = ro.y; r->ro[2] = ro.z; r->rd[0] = rd.x; r->rd[1] = rd.y; r->rd[2] = rd.z;
            r->t = hit ? out->t : INFINITY; r->tri = hit ? out->tri : -1;
            r->light = light; r->occluded = kind == ORC_RAY_SHADOW && hit && out->tri != light;
        }
        else cc->overflow = 1;
    }
    return hit;
}

/* ---- hemisphere / lobe samplers, pathtracer.cpp:606-611 and :618-623 ------------------------------
 * pole: the axis the sample is built around (n or r); basis_from: vector crossed to make u,v
 * (n for the hemisphere form, r for the lobe form); nx_test: |n.x| against thr chooses the helper. */
ORC_INLINE v3 sample_about_impl(v3 n_for_test, float thr, v3 basis_from, v3 pole, float w, float theta, int64_t* cz, int site)
{
    if (cz)
    {
        const float ax = fabsf(n_for_test.x);
        cz[ORC_ARM_SA + site * ORC_SA_CLASSES + (ax < 1.0f - ORC_EPS ? ORC_SA_BELOW : (ax < 1.0f - ORC_FLT_EPSILON ? ORC_SA_BAND : ORC_SA_POLE))]++;
    }
    v3 u = fabsf(n_for_test.x) < thr ? cross(V(1.0f, 0.0f, 0.0f), basis_from) : cross(V(1.0f, 1.0f, 1.0f), basis_from);
    u = normalize(u);
    v3 v = normalize(cross(u, basis_from));
    float ang = (float)(2.0f * ORC_PI_D * theta);       /* 2.0f*M_PI*theta evaluated in double */
    float sn, cs;
    orc_sincos(ang, &sn, &cs);
    v3 d = add(add(muls(u, w * cs), muls(v, w * sn)), muls(pole, sqrtf(1.0f - w * w)));
    return normalize(d);
}

/* PathTracer::SampleTriangle + DirectIllumimation, pathtracer.cpp:494-531 */
ORC_INLINE v3 direct_illumination_impl(const orc_scene* s, v3 p, v3 n, v3 diffuse, rng_t* rng, uint32_t* ray, count_t* cc, int64_t* cz,
                                       int brute)
{
    if (s->nl == 0) { ARM(cz, ORC_ARM_DI_NO_LIGHTS); return V(0.0f, 0.0f, 0.0f); }
    int lightId = (int)floorf(rnd(rng) * (float)s->nl);
    if (lightId == s->nl && lightId > 0) { ARM(cz, ORC_ARM_DI_LIGHT_ID_CLAMPED); lightId--; }
    int ltri = s->lights[lightId];
    const float* lp = s->verts + (size_t)ltri * 9;
    float u = sqrtf(rnd(rng));
    float v = rnd(rng);
    float w0 = 1.0f - u, w1 = u * (1.0f - v), w2 = u * v;
    v3 vLight = add(add(muls(ld3(lp), w0), muls(ld3(lp + 3), w1)), muls(ld3(lp + 6), w2));
    v3 l = normalize(sub(vLight, p));
    float ndl = dot(neg(n), neg(l));
    if (ndl <= 0.0f) { ARM(cz, ORC_ARM_DI_NDL_NOT_POSITIVE); return V(0.0f, 0.0f, 0.0f); }
    hit_t h;
    uint32_t r = (*ray)++;
    if (cz ? closest_hit_census(s, p, l, rng, r, &h, cz, brute)
           : (cc ? closest_hit_counted(s, p, l, rng, r, ORC_RAY_SHADOW, ltri, cc, &h) : closest_hit(s, p, l, rng, r, &h)))
    {
        if (h.tri != ltri) { ARM(cz, ORC_ARM_DI_HIT_OTHER); return V(0.0f, 0.0f, 0.0f); }
        ARM(cz, ORC_ARM_DI_HIT_LIGHT);
    }
    else ARM(cz, ORC_ARM_DI_SHADOW_MISSED);
    const orc_material* lm = &s->mats[s->material[ltri]];
    v3 lColor = muls(ld3(lm->emissive), lm->emissive_intensity);
    return muls(mulv(lColor, diffuse), ndl);
}
static v3 direct_illumination_c(const orc_scene* s, v3 p, v3 n, v3 diffuse, rng_t* rng, uint32_t* ray, count_t* cc)
{
    return direct_illumination_impl(s, p, n, diffuse, rng, ray, cc, NULL, 0);
}
static v3 direct_illumination(const orc_scene* s, v3 p, v3 n, v3 diffuse, rng_t* rng, uint32_t* ray)
{
    return direct_illumination_c(s, p, n, diffuse, rng, ray, NULL);
}

/* One surface interaction of PathTracer::Trace (pathtracer.cpp:551-727): everything between the
 * closest hit and the recursive call.  Returns 0 when the path ends here with no contribution
 * (terminal bounce :571, Russian roulette :590-594). */
typedef struct {
    v3 p, n, dir;        /* offset hit point, shading normal, sampled continuation direction */
    v3 e;                /* emiss * emissiveIntensity */
    v3 weight;           /* factor on the recursive term (specular or diffuse) */
    v3 diffuse;          /* textured diffuse colour (argument of DirectIllumimation) */
    int diffuse_bounce;  /* 1: DirectIllumimation is added (:638, :724) */
} bounce_t;

ORC_INLINE int shade_impl(const orc_scene* s, v3 ro, v3 rd, const hit_t* h, int D, int* depth_io, int* iter_io,
                          int* inside_io, rng_t* rng, bounce_t* b, int64_t* cz)
{
    int depth = *depth_io, iter = *iter_io, inside = *inside_io;
    const orc_material* mat = &s->mats[s->material[h->tri]];
    v3 p = add(ro, muls(rd, h->t));                                       /* :553 */
    float uvx, uvy;
    get_uv(s, h->tri, h->u, h->v, &uvx, &uvy);
    const float* tb = s->tbn + (size_t)h->tri * 9;
    v3 n = ld3(tb);
    ARM(cz, s->smoothing[h->tri] ? ORC_ARM_SMOOTHING_ON : ORC_ARM_SMOOTHING_OFF);
    ARM(cz, mat->tex[1] >= 0 ? ORC_ARM_NORMAL_MAP_ON : ORC_ARM_NORMAL_MAP_OFF);
    if (s->smoothing[h->tri])                                             /* :556, :538-543 */
    {
        const float* nn = s->normals + (size_t)h->tri * 9;
        float w = 1.0f - h->u - h->v;
        v3 sn = add(add(muls(ld3(nn), w), muls(ld3(nn + 3), h->u)), muls(ld3(nn + 6), h->v));
        n = normalize(sn);
    }
    if (mat->tex[1] >= 0)                                                 /* :558-566 */
    {
        float c[4];
        tex2d_impl(s, mat->tex[1], uvx, uvy, c, cz, 1);
        v3 nt = V(c[0] * 2.0f - 1.0f, c[1] * 2.0f - 1.0f, c[2] * 2.0f - 1.0f);
        if (nt.z <= 0.0f) { ARM(cz, ORC_ARM_NT_Z_CLAMPED); nt = V(nt.x, nt.y, ORC_EPS); }
        nt = normalize(nt);
        v3 tg = ld3(tb + 3), bt = ld3(tb + 6);
        v3 m = V(tg.x * nt.x + bt.x * nt.y + n.x * nt.z,
                 tg.y * nt.x + bt.y * nt.y + n.y * nt.z,
                 tg.z * nt.x + bt.z * nt.y + n.z * nt.z);                  /* glm mat3*vec3 */
        n = normalize(m);
    }
    if (dot(n, rd) > 0.0f) { ARM(cz, ORC_ARM_NORMAL_FLIPPED); n = neg(n); }   /* :567-568 */
    p = add(p, muls(n, ORC_EPS));                                          /* :569 */

    if (!(iter < D)) { ARM(cz, ORC_ARM_TERMINAL); return 0; }             /* :571 */

    v3 diffuse = ld3(mat->diffuse);
    float c4[4];
    if (mat->tex[0] >= 0) { tex2d_impl(s, mat->tex[0], uvx, uvy, c4, cz, 0); diffuse = V(c4[0], c4[1], c4[2]); }
    v3 emiss = ld3(mat->emissive);
    if (mat->tex[2] >= 0) { tex2d_impl(s, mat->tex[2], uvx, uvy, c4, cz, 2); emiss = V(c4[0], c4[1], c4[2]); }
    float roughness = mat->roughness;
    if (mat->tex[3] >= 0)
    {
        tex2d_impl(s, mat->tex[3], uvx, uvy, c4, cz, 3); roughness = c4[0];
        if (roughness == 1.0f) ARM(cz, ORC_ARM_ROUGHNESS_TEXEL_ONE);
        if (roughness == 0.0f) ARM(cz, ORC_ARM_ROUGHNESS_TEXEL_ZERO);
    }
    float reflectiveness = mat->reflectiveness;
    if (mat->tex[4] >= 0)
    {
        tex2d_impl(s, mat->tex[4], uvx, uvy, c4, cz, 4); reflectiveness = c4[0];
        if (reflectiveness == 1.0f) ARM(cz, ORC_ARM_REFLECTIVENESS_TEXEL_ONE);
        if (reflectiveness == 0.0f) ARM(cz, ORC_ARM_REFLECTIVENESS_TEXEL_ZERO);
    }

    depth++; iter++;                                                      /* :586-587 */
    float mx = mat->diffuse[0] < mat->diffuse[1] ? mat->diffuse[1] : mat->diffuse[0];   /* glm::max */
    mx = mx < mat->diffuse[2] ? mat->diffuse[2] : mx;
    float prob = 0.95f < mx ? 0.95f : mx;                                 /* glm::min(0.95f, mx) */
    if (depth >= D)
    {
        const float rr = fabsf(rnd(rng));
        if (cz)
        {
            cz[ORC_ARM_RR_ENGAGED]++;
            cz[ORC_ARM_RR_CAP_ACTIVE] += 0.95f < mx;
            if (rr > prob) cz[0.95f < rr && rr <= mx ? ORC_ARM_RR_KILLED_UNDER_THE_CAP_ONLY : ORC_ARM_RR_KILLED_OTHERWISE]++;
            else cz[ORC_ARM_RR_SURVIVED]++;
        }
        if (rr > prob) return 0;                                          /* :590-594, no 1/prob */
    }

    v3 r = reflect(rd, n);                                                /* :596 */
    v3 dir;
    int diffuse_bounce = 0;
    v3 weight;

    if (mat->type == 0)
    {
        if (rnd(rng) < reflectiveness)                                    /* :601 */
        {
            if (roughness == 1.0f) { ARM(cz, ORC_ARM_OPAQUE_REFLECT_ROUGH_ONE); float w = rnd(rng), th = rnd(rng); dir = sample_about_impl(n, 1.0f - ORC_EPS, n, n, w, th, cz, 0); }
            else if (roughness == 0.0f) { ARM(cz, ORC_ARM_OPAQUE_REFLECT_MIRROR); dir = r; }
            else { ARM(cz, ORC_ARM_OPAQUE_REFLECT_LOBE); float w = rnd(rng) * roughness, th = rnd(rng); dir = sample_about_impl(n, 1.0f - ORC_FLT_EPSILON, r, r, w, th, cz, 1); }
            iter--;
            weight = ld3(mat->specular);                                  /* :626 */
        }
        else
        {
            float w = rnd(rng), th = rnd(rng);
            ARM(cz, ORC_ARM_OPAQUE_DIFFUSE);
            dir = sample_about_impl(n, 1.0f - ORC_EPS, n, n, w, th, cz, 2);   /* :631-636 */
            diffuse_bounce = 1;
            weight = diffuse;                                             /* :638 */
        }
    }
    else
    {
        int refract = 0;
        v3 refractN = n;
        ARM(cz, inside ? ORC_ARM_GLASS_ENTERED_INSIDE : ORC_ARM_GLASS_ENTERED_OUTSIDE);
        if (roughness != 0.0f)                                            /* :645-654 */
        {
            float w = rnd(rng) * roughness, th = rnd(rng);
            ARM(cz, ORC_ARM_GLASS_ROUGH_NORMAL);
            refractN = sample_about_impl(n, 1.0f - ORC_FLT_EPSILON, r, n, w, th, cz, 3);
        }
        float nc = 1.0f, ng = mat->ior;
        float eta = inside ? ng / nc : nc / ng;                           /* :658 */
        float r0 = (nc - ng) / (nc + ng);
        r0 = r0 * r0;
        float c = fabsf(dot(rd, refractN));
        float k = 1.0f - eta * eta * (1.0f - c * c);
        if (k < 0.0f) { ARM(cz, ORC_ARM_GLASS_TIR); refract = 0; }
        else
        {
            float re = r0 + (1.0f - r0) * (1.0f - c) * (1.0f - c);        /* :668 (squared) */
            if (fabsf(rnd(rng)) < re) { ARM(cz, ORC_ARM_GLASS_FRESNEL_REFLECT); refract = 0; }
            else if (rnd(rng) < reflectiveness) { ARM(cz, ORC_ARM_GLASS_REFLECTIVENESS_REFLECT); refract = 0; }
            else refract = 1;
        }
        if (!refract)
        {
            if (roughness == 1.0f) { ARM(cz, ORC_ARM_GLASS_REFLECT_ROUGH_ONE); float w = rnd(rng), th = rnd(rng); dir = sample_about_impl(n, 1.0f - ORC_EPS, n, n, w, th, cz, 4); }
            else if (roughness == 0.0f) { ARM(cz, ORC_ARM_GLASS_REFLECT_MIRROR); dir = r; }
            else { ARM(cz, ORC_ARM_GLASS_REFLECT_LOBE); float w = rnd(rng) * roughness, th = rnd(rng); dir = sample_about_impl(n, 1.0f - ORC_FLT_EPSILON, r, r, w, th, cz, 5); }
            iter--;
            weight = ld3(mat->specular);                                  /* :702 */
        }
        else if (rnd(rng) < mat->translucency)                            /* :706 */
        {
            ARM(cz, ORC_ARM_GLASS_REFRACT_TRANSMIT);
            float a = eta * dot(n, rd) + sqrtf(k);
            dir = normalize(sub(muls(rd, eta), muls(refractN, a)));       /* :708 */
            p = sub(p, muls(muls(n, ORC_EPS), 2.0f));                      /* :709 */
            inside = !inside;
            iter--;
            weight = diffuse;                                             /* :712 */
        }
        else
        {
            float w = rnd(rng), th = rnd(rng);
            ARM(cz, ORC_ARM_GLASS_REFRACT_DIFFUSE);
            dir = sample_about_impl(n, 1.0f - ORC_EPS, n, n, w, th, cz, 6);   /* :717-722 */
            diffuse_bounce = 1;
            weight = diffuse;                                             /* :724 */
        }
    }
    b->p = p; b->n = n; b->dir = dir;
    b->e = muls(emiss, mat->emissive_intensity);
    b->weight = weight; b->diffuse = diffuse; b->diffuse_bounce = diffuse_bounce;
    *depth_io = depth; *iter_io = iter; *inside_io = inside;
    return 1;
}

static int shade(const orc_scene* s, v3 ro, v3 rd, const hit_t* h, int D, int* depth_io, int* iter_io,
                 int* inside_io, rng_t* rng, bounce_t* b)
{
    return shade_impl(s, ro, rd, h, D, depth_io, iter_io, inside_io, rng, b, NULL);
}

/* PathTracer::Trace pathtracer.cpp:545-732, ITERATIVE form: L += T*emission; L += T*direct; T *= weight.
 * This is the estimator the HIP kernel implements and the one orc_render uses.  Draw order per
 * bounce: [RR] branch, direction (w, theta), then the three DirectIllumimation draws. */
static v3 trace(const orc_scene* s, v3 ro, v3 rd, int D, rng_t* rng)
{
    v3 L = V(0.0f, 0.0f, 0.0f), T = V(1.0f, 1.0f, 1.0f);
    int depth = 0, iter = 0, inside = 0;
    uint32_t ray = 0;
    for (;;)
    {
        hit_t h; bounce_t b;
        if (!closest_hit(s, ro, rd, rng, ray++, &h)) break;                  /* :550 */
        if (!shade(s, ro, rd, &h, D, &depth, &iter, &inside, rng, &b)) break;
        L = add(L, mulv(T, b.e));                                            /* emiss * I */
        if (b.diffuse_bounce)
        {
            v3 di = direct_illumination(s, b.p, b.n, b.diffuse, rng, &ray);   /* :638 / :724 */
            L = add(L, mulv(T, di));
        }
        T = mulv(T, b.weight);
        ro = b.p; rd = b.dir;
    }
    return L;
}

/* trace() with the counters of orc_render_counted: the same calls in the same order, so the same radiance bit for bit */
static v3 trace_counted(const orc_scene* s, v3 ro, v3 rd, int D, rng_t* rng, count_t* cc)
{
    v3 L = V(0.0f, 0.0f, 0.0f), T = V(1.0f, 1.0f, 1.0f);
    int depth = 0, iter = 0, inside = 0;
    uint32_t ray = 0;
    cc->px[ORC_CNT_PATHS]++;
    for (;;)
    {
        hit_t h; bounce_t b;
        const uint32_t r = ray++;
        if (!closest_hit_counted(s, ro, rd, rng, r, r == 0 ? ORC_RAY_CAMERA : ORC_RAY_BOUNCE, -1, cc, &h)) break;
        /* shade() looks up the normal map of every hit, the other four maps only below the depth limit (:571) */
        const int32_t* tx = s->mats[s->material[h.tri]].tex;
        cc->px[ORC_CNT_SHADED]++;
        cc->px[ORC_CNT_TEX_SHADE] += (tx[1] >= 0) + (iter < D ? (tx[0] >= 0) + (tx[2] >= 0) + (tx[3] >= 0) + (tx[4] >= 0) : 0);
        if (!shade(s, ro, rd, &h, D, &depth, &iter, &inside, rng, &b)) break;
        L = add(L, mulv(T, b.e));
        if (b.diffuse_bounce)
        {
            v3 di = direct_illumination_c(s, b.p, b.n, b.diffuse, rng, &ray, cc);
            L = add(L, mulv(T, di));
        }
        T = mulv(T, b.weight);
        ro = b.p; rd = b.dir;
    }
    cc->px[ORC_CNT_RAY_NUMBERS] += ray;
    return L;
}

/* trace() with the census: the same calls in the same order, so the same radiance bit for bit */
static v3 trace_census(const orc_scene* s, v3 ro, v3 rd, int D, rng_t* rng, int64_t* cz, int brute)
{
    v3 L = V(0.0f, 0.0f, 0.0f), T = V(1.0f, 1.0f, 1.0f);
    int depth = 0, iter = 0, inside = 0;
    uint32_t ray = 0;
    for (;;)
    {
        hit_t h; bounce_t b;
        if (!closest_hit_census(s, ro, rd, rng, ray++, &h, cz, brute)) break;
        if (!shade_impl(s, ro, rd, &h, D, &depth, &iter, &inside, rng, &b, cz)) break;
        L = add(L, mulv(T, b.e));
        if (b.diffuse_bounce)
        {
            v3 di = direct_illumination_impl(s, b.p, b.n, b.diffuse, rng, &ray, NULL, cz, brute);
            L = add(L, mulv(T, di));
        }
        T = mulv(T, b.weight);
        ro = b.p; rd = b.dir;
    }
    return L;
}

/* The same estimator in the reference's RECURSIVE form, with the operand evaluation order g++
 * chose for `emiss*I + DirectIllumimation(..) + Trace(..)*diffuse` (pathtracer.cpp:638, :724):
 * nee_last=1 evaluates the recursive Trace before DirectIllumimation.  Used only to replay the
 * reference's draw tapes (tier T) and to tie the iterative form to them. */
static v3 trace_rec(const orc_scene* s, v3 ro, v3 rd, int D, int depth, int iter, int inside,
                    rng_t* rng, uint32_t* ray, int nee_last)
{
    hit_t h; bounce_t b;
    if (!closest_hit(s, ro, rd, rng, (*ray)++, &h)) return V(0.0f, 0.0f, 0.0f);
    if (!shade(s, ro, rd, &h, D, &depth, &iter, &inside, rng, &b)) return V(0.0f, 0.0f, 0.0f);
    if (!b.diffuse_bounce)
        return add(b.e, mulv(trace_rec(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last), b.weight));
    v3 di, sub_;
    if (nee_last)
    {
        sub_ = trace_rec(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last);
        di = direct_illumination(s, b.p, b.n, b.diffuse, rng, ray);
    }
    else
    {
        di = direct_illumination(s, b.p, b.n, b.diffuse, rng, ray);
        sub_ = trace_rec(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last);
    }
    return add(add(b.e, di), mulv(sub_, b.weight));
}

/* trace_rec() with the census: the same calls in the same order, so the same radiance bit for bit.  (A recursive function cannot
 * be always-inlined with a literal NULL, so it is a copy, as trace_census is of trace; the walk is the tree's, as trace_rec's.) */
static v3 trace_rec_census(const orc_scene* s, v3 ro, v3 rd, int D, int depth, int iter, int inside,
                           rng_t* rng, uint32_t* ray, int nee_last, int64_t* cz)
{
    hit_t h; bounce_t b;
    memset(&b, 0, sizeof b);
    if (!closest_hit_census(s, ro, rd, rng, (*ray)++, &h, cz, 0)) return V(0.0f, 0.0f, 0.0f);
    if (!shade_impl(s, ro, rd, &h, D, &depth, &iter, &inside, rng, &b, cz)) return V(0.0f, 0.0f, 0.0f);
    if (!b.diffuse_bounce)
        return add(b.e, mulv(trace_rec_census(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last, cz), b.weight));
    v3 di, sub_;
    if (nee_last)
    {
        sub_ = trace_rec_census(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last, cz);
        di = direct_illumination_impl(s, b.p, b.n, b.diffuse, rng, ray, NULL, cz, 0);
    }
    else
    {
        di = direct_illumination_impl(s, b.p, b.n, b.diffuse, rng, ray, NULL, cz, 0);
        sub_ = trace_rec_census(s, b.p, b.dir, D, depth, iter, inside, rng, ray, nee_last, cz);
    }
    return add(add(b.e, di), mulv(sub_, b.weight));
}

/* mode 0: iterative (NEE draws first); 1: recursive, NEE first; 2: recursive, NEE last */
ORC_INLINE int trace_tape_impl(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                               const float* tape, int tape_len, int mode, float* out3, int64_t* cz)
{
    rng_t r; rng_init(&r, 0, 0);
    r.tape = tape; r.tape_len = tape_len; r.tape_pos = 0;
    v3 c;
    uint32_t ray = 0;
    if (mode == 0) c = cz ? trace_census(s, ld3(ro), ld3(rd), max_depth, &r, cz, 0) : trace(s, ld3(ro), ld3(rd), max_depth, &r);
    else c = cz ? trace_rec_census(s, ld3(ro), ld3(rd), max_depth, 0, 0, 0, &r, &ray, mode == 2, cz)
                : trace_rec(s, ld3(ro), ld3(rd), max_depth, 0, 0, 0, &r, &ray, mode == 2);
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
    return r.tape_pos;
}
int orc_trace_tape(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                   const float* tape, int tape_len, int mode, float* out3)
{
    return trace_tape_impl(s, ro, rd, max_depth, tape, tape_len, mode, out3, NULL);
}
/* ... ADDING the arms the replay takes to arms[ORC_ARM_N] (the caller zeroes them: a tier-T fixture is many paths) */
int orc_trace_tape_census(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                          const float* tape, int tape_len, int mode, float* out3, int64_t* arms)
{
    return trace_tape_impl(s, ro, rd, max_depth, tape, tape_len, mode, out3, arms);
}

/* Counter-RNG radiance of sample `sample` of `pixel` from an explicit ray, iterative (mode 0) or
 * recursive NEE-first (mode 1): ties the two forms together on identical draws. */
void orc_trace_counter(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                       uint64_t seed, uint32_t pixel, uint32_t sample, int mode, float* out3)
{
    rng_t r; rng_init(&r, pixel_key(seed, pixel), sample);
    v3 c;
    uint32_t ray = 0;
    if (mode == 0) c = trace(s, ld3(ro), ld3(rd), max_depth, &r);
    else c = trace_rec(s, ld3(ro), ld3(rd), max_depth, 0, 0, 0, &r, &ray, 0);
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
}

/* ---- camera, PathTracer::RenderFrame pathtracer.cpp:755-766 -----------------------------------*/
typedef struct { v3 pos, dir, up, right, topLeft; float deltaX, deltaY; } frame_t;

static void frame_setup(const orc_camera* cam, int W, int H, frame_t* f)
{
    f->pos = ld3(cam->pos); f->dir = ld3(cam->dir); f->up = ld3(cam->up);
    v3 imgCenter = add(f->pos, muls(f->dir, cam->focal));
    float imgHeight = (float)((double)(2.0f * cam->focal) * tan((double)(cam->fovy / 2.0f) * ORC_PI_D / (double)180.0f));
    float aspect = (float)W / (float)H;
    float imgWidth = imgHeight * aspect;
    f->deltaX = imgWidth / (float)W;
    f->deltaY = imgHeight / (float)H;
    f->right = normalize(cross(f->up, f->dir));
    v3 topLeft = sub(imgCenter, muls(f->right, imgWidth * 0.5f));
    f->topLeft = add(topLeft, muls(f->up, imgHeight * 0.5f));
}

static void primary_row(const frame_t* f, int W, int i, float* out /* [W][3] */)
{
    v3 pixel = sub(f->topLeft, muls(f->up, (float)i * f->deltaY));             /* :782 */
    v3 step = muls(f->right, f->deltaX);
    for (int j = 0; j < W; j++)
    {
        v3 rayDir = normalize(sub(pixel, f->pos));                             /* :785 */
        out[j * 3] = rayDir.x; out[j * 3 + 1] = rayDir.y; out[j * 3 + 2] = rayDir.z;
        pixel = add(pixel, step);                                              /* :814 */
    }
}

void orc_primary_dirs(const orc_camera* cam, int W, int H, float* out)
{
    frame_t f; frame_setup(cam, W, H, &f);
    for (int i = 0; i < H; i++) primary_row(&f, W, i, out + (size_t)i * W * 3);
}

/* PathTracer::SampleCircle pathtracer.cpp:734-739 with the two draws passed in */
void orc_sample_circle(float r1, float r2, float* out2)
{
    float angle = (float)((double)r1 * 2. * ORC_PI_D);
    float radius = sqrtf(r2);
    float sn, cs;
    orc_sincos(angle, &sn, &cs);
    out2[0] = cs * radius; out2[1] = sn * radius;
}

/* AABB::Intersect, mesh.cpp:48-59, verbatim semantics: (min - ro) / rd with IEEE division (rd components may be 0),
 * glm min/max = (y < x ? y : x) / (x < y ? y : x), no t-max, boxes behind the ray are NOT rejected.  The oracle's own
 * traversal does not use it (its boxes only accelerate; closest hit is tree-independent) - this probe pins the row a5. */
int orc_aabb_intersect(const float* bmin, const float* bmax, const float* ro, const float* rd)
{
    float t1[3], t2[3];
    for (int a = 0; a < 3; a++)
    {
        float tmin = (bmin[a] - ro[a]) / rd[a], tmax = (bmax[a] - ro[a]) / rd[a];
        t1[a] = tmax < tmin ? tmax : tmin;          /* glm::min(tMin, tMax) */
        t2[a] = tmin < tmax ? tmax : tmin;          /* glm::max(tMin, tMax) */
    }
    float m01 = t1[0] < t1[1] ? t1[1] : t1[0];
    float tNear = m01 < t1[2] ? t1[2] : m01;
    float n01 = t2[1] < t2[0] ? t2[1] : t2[0];
    float tFar = t2[2] < n01 ? t2[2] : n01;
    return tNear >= tFar ? 0 : 1;
}

/* AABB::Build over n points then AABB::Check, mesh.cpp:6-46 (min/max start at +-(float)0xFFFF, mesh.h:13,63-64;
 * Check inflates a zero-thickness axis by EPS) */
void orc_aabb_build(const float* pts, int n, float* out6)
{
    const float INF_ = (float)0xFFFF;
    float mn[3] = { INF_, INF_, INF_ }, mx[3] = { -INF_, -INF_, -INF_ };
    for (int i = 0; i < n; i++)
        for (int a = 0; a < 3; a++)
        {
            float v = pts[i * 3 + a];
            if (v < mn[a]) mn[a] = v;
            if (v > mx[a]) mx[a] = v;
        }
    for (int a = 0; a < 3; a++) if (mn[a] == mx[a]) mx[a] += ORC_EPS;
    for (int a = 0; a < 3; a++) { out6[a] = mn[a]; out6[3 + a] = mx[a]; }
}

/* DirectIllumimation (pathtracer.cpp:504-531) with its three draws taken from `tape3` */
void orc_direct_illumination_tape(const orc_scene* s, const float* p, const float* n, const float* diffuse, const float* tape3, float* out3)
{
    rng_t rng; memset(&rng, 0, sizeof rng);
    rng.tape = tape3; rng.tape_len = 3; rng.tape_pos = 0;
    uint32_t ray = 0;
    v3 c = direct_illumination(s, ld3(p), ld3(n), ld3(diffuse), &rng, &ray);
    out3[0] = c.x; out3[1] = c.y; out3[2] = c.z;
}

void orc_render(const orc_scene* s, const orc_camera* cam, int W, int H, int D,
                uint32_t first_sample, uint32_t spp, uint64_t seed, int rank, int world,
                float* total, uint8_t* rgb8, int threads)
{
    frame_t f; frame_setup(cam, W, H, &f);
    int tiles_x = (W + ORC_TILE - 1) / ORC_TILE, tiles_y = (H + ORC_TILE - 1) / ORC_TILE;
    if (world < 1) world = 1;
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
#endif
    /* the rows' primary directions first (each row is an incremental walk from its first column, :782-785, :814) ... */
    float* dirs_all = (float*)malloc((size_t)W * H * 3 * sizeof(float));
#ifdef _OPENMP
#pragma omp parallel for schedule(static) num_threads(threads)
#endif
    for (int i = 0; i < H; i++) primary_row(&f, W, i, dirs_all + (size_t)i * W * 3);
    /* ... then the pixels, dealt to the threads as 16 x 16 tiles (the reference deals whole rows to its workers, :777: with
     * hundreds of threads and a frame whose lit pixels sit in a band of rows that leaves most of them idle; the result
     * of a pixel does not depend on who computes it) */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
#endif
    for (int t = 0; t < tiles_x * tiles_y; t++)
    {
        const int ty = t / tiles_x, tx = t % tiles_x;
        const int tile = ty * tiles_x + (tx + 3 * ty) % tiles_x;    /* rows rotated by 3 tiles: diagonal ownership */
        if (tile % world != rank) continue;
        for (int i = ty * ORC_TILE; i < (ty + 1) * ORC_TILE && i < H; i++)     /* :777 */
        {
            const float* dirs = dirs_all + (size_t)i * W * 3;
            for (int j = tx * ORC_TILE; j < (tx + 1) * ORC_TILE && j < W; j++) /* :783 */
            {
                uint32_t pkey = pixel_key(seed, (uint32_t)(i * W + j));
                size_t px = ((size_t)(H - 1 - i) * W + j) * 3;                 /* :796 bottom-up */
                v3 acc = ld3(total + px);
                v3 rayDir0 = ld3(dirs + j * 3);
                for (uint32_t k = 0; k < spp; k++)
                {
                    rng_t rng; rng_init(&rng, pkey, first_sample + k);
                    v3 camPos = f.pos;                                         /* :787 */
                    v3 focalPoint = add(camPos, muls(rayDir0, cam->focal_dist));   /* :788 */
                    float r1 = rnd(&rng), r2 = rnd(&rng), off[2];
                    orc_sample_circle(r1, r2, off);
                    off[0] = off[0] * cam->aperture; off[1] = off[1] * cam->aperture;   /* :789 */
                    camPos = add(camPos, add(muls(f.right, off[0]), muls(f.up, off[1])));   /* :790 */
                    v3 rayDir = normalize(sub(focalPoint, camPos));            /* :791 */
                    v3 color = trace(s, camPos, rayDir, D, &rng);              /* :793 */
                    acc = add(acc, color);                                     /* :798-800 */
                }
                total[px] = acc.x; total[px + 1] = acc.y; total[px + 2] = acc.z;
                if (rgb8)
                {
                    float ns = (float)(first_sample + spp);                    /* (float)mSamples */
                    float c[3] = { acc.x / ns, acc.y / ns, acc.z / ns };
                    for (int k = 0; k < 3; k++)
                    {
                        float x = c[k];
                        x = x < 0.0f ? 0.0f : (x > 1.0f ? 1.0f : x);           /* glm::clamp; NaN -> NaN */
                        if (!(x == x)) x = 0.0f;
                        rgb8[px + k] = (uint8_t)(x * 255);                     /* :810-812 truncation */
                    }
                }
            }
        }
    }
    free(dirs_all);
}

int orc_render_counted(const orc_scene* s, const orc_camera* cam, int W, int H, int D,
                       uint32_t first_sample, uint32_t spp, uint64_t seed, int rank, int world,
                       float* total, int64_t* counts, orc_ray_rec* rec, const int64_t* rec_offsets, int64_t rec_capacity, int threads)
{
    frame_t f; frame_setup(cam, W, H, &f);
    int tiles_x = (W + ORC_TILE - 1) / ORC_TILE, tiles_y = (H + ORC_TILE - 1) / ORC_TILE;
    if (world < 1) world = 1;
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
#endif
    int brute = 0;
    for (int m = 0; m < s->nm; m++) brute |= s->mats[m].tex[5] >= 0;
    float* dirs_all = (float*)malloc((size_t)W * H * 3 * sizeof(float));
    for (int i = 0; i < H; i++) primary_row(&f, W, i, dirs_all + (size_t)i * W * 3);
    memset(counts, 0, (size_t)W * H * ORC_CNT_N * sizeof(int64_t));
    int overflow = 0;
    /* every pixel's counters and records are written by the one thread that traces it: the result does not depend on the
       thread count */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads) reduction(| : overflow)
#endif
    for (int t = 0; t < tiles_x * tiles_y; t++)
    {
        const int ty = t / tiles_x, tx = t % tiles_x;
        const int tile = ty * tiles_x + (tx + 3 * ty) % tiles_x;
        if (tile % world != rank) continue;
        for (int i = ty * ORC_TILE; i < (ty + 1) * ORC_TILE && i < H; i++)
            for (int j = tx * ORC_TILE; j < (tx + 1) * ORC_TILE && j < W; j++)
            {
                const size_t pix = (size_t)i * W + j;
                count_t cc;
                cc.px = counts + pix * ORC_CNT_N; cc.brute = brute; cc.overflow = 0; cc.pixel = (uint32_t)pix;
                cc.rec = rec ? rec + rec_offsets[pix] : NULL;
                cc.rec_end = rec ? rec + rec_capacity : NULL;
                uint32_t pkey = pixel_key(seed, (uint32_t)pix);
                size_t px = ((size_t)(H - 1 - i) * W + j) * 3;
                v3 acc = total ? ld3(total + px) : V(0.0f, 0.0f, 0.0f);
                v3 rayDir0 = ld3(dirs_all + pix * 3);
                for (uint32_t k = 0; k < spp; k++)
                {
                    rng_t rng; rng_init(&rng, pkey, first_sample + k);
                    cc.sample = first_sample + k;
                    v3 camPos = f.pos;
                    v3 focalPoint = add(camPos, muls(rayDir0, cam->focal_dist));
                    float r1 = rnd(&rng), r2 = rnd(&rng), off[2];
                    orc_sample_circle(r1, r2, off);
                    off[0] = off[0] * cam->aperture; off[1] = off[1] * cam->aperture;
                    camPos = add(camPos, add(muls(f.right, off[0]), muls(f.up, off[1])));
                    v3 rayDir = normalize(sub(focalPoint, camPos));
                    acc = add(acc, trace_counted(s, camPos, rayDir, D, &rng, &cc));
                }
                if (total) { total[px] = acc.x; total[px + 1] = acc.y; total[px + 2] = acc.z; }
                overflow |= cc.overflow;
            }
    }
    free(dirs_all);
    return overflow ? -1 : 0;
}

static const char* const orc_arm_names[ORC_ARM_N] = {
#define TEX_NAMES(slot, name) \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_MISSING] = "tex2d." name ".missing_texture", \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_HI_X] = "tex2d." name ".upper_clamp_x", \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_HI_Y] = "tex2d." name ".upper_clamp_y", \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_LO_X] = "tex2d." name ".lower_clamp_x", \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_LO_Y] = "tex2d." name ".lower_clamp_y", \
    [ORC_ARM_TEX + slot * ORC_TEX_ARMS + ORC_TEX_PLAIN] = "tex2d." name ".plain_fetch"
    TEX_NAMES(0, "diffuse"), TEX_NAMES(1, "normal"), TEX_NAMES(2, "emissive"), TEX_NAMES(3, "roughness"), TEX_NAMES(4, "metallic"),
    TEX_NAMES(5, "opacity"),
#undef TEX_NAMES
    [ORC_ARM_TRI_FARTHER] = "test_triangle.rejected_farther", [ORC_ARM_TRI_NEARER] = "test_triangle.accepted_nearer",
    [ORC_ARM_TRI_TIE_ACCEPTED] = "test_triangle.tie_accepted_smaller_index",
    [ORC_ARM_TRI_TIE_REJECTED] = "test_triangle.tie_rejected_larger_index",
    [ORC_ARM_TRI_OPACITY_KEPT] = "test_triangle.opacity_draw_kept", [ORC_ARM_TRI_OPACITY_DROPPED] = "test_triangle.opacity_draw_dropped",
    [ORC_ARM_WALK_STACK_FULL] = "closest_hit.stack_guard",
    [ORC_ARM_SMOOTHING_ON] = "shade.smoothing_on", [ORC_ARM_SMOOTHING_OFF] = "shade.smoothing_off",
    [ORC_ARM_NORMAL_MAP_ON] = "shade.normal_map_on", [ORC_ARM_NORMAL_MAP_OFF] = "shade.normal_map_off",
    [ORC_ARM_NT_Z_CLAMPED] = "shade.nt_z_clamped", [ORC_ARM_NORMAL_FLIPPED] = "shade.normal_flipped",
    [ORC_ARM_TERMINAL] = "shade.terminal", [ORC_ARM_RR_ENGAGED] = "shade.rr_engaged", [ORC_ARM_RR_CAP_ACTIVE] = "shade.rr_cap_active",
    [ORC_ARM_RR_KILLED_UNDER_THE_CAP_ONLY] = "shade.rr_killed_between_cap_and_max",
    [ORC_ARM_RR_KILLED_OTHERWISE] = "shade.rr_killed_otherwise", [ORC_ARM_RR_SURVIVED] = "shade.rr_survived",
    [ORC_ARM_OPAQUE_REFLECT_ROUGH_ONE] = "shade.opaque.reflect_roughness_one", [ORC_ARM_OPAQUE_REFLECT_MIRROR] = "shade.opaque.reflect_roughness_zero",
    [ORC_ARM_OPAQUE_REFLECT_LOBE] = "shade.opaque.reflect_lobe", [ORC_ARM_OPAQUE_DIFFUSE] = "shade.opaque.diffuse",
    [ORC_ARM_GLASS_ENTERED_OUTSIDE] = "shade.glass.inside_0", [ORC_ARM_GLASS_ENTERED_INSIDE] = "shade.glass.inside_1",
    [ORC_ARM_GLASS_ROUGH_NORMAL] = "shade.glass.roughness_nonzero", [ORC_ARM_GLASS_TIR] = "shade.glass.tir",
    [ORC_ARM_GLASS_FRESNEL_REFLECT] = "shade.glass.fresnel_reflect", [ORC_ARM_GLASS_REFLECTIVENESS_REFLECT] = "shade.glass.reflectiveness_reflect",
    [ORC_ARM_GLASS_REFLECT_ROUGH_ONE] = "shade.glass.reflect_roughness_one", [ORC_ARM_GLASS_REFLECT_MIRROR] = "shade.glass.reflect_roughness_zero",
    [ORC_ARM_GLASS_REFLECT_LOBE] = "shade.glass.reflect_lobe",
    [ORC_ARM_GLASS_REFRACT_TRANSMIT] = "shade.glass.refract_transmit", [ORC_ARM_GLASS_REFRACT_DIFFUSE] = "shade.glass.refract_diffuse",
    [ORC_ARM_ROUGHNESS_TEXEL_ONE] = "shade.roughness_texel_one", [ORC_ARM_ROUGHNESS_TEXEL_ZERO] = "shade.roughness_texel_zero",
    [ORC_ARM_REFLECTIVENESS_TEXEL_ZERO] = "shade.reflectiveness_texel_zero", [ORC_ARM_REFLECTIVENESS_TEXEL_ONE] = "shade.reflectiveness_texel_one",
#define SA_NAMES(site, name) \
    [ORC_ARM_SA + site * ORC_SA_CLASSES + ORC_SA_BELOW] = "sample_about." name ".below_1_minus_eps", \
    [ORC_ARM_SA + site * ORC_SA_CLASSES + ORC_SA_BAND] = "sample_about." name ".in_the_band", \
    [ORC_ARM_SA + site * ORC_SA_CLASSES + ORC_SA_POLE] = "sample_about." name ".at_or_above_1_minus_flt_epsilon"
    SA_NAMES(0, "opaque_rough_one"), SA_NAMES(1, "opaque_lobe"), SA_NAMES(2, "opaque_diffuse"), SA_NAMES(3, "glass_refract_normal"),
    SA_NAMES(4, "glass_rough_one"), SA_NAMES(5, "glass_lobe"), SA_NAMES(6, "glass_diffuse"),
#undef SA_NAMES
    [ORC_ARM_DI_NO_LIGHTS] = "direct.no_lights", [ORC_ARM_DI_LIGHT_ID_CLAMPED] = "direct.light_id_clamped",
    [ORC_ARM_DI_NDL_NOT_POSITIVE] = "direct.ndl_not_positive", [ORC_ARM_DI_SHADOW_MISSED] = "direct.shadow_ray_missed_everything",
    [ORC_ARM_DI_HIT_LIGHT] = "direct.shadow_ray_hit_its_light", [ORC_ARM_DI_HIT_OTHER] = "direct.shadow_ray_hit_something_else",
};
int orc_arm_count(void) { return ORC_ARM_N; }
const char* orc_arm_name(int arm) { return arm >= 0 && arm < ORC_ARM_N ? orc_arm_names[arm] : NULL; }

void orc_render_census(const orc_scene* s, const orc_camera* cam, int W, int H, int D, uint32_t first_sample, uint32_t spp,
                       uint64_t seed, int brute, float* total, int64_t* arms, int threads)
{
    frame_t f; frame_setup(cam, W, H, &f);
#ifdef _OPENMP
    if (threads <= 0) threads = omp_get_max_threads();
#endif
    float* dirs_all = (float*)malloc((size_t)W * H * 3 * sizeof(float));
    for (int i = 0; i < H; i++) primary_row(&f, W, i, dirs_all + (size_t)i * W * 3);
    memset(arms, 0, ORC_ARM_N * sizeof(int64_t));
    /* a row's arms are counted by the one thread that traces it and added under a lock: sums, so no thread count shows */
#ifdef _OPENMP
#pragma omp parallel for schedule(dynamic, 1) num_threads(threads)
#endif
    for (int i = 0; i < H; i++)
    {
        int64_t row[ORC_ARM_N];
        memset(row, 0, sizeof row);
        for (int j = 0; j < W; j++)
        {
            const size_t pix = (size_t)i * W + j;
            uint32_t pkey = pixel_key(seed, (uint32_t)pix);
            size_t px = ((size_t)(H - 1 - i) * W + j) * 3;
            v3 acc = total ? ld3(total + px) : V(0.0f, 0.0f, 0.0f);
            v3 rayDir0 = ld3(dirs_all + pix * 3);
            for (uint32_t k = 0; k < spp; k++)
            {
                rng_t rng; rng_init(&rng, pkey, first_sample + k);
                v3 camPos = f.pos;
                v3 focalPoint = add(camPos, muls(rayDir0, cam->focal_dist));
                float r1 = rnd(&rng), r2 = rnd(&rng), off[2];
                orc_sample_circle(r1, r2, off);
                off[0] = off[0] * cam->aperture; off[1] = off[1] * cam->aperture;
                camPos = add(camPos, add(muls(f.right, off[0]), muls(f.up, off[1])));
                v3 rayDir = normalize(sub(focalPoint, camPos));
                acc = add(acc, trace_census(s, camPos, rayDir, D, &rng, row, brute));
            }
            if (total) { total[px] = acc.x; total[px + 1] = acc.y; total[px + 2] = acc.z; }
        }
#ifdef _OPENMP
#pragma omp critical(orc_census)
#endif
        for (int a = 0; a < ORC_ARM_N; a++) arms[a] += row[a];
    }
    free(dirs_all);
}

/* RenderFrame (pathtracer.cpp:741-817) for ONE frame with the draws of the reference's single engine on tape, in the order its
 * loop consumes them when it runs on one thread: rows top to bottom, columns left to right, per pixel the two draws of
 * SampleCircle (:736-737) and then the path's (recursive form, g++'s operand order).  Adds into `total` (rows bottom-up, :796)
 * and returns the number of draws consumed.  Test infrastructure for tools/fuzz_frame_vs_reference.py. */
ORC_INLINE int render_tape_impl(const orc_scene* s, const orc_camera* cam, int W, int H, int D, const float* tape, int tape_len, float* total,
                                int64_t* cz)
{
    frame_t f; frame_setup(cam, W, H, &f);
    float* dirs = (float*)malloc((size_t)W * 3 * sizeof(float));
    rng_t r; rng_init(&r, 0, 0);
    r.tape = tape; r.tape_len = tape_len; r.tape_pos = 0;
    for (int i = 0; i < H; i++)
    {
        primary_row(&f, W, i, dirs);
        for (int j = 0; j < W; j++)
        {
            size_t px = ((size_t)(H - 1 - i) * W + j) * 3;
            v3 rayDir0 = ld3(dirs + j * 3);
            v3 camPos = f.pos;
            v3 focalPoint = add(camPos, muls(rayDir0, cam->focal_dist));
            float r1 = rnd(&r), r2 = rnd(&r), off[2];
            orc_sample_circle(r1, r2, off);
            off[0] = off[0] * cam->aperture; off[1] = off[1] * cam->aperture;
            camPos = add(camPos, add(muls(f.right, off[0]), muls(f.up, off[1])));
            v3 rayDir = normalize(sub(focalPoint, camPos));
            uint32_t ray = 0;
            v3 color = cz ? trace_rec_census(s, camPos, rayDir, D, 0, 0, 0, &r, &ray, 1, cz) : trace_rec(s, camPos, rayDir, D, 0, 0, 0, &r, &ray, 1);
            total[px] += color.x; total[px + 1] += color.y; total[px + 2] += color.z;
        }
    }
    free(dirs);
    return r.tape_pos;
}
int orc_render_tape(const orc_scene* s, const orc_camera* cam, int W, int H, int D, const float* tape, int tape_len, float* total)
{
    return render_tape_impl(s, cam, W, H, D, tape, tape_len, total, NULL);
}
/* ... ADDING the arms the replay takes to arms[ORC_ARM_N] */
int orc_render_tape_census(const orc_scene* s, const orc_camera* cam, int W, int H, int D, const float* tape, int tape_len, float* total,
                           int64_t* arms)
{
    return render_tape_impl(s, cam, W, H, D, tape, tape_len, total, arms);
}


void orc_intersect_many(int64_t n, const float* ro, const float* rd, const float* tri9, float* out3)
{
    for (int64_t i = 0; i < n; i++)
        orc_intersect_triangle(ro + 3 * i, rd + 3 * i, tri9 + 9 * i, tri9 + 9 * i + 3, tri9 + 9 * i + 6, out3 + 3 * i);
}
