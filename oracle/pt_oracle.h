/* TEST INFRASTRUCTURE ONLY — never imported, linked or executed by the product path.
 *
 * CPU restatement (plain C99) of the reference's per-pixel render loop
 *   PathTracer::RenderFrame -> Trace -> Hit -> {IntersectTriangle, Image::tex2D, DirectIllumimation}
 *   (reference PathTracing/src/pathtracer.cpp:367-822, mesh.cpp:48-83, image.cpp:63-86)
 * used by tests/, __graft_entry__.smoke() and bench.py's cpu_baseline leg as the checker for the HIP
 * kernels.  Parity pinning: tests/golden/ holds vectors generated from the REAL reference
 * (oracle/_ref, built from /root/reference by oracle/Makefile.ref) with oracle/gen_golden.py; the
 * "not gpu" tests replay them against this file (tiers K / T / S of SURVEY.md §8c4).
 *
 * Deliberate, documented differences from the reference (none changes the estimator):
 *   - Trace is iterative (L += T*(emission + direct); T *= weight) — exact for a recursion that is
 *     linear in the recursive term; differs from the recursion by float rounding only (<=1e-5 rel).
 *   - The RNG is counter-based PCG (key = seed, pixel, sample) instead of one raced std::mt19937;
 *     a "tape" mode replays the reference's own draw stream for the tier-T vectors.
 *   - Closest hit is the minimum over all accepted triangles with the order-independent tie rule
 *     (smaller t, then smaller triangle index); the reference's tie depends on its random tree.
 *   - Stochastic opacity is evaluated only for candidates nearer than the current best hit, each
 *     with an independent hashed draw (same distribution of the closest accepted hit).
 *   - tex2D clamps the texel coordinate to the image (the reference reads one texel past a row when
 *     u rounds to 1.0 after the wrap, image.cpp:71-77).
 *   - sin/cos use the polynomial below instead of libm (<=1 ulp from cosf/sinf) so that this file
 *     and the HIP kernel can be bit-identical.
 */
#ifndef PT_ORACLE_H
#define PT_ORACLE_H

#include <stdint.h>
#include <stddef.h>

#ifdef __cplusplus
extern "C" {
#endif

/* Same memory layout as include/ptk.h (the drop-in boundary's data format), restated here so the
 * oracle does not include product headers. */
typedef struct {
    int32_t type;              /* 0 OPAQUE, 1 TRANSLUCENT (mesh.h:15-19) */
    float diffuse[3];
    float specular[3];
    float emissive[3];
    float emissive_intensity;
    float roughness;
    float reflectiveness;
    float translucency;
    float ior;
    int32_t tex[6];            /* diffuse, normal, emissive, roughness, metallic, opacity; -1 none */
} orc_material;                /* 84 bytes */

typedef struct {
    int32_t width, height;
    int64_t offset;            /* byte offset of the RGBA8 texels in the atlas */
} orc_texture;

typedef struct {
    int32_t num_triangles;
    const float* verts;        /* [N][9]  v1 v2 v3 (world space) */
    const float* normals;      /* [N][9]  n1 n2 n3 */
    const float* uvs;          /* [N][6]  uv1 uv2 uv3 */
    const float* tbn;          /* [N][9]  normal, tangent, bitangent (Triangle::Init) */
    const uint8_t* smoothing;  /* [N] */
    const int32_t* material;   /* [N] index into materials */
    int32_t num_materials;
    const orc_material* materials;
    int32_t num_textures;
    const orc_texture* textures;
    const uint8_t* texels;
    int64_t texel_bytes;
    int32_t num_lights;
    const int32_t* lights;     /* triangle indices with |emissive| >= EPS (pathtracer.cpp:267-273) */
} orc_scene_desc;

typedef struct {
    float pos[3], dir[3], up[3];   /* dir/up already normalised (SetCamera, pathtracer.cpp:333-338) */
    float focal, fovy;             /* SetProjection (already clamped) */
    float focal_dist, aperture;
} orc_camera;

typedef struct orc_scene orc_scene;

orc_scene* orc_create(const orc_scene_desc* desc);   /* copies everything, builds its own BVH */
void orc_destroy(orc_scene* s);

/* Render samples [first_sample, first_sample+spp) of every pixel, OpenMP over rows.
 * total: float RGB W*H*3, bottom-up rows (the reference's mTotalImg layout, pathtracer.cpp:796);
 * it is READ and accumulated into, sample by sample, like successive RenderFrame() calls.
 * rgb8 (may be NULL): clamp(total/(first_sample+spp))*255 truncated (pathtracer.cpp:802-812).
 * rank/world: only pixels of tiles owned by `rank` are rendered (tile = 16x16 pixels, owner of tile
 * (tx, ty) = (ty*tiles_x + (tx + 3*ty) % tiles_x) % world, as include/ptk.h ptk_set_tile).  threads<=0: OpenMP default. */
void orc_render(const orc_scene* s, const orc_camera* cam, int width, int height, int max_depth,
                uint32_t first_sample, uint32_t spp, uint64_t seed, int rank, int world,
                float* total, uint8_t* rgb8, int threads);

/* orc_render that also COUNTS, per pixel (counts [H][W][ORC_CNT_N], rows top-down, the kernels' pixel index), what the trace
 * kernels' STATS build counts (include/ptk.h ptk_stats): paths, closest-hit traversals by kind, surface interactions shaded,
 * texel lookups at shading time, opacity texels looked up, and the sum over paths of the final ray number.  The opacity count
 * follows the brute-force ascending-index candidate order (orc_hit_brute), the FLAT kernel's.  rec (may be NULL): one record
 * per closest-hit traversal; pixel p's records start at rec[rec_offsets[p]] (exclusive prefix sums of a previous call's
 * camera + bounce + shadow counts), in the order they are cast.  total (may be NULL) is accumulated as orc_render does.
 * Returns 0, or -1 when rec_capacity was too small.  The result does not depend on the thread count. */
enum { ORC_CNT_PATHS = 0, ORC_CNT_CAMERA, ORC_CNT_BOUNCE, ORC_CNT_SHADOW, ORC_CNT_SHADED, ORC_CNT_TEX_SHADE, ORC_CNT_TEX_OPACITY,
       ORC_CNT_RAY_NUMBERS, ORC_CNT_N };
enum { ORC_RAY_CAMERA = 0, ORC_RAY_BOUNCE = 1, ORC_RAY_SHADOW = 2 };
typedef struct {
    uint32_t pixel, sample, ray;   /* ray: the path's ray number (the opacity draws' key) */
    int32_t kind;                  /* ORC_RAY_* */
    float ro[3], rd[3];
    float t; int32_t tri;          /* closest accepted hit; +inf / -1 on a miss */
    int32_t light;                 /* shadow rays: the sampled light triangle; -1 otherwise */
    int32_t occluded;              /* shadow rays: the closest hit is not the light triangle */
} orc_ray_rec;                     /* 56 bytes */
int orc_render_counted(const orc_scene* s, const orc_camera* cam, int width, int height, int max_depth,
                       uint32_t first_sample, uint32_t spp, uint64_t seed, int rank, int world,
                       float* total, int64_t* counts, orc_ray_rec* rec, const int64_t* rec_offsets, int64_t rec_capacity, int threads);

/* orc_render that takes a CENSUS of the named arms of tex2d, test_triangle, closest_hit, shade, sample_about and
 * direct_illumination: arms[ORC_ARM_N], summed over the frame; orc_arm_name(i) names arm i.  Value classes that decide which code
 * runs are arms too (the class of |n.x| at each sampler site, texels that are exactly 0 or 1).  brute != 0: candidates in
 * ascending index order (the FLAT and PLAIN passes' order, which decides which tie arm a tie takes); 0: the oracle's tree walk.
 * total (may be NULL) is accumulated as orc_render does, bit for bit.  The result does not depend on the thread count. */
enum { ORC_TEX_MISSING = 0, ORC_TEX_HI_X, ORC_TEX_HI_Y, ORC_TEX_LO_X, ORC_TEX_LO_Y, ORC_TEX_PLAIN, ORC_TEX_ARMS };
enum { ORC_SA_BELOW = 0, ORC_SA_BAND, ORC_SA_POLE, ORC_SA_CLASSES };
enum {
    ORC_ARM_TEX = 0,                                    /* + slot * ORC_TEX_ARMS + ORC_TEX_*; slots as orc_material.tex */
    ORC_ARM_TRI_FARTHER = ORC_ARM_TEX + 6 * ORC_TEX_ARMS, ORC_ARM_TRI_NEARER, ORC_ARM_TRI_TIE_ACCEPTED, ORC_ARM_TRI_TIE_REJECTED,
    ORC_ARM_TRI_OPACITY_KEPT, ORC_ARM_TRI_OPACITY_DROPPED, ORC_ARM_WALK_STACK_FULL,
    ORC_ARM_SMOOTHING_ON, ORC_ARM_SMOOTHING_OFF, ORC_ARM_NORMAL_MAP_ON, ORC_ARM_NORMAL_MAP_OFF, ORC_ARM_NT_Z_CLAMPED,
    ORC_ARM_NORMAL_FLIPPED, ORC_ARM_TERMINAL, ORC_ARM_RR_ENGAGED, ORC_ARM_RR_CAP_ACTIVE, ORC_ARM_RR_KILLED_UNDER_THE_CAP_ONLY,
    ORC_ARM_RR_KILLED_OTHERWISE, ORC_ARM_RR_SURVIVED,
    ORC_ARM_OPAQUE_REFLECT_ROUGH_ONE, ORC_ARM_OPAQUE_REFLECT_MIRROR, ORC_ARM_OPAQUE_REFLECT_LOBE, ORC_ARM_OPAQUE_DIFFUSE,
    ORC_ARM_GLASS_ENTERED_OUTSIDE, ORC_ARM_GLASS_ENTERED_INSIDE, ORC_ARM_GLASS_ROUGH_NORMAL, ORC_ARM_GLASS_TIR,
    ORC_ARM_GLASS_FRESNEL_REFLECT, ORC_ARM_GLASS_REFLECTIVENESS_REFLECT, ORC_ARM_GLASS_REFLECT_ROUGH_ONE, ORC_ARM_GLASS_REFLECT_MIRROR,
    ORC_ARM_GLASS_REFLECT_LOBE, ORC_ARM_GLASS_REFRACT_TRANSMIT, ORC_ARM_GLASS_REFRACT_DIFFUSE,
    ORC_ARM_ROUGHNESS_TEXEL_ONE, ORC_ARM_ROUGHNESS_TEXEL_ZERO, ORC_ARM_REFLECTIVENESS_TEXEL_ZERO, ORC_ARM_REFLECTIVENESS_TEXEL_ONE,
    ORC_ARM_SA,                                         /* + site * ORC_SA_CLASSES + ORC_SA_*; sites in shade()'s order */
    ORC_ARM_DI_NO_LIGHTS = ORC_ARM_SA + 7 * ORC_SA_CLASSES, ORC_ARM_DI_LIGHT_ID_CLAMPED, ORC_ARM_DI_NDL_NOT_POSITIVE,
    ORC_ARM_DI_SHADOW_MISSED, ORC_ARM_DI_HIT_LIGHT, ORC_ARM_DI_HIT_OTHER,
    ORC_ARM_N
};
int orc_arm_count(void);
const char* orc_arm_name(int arm);
void orc_render_census(const orc_scene* s, const orc_camera* cam, int width, int height, int max_depth,
                       uint32_t first_sample, uint32_t spp, uint64_t seed, int brute, float* total, int64_t* arms, int threads);
/* Moeller-Trumbore of orc_intersect_triangle on n (ray, triangle) pairs: ro, rd [n][3], tri9 [n][9] -> out3 [n][3] */
void orc_intersect_many(int64_t n, const float* ro, const float* rd, const float* tri9, float* out3);

/* Primary ray directions before DOF, row-major top-down [H][W][3]; follows the incremental
 * `pixel += camRight*deltaX` arithmetic of pathtracer.cpp:755-766,782-785,814. */
void orc_primary_dirs(const orc_camera* cam, int width, int height, float* out);
int orc_render_tape(const orc_scene* s, const orc_camera* cam, int width, int height, int max_depth, const float* tape, int tape_len, float* total);
/* orc_render_tape that also ADDS the arms the replay takes to arms[ORC_ARM_N] (not zeroed here): the same image, the same draws */
int orc_render_tape_census(const orc_scene* s, const orc_camera* cam, int width, int height, int max_depth, const float* tape, int tape_len,
                           float* total, int64_t* arms);

/* Radiance of one path with the draws taken from `tape` (tier T).  Returns #draws consumed. */
int orc_trace_tape(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                   const float* tape, int tape_len, int mode, float* out3);
/* mode 0 = iterative form (what orc_render and the HIP kernel compute), 1 = recursive form with
 * DirectIllumimation evaluated before the recursive Trace, 2 = recursive, Trace first (the order
 * g++ picked for the reference build the fixtures were recorded from). */
/* orc_trace_tape that also ADDS the arms the replay takes to arms[ORC_ARM_N] (not zeroed here): the same radiance, the same draws */
int orc_trace_tape_census(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                          const float* tape, int tape_len, int mode, float* out3, int64_t* arms);
void orc_trace_counter(const orc_scene* s, const float* ro, const float* rd, int max_depth,
                       uint64_t seed, uint32_t pixel, uint32_t sample, int mode, float* out3);

/* Per-function probes (tier K) */
void orc_intersect_triangle(const float* ro, const float* rd, const float* v0, const float* v1,
                            const float* v2, float* out3);
int  orc_hit(const orc_scene* s, const float* ro, const float* rd, float* tuv, int32_t* tri);
int  orc_hit_brute(const orc_scene* s, const float* ro, const float* rd, float* tuv, int32_t* tri);
void orc_tex2d(const orc_scene* s, int tex, float u, float v, float* out4);
void orc_triangle_init(const float* in15, float* out9);
void orc_sincos(float a, float* s, float* c);
void orc_sincos_n(const float* a, int n, float* s, float* c);                                   /* orc_sincos on an array */
float orc_rand_u01(uint64_t seed, uint32_t pixel, uint32_t sample, int n);  /* n-th draw of a path */
void orc_sample_circle(float r1, float r2, float* out2);
int  orc_aabb_intersect(const float* bmin, const float* bmax, const float* ro, const float* rd);   /* AABB::Intersect */
void orc_aabb_build(const float* pts, int n, float* out6);                                         /* AABB::Build + Check */
void orc_direct_illumination_tape(const orc_scene* s, const float* p, const float* n, const float* diffuse, const float* tape3, float* out3);

/* traversal statistics of the oracle's own BVH (diagnostics only) */
void orc_bvh_info(const orc_scene* s, int32_t* nodes, int32_t* depth);

#ifdef __cplusplus
}
#endif
#endif
