// Host side of the ptk C-ABI: crossing counts, point containment and a signed distance (ptk.h ptk_crossings_rays,
// ptk_contains_points, ptk_signed_distance).
#include <hip/hip_runtime.h>

#include <cstring>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_closest.h"
#include "ptk_crossings.h"

using namespace ptk;

static const float k_default_dirs[9] = PTK_INSIDE_DEFAULT_DIRS;

// The argument checks the entries share: check_query_args with the word of these entries' texts.
static int check_cross_args(ptk_ctx* c, const char* who, int32_t num, const void* a, const void* b, bool have_out, bool* nothing)
{
    return check_query_args(c, who, "count", num, a, b, have_out, nothing);
}

// ... and what the containment entries add: the direction set and the mode
static int check_dirs_args(ptk_ctx* c, const char* who, int32_t num_dirs, const float* dirs, int32_t mode)
{
    if (num_dirs < 1 || num_dirs > 31 || num_dirs % 2 == 0) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": num_dirs must be odd and in 1 .. 31");
    if (!dirs && num_dirs != 3) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": the built-in direction set has 3 directions");
    if (mode != PTK_INSIDE_WINDING && mode != PTK_INSIDE_PARITY) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": unknown mode");
    return PTK_OK;
}

static void scene_half(ptk_ctx* c, CrossingsParams& h)
{
    h.nodes = c->d_nodes; h.tris = c->d_tris; h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound; h.tri_thr = c->opt_tri_thr;
}

// The calls proper, on the context's stream, every pointer into this GPU's memory.  The kernels of a call between the two events;
// a scene without triangles has no tree to walk and gets its zeros (and the closest-point misses) from fills.
static int crossings_on_stream(ptk_ctx* c, CrossingsParams& h)
{
    c->ev_crossings.begin();
    const size_t n = (size_t)h.num;
    if (c->num_nodes == 0)
    {
        if (h.front) HIPCHK(c, hipMemsetAsync(h.front, 0, n * sizeof(int32_t), c->stream));
        if (h.back) HIPCHK(c, hipMemsetAsync(h.back, 0, n * sizeof(int32_t), c->stream));
        return PTK_OK;
    }
    scene_half(c, h);
    if (const int rc = c->ev_crossings.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch_crossings(h, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rc = c->ev_crossings.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_crossings.done();
    return PTK_OK;
}

// `closest`: null, or ptk_signed_distance's closest-point query, which runs first; then h.dist is its dist
static int contains_on_stream(ptk_ctx* c, CrossingsParams& h, ClosestParams* closest)
{
    c->ev_crossings.begin();
    const size_t n = (size_t)h.num;
    if (c->num_nodes == 0)
    {
        if (h.inside) HIPCHK(c, hipMemsetAsync(h.inside, 0, n, c->stream));
        if (h.winding) HIPCHK(c, hipMemsetAsync(h.winding, 0, n * (size_t)h.num_dirs * sizeof(int32_t), c->stream));
        if (closest)
        {
            if (closest->tri) HIPCHK(c, hipMemsetAsync(closest->tri, 0xff, n * sizeof(int32_t), c->stream));
            if (closest->dist) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)closest->dist, 0x7f800000, n, c->stream));
            if (closest->point) HIPCHK(c, hipMemsetAsync(closest->point, 0, n * 3 * sizeof(float), c->stream));
            if (closest->bary) HIPCHK(c, hipMemsetAsync(closest->bary, 0, n * 2 * sizeof(float), c->stream));
        }
        return PTK_OK;
    }
    scene_half(c, h);
    if (const int rc = c->ev_crossings.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    if (closest)
    {
        closest->nodes = c->d_nodes; closest->tris = c->d_tris; closest->num_nodes = c->num_nodes; closest->scene_bound = c->scene_bound;
        launch_closest(*closest, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (!closest || h.dist)                          // (a signed distance without dist is a closest-point query)
    {
        launch_contains(h, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (const int rc = c->ev_crossings.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_crossings.done();
    return PTK_OK;
}

extern "C" {

int ptk_inside_default_dirs(float out[3][3])
{
    if (!out) return PTK_ERR_BAD_ARG;
    std::memcpy(out, k_default_dirs, sizeof(k_default_dirs));
    return PTK_OK;
}

int ptk_crossings_rays_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, const float* d_tmax, int32_t* d_front,
                              int32_t* d_back)
{
    bool nothing;
    const int rc = check_cross_args(c, "ptk_crossings_rays", num_rays, d_origins, d_dirs, d_front || d_back, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    CrossingsParams h = {};
    h.origins = d_origins; h.dirs = d_dirs; h.tmax = d_tmax; h.num = num_rays; h.front = d_front; h.back = d_back;
    return crossings_on_stream(c, h);
}

int ptk_crossings_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, const float* tmax, int32_t* front, int32_t* back)
{
    bool nothing;
    const int rc = check_cross_args(c, "ptk_crossings_rays", num_rays, origins, dirs, front || back, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_rays;
    Stage s(c);
    const auto d_origins = s.in(origins, 3 * n), d_dirs = s.in(dirs, 3 * n), d_tmax = s.in(tmax, n);
    const auto d_front = s.out(front, n), d_back = s.out(back, n);
    return s.run([&] { return ptk_crossings_rays_device(c, num_rays, d_origins, d_dirs, d_tmax, d_front, d_back); });
}

int ptk_contains_points_device(ptk_ctx* c, int32_t num_points, const float* d_points, int32_t num_dirs, const float* d_dirs, int32_t mode,
                               uint8_t* d_inside, int32_t* d_winding)
{
    bool nothing;
    int rc = check_cross_args(c, "ptk_contains_points", num_points, d_points, d_points, d_inside || d_winding, &nothing);
    if (rc == PTK_OK) rc = check_dirs_args(c, "ptk_contains_points", num_dirs, d_dirs, mode);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    CrossingsParams h = {};
    h.origins = d_points; h.dirs = d_dirs; h.num = num_points; h.num_dirs = num_dirs; h.mode = mode; h.inside = d_inside; h.winding = d_winding;
    return contains_on_stream(c, h, nullptr);
}

int ptk_contains_points(ptk_ctx* c, int32_t num_points, const float* points, int32_t num_dirs, const float* dirs, int32_t mode, uint8_t* inside,
                        int32_t* winding)
{
    bool nothing;
    int rc = check_cross_args(c, "ptk_contains_points", num_points, points, points, inside || winding, &nothing);
    if (rc == PTK_OK) rc = check_dirs_args(c, "ptk_contains_points", num_dirs, dirs, mode);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_points;
    Stage s(c);
    const auto d_points = s.in(points, 3 * n), d_dirs = s.in(dirs, 3 * (size_t)num_dirs);
    const auto d_inside = s.out(inside, n);
    const auto d_winding = s.out(winding, n * (size_t)num_dirs);
    return s.run([&] { return ptk_contains_points_device(c, num_points, d_points, num_dirs, d_dirs, mode, d_inside, d_winding); });
}

int ptk_signed_distance_device(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, int32_t num_dirs, const float* d_dirs,
                               int32_t mode, int32_t* d_tri, float* d_dist, float* d_point, float* d_bary)
{
    bool nothing;
    int rc = check_cross_args(c, "ptk_signed_distance", num_points, d_points, d_points, d_tri || d_dist || d_point || d_bary, &nothing);
    if (rc == PTK_OK) rc = check_dirs_args(c, "ptk_signed_distance", num_dirs, d_dirs, mode);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ClosestParams q = {};
    q.points = d_points; q.max_dist = d_max_dist; q.num_points = num_points; q.tri = d_tri; q.dist = d_dist; q.point = d_point; q.bary = d_bary;
    CrossingsParams h = {};
    h.origins = d_points; h.dirs = d_dirs; h.num = num_points; h.num_dirs = num_dirs; h.mode = mode; h.dist = d_dist;
    return contains_on_stream(c, h, &q);
}

int ptk_signed_distance(ptk_ctx* c, int32_t num_points, const float* points, const float* max_dist, int32_t num_dirs, const float* dirs, int32_t mode,
                        int32_t* tri, float* dist, float* point, float* bary)
{
    bool nothing;
    int rc = check_cross_args(c, "ptk_signed_distance", num_points, points, points, tri || dist || point || bary, &nothing);
    if (rc == PTK_OK) rc = check_dirs_args(c, "ptk_signed_distance", num_dirs, dirs, mode);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_points;
    Stage s(c);
    const auto d_points = s.in(points, 3 * n), d_max_dist = s.in(max_dist, n), d_dirs = s.in(dirs, 3 * (size_t)num_dirs);
    const auto d_tri = s.out(tri, n);
    const auto d_dist = s.out(dist, n), d_point = s.out(point, 3 * n), d_bary = s.out(bary, 2 * n);
    return s.run([&] { return ptk_signed_distance_device(c, num_points, d_points, d_max_dist, num_dirs, d_dirs, mode, d_tri, d_dist, d_point, d_bary); });
}

int ptk_last_crossings_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_crossings, ms); }

}  // extern "C"
