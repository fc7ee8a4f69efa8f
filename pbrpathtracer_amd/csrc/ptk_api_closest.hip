// Host side of the ptk C-ABI: closest-point queries for caller-supplied points (ptk.h ptk_closest_points).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_closest.h"

using namespace ptk;

// The argument checks the entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_closest_args(ptk_ctx* c, const char* who, int32_t num_points, const float* points, bool have_out, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (num_points < 0) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": negative point count");
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!have_out) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": no output array");
    if (num_points > 0 && !points) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null array");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num_points == 0;
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory: h holds the points and the outputs, the scene
// half is filled in here.  One kernel between the two events; a scene without triangles has no tree to walk and gets its misses
// from fills.
static int closest_on_stream(ptk_ctx* c, ClosestParams& h)
{
    c->closest_timed = false;
    const size_t n = (size_t)h.num_points;
    if (c->num_nodes == 0)
    {
        if (h.tri) HIPCHK(c, hipMemsetAsync(h.tri, 0xff, n * sizeof(int32_t), c->stream));
        if (h.dist) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h.dist, 0x7f800000, n, c->stream));
        if (h.point) HIPCHK(c, hipMemsetAsync(h.point, 0, n * 3 * sizeof(float), c->stream));
        if (h.bary) HIPCHK(c, hipMemsetAsync(h.bary, 0, n * 2 * sizeof(float), c->stream));
        return PTK_OK;
    }
    h.nodes = c->d_nodes; h.tris = c->d_tris;
    h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound;
    if (const int rc = ensure_events(c, c->ev_closest); rc != PTK_OK) return rc;
    HIPCHK(c, hipEventRecord(c->ev_closest[0], c->stream));
    launch_closest(h, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_closest[1], c->stream));
    c->closest_timed = true;
    return PTK_OK;
}

extern "C" {

int ptk_closest_points_device(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, int32_t* d_tri, float* d_dist,
                              float* d_point, float* d_bary)
{
    bool nothing;
    const int rc = check_closest_args(c, "ptk_closest_points", num_points, d_points, d_tri || d_dist || d_point || d_bary, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    ClosestParams h = {};
    h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points;
    h.tri = d_tri; h.dist = d_dist; h.point = d_point; h.bary = d_bary;
    return closest_on_stream(c, h);
}

// The host entry: the points, the radii and the requested outputs staged for the length of the call
int ptk_closest_points(ptk_ctx* c, int32_t num_points, const float* points, const float* max_dist, int32_t* tri, float* dist, float* point,
                       float* bary)
{
    bool nothing;
    const int rc = check_closest_args(c, "ptk_closest_points", num_points, points, tri || dist || point || bary, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_points;
    Stage s(c);
    const auto d_points = s.in(points, 3 * n), d_max_dist = s.in(max_dist, n);
    const auto d_tri = s.out(tri, n);
    const auto d_dist = s.out(dist, n), d_point = s.out(point, 3 * n), d_bary = s.out(bary, 2 * n);
    return s.run([&] {
        ClosestParams h = {};
        h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points;
        h.tri = d_tri; h.dist = d_dist; h.point = d_point; h.bary = d_bary;
        return closest_on_stream(c, h);
    });
}

int ptk_last_closest_ms(ptk_ctx* c, float* ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t = 0.0f;
    if (c->closest_timed)
    {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventSynchronize(c->ev_closest[1]));
        HIPCHK(c, hipEventElapsedTime(&t, c->ev_closest[0], c->ev_closest[1]));
    }
    if (ms) *ms = t;
    return PTK_OK;
}

int ptk_closest_stats(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, uint64_t* node_visits, uint64_t* tri_tests)
{
    bool nothing;
    const int rc = check_closest_args(c, "ptk_closest_stats", num_points, d_points, node_visits || tri_tests, &nothing);
    if (rc != PTK_OK) return rc;
    unsigned long long got[2] = { 0, 0 };
    if (!nothing && c->num_nodes > 0)
    {
        HIPCHK(c, hipSetDevice(c->device));
        if (!c->d_closest_stats) HIPCHK(c, hipMalloc(&c->d_closest_stats, sizeof(got)));
        HIPCHK(c, hipMemsetAsync(c->d_closest_stats, 0, sizeof(got), c->stream));
        ClosestParams h = {};
        h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points;
        h.stats = c->d_closest_stats;
        h.nodes = c->d_nodes; h.tris = c->d_tris; h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound;
        launch_closest(h, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(got, c->d_closest_stats, sizeof(got), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    if (node_visits) *node_visits = got[0];
    if (tri_tests) *tri_tests = got[1];
    return PTK_OK;
}

}  // extern "C"
