// Host side of the ptk C-ABI: closest-point queries for caller-supplied points (ptk.h ptk_closest_points).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_closest.h"

using namespace ptk;

// The argument checks the entries share: check_query_args with the word of these entries' texts.
static int check_closest_args(ptk_ctx* c, const char* who, int32_t num_points, const float* points, bool have_out, bool* nothing)
{
    return check_query_args(c, who, "point count", num_points, points, points, have_out, nothing);
}

// The call proper, on the context's stream, every pointer into this GPU's memory: h holds the points and the outputs, the scene
// half is filled in here.  One kernel between the two events; a scene without triangles has no tree to walk and gets its misses
// from fills.
static int closest_on_stream(ptk_ctx* c, ClosestParams& h)
{
    c->ev_closest.begin();
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
    if (const int rc = c->ev_closest.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch_closest(h, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rc = c->ev_closest.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_closest.done();
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
    return s.run([&] { return ptk_closest_points_device(c, num_points, d_points, d_max_dist, d_tri, d_dist, d_point, d_bary); });
}

int ptk_last_closest_ms(ptk_ctx* c, float* ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t = 0.0f;
    const int rc = c->ev_closest.elapsed(c, 0, 1, &t);
    if (ms) *ms = t;
    return rc;
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
        if (!c->d_closest_stats) HIPCHK(c, hipMalloc(&c->d_closest_stats.p, sizeof(got)));
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
