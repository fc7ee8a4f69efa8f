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

// The call proper (query_on_stream): h holds the points and the outputs
static int closest_on_stream(ptk_ctx* c, ClosestParams& h)
{
    return query_on_stream(c, c->ev_closest, h, launch_closest, [&] {
        const size_t n = (size_t)h.num_points;
        if (h.tri) HIPCHK(c, hipMemsetAsync(h.tri, 0xff, n * sizeof(int32_t), c->stream));
        if (h.dist) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h.dist, 0x7f800000, n, c->stream));
        if (h.point) HIPCHK(c, hipMemsetAsync(h.point, 0, n * 3 * sizeof(float), c->stream));
        if (h.bary) HIPCHK(c, hipMemsetAsync(h.bary, 0, n * 2 * sizeof(float), c->stream));
        return (int)PTK_OK;
    });
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

int ptk_last_closest_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_closest, ms); }

int ptk_closest_stats(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, uint64_t* node_visits, uint64_t* tri_tests)
{
    bool nothing;
    const int rc = check_closest_args(c, "ptk_closest_stats", num_points, d_points, node_visits || tri_tests, &nothing);
    if (rc != PTK_OK) return rc;
    unsigned long long got[2] = { 0, 0 };
    ClosestParams h = {};
    h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points;
    if (const int rs = query_stats(c, nothing, c->d_closest_stats, h, launch_closest, got); rs != PTK_OK) return rs;
    if (node_visits) *node_visits = got[0];
    if (tri_tests) *tri_tests = got[1];
    return PTK_OK;
}

}  // extern "C"
