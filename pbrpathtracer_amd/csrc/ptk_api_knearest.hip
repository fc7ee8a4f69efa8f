// Host side of the ptk C-ABI: K-nearest triangle queries for caller-supplied points (ptk.h ptk_nearest_triangles).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_knearest.h"

using namespace ptk;

// The shared argument checks (check_query_args) and k
static int check_nearest_args(ptk_ctx* c, const char* who, int32_t num_points, const void* points, int32_t k, bool have_out, bool* nothing)
{
    const std::string range = "k must be in 1 .. " + std::to_string(PTK_NEAREST_MAX_K);
    return check_query_args(c, who, "point count", num_points, points, points, have_out, nothing,
                            (k < 1 || k > PTK_NEAREST_MAX_K) ? range.c_str() : nullptr);
}

// The call proper (query_on_stream): h holds the points, k and the outputs; the fills are the unused-slot values
static int nearest_on_stream(ptk_ctx* c, NearestParams& h)
{
    return query_on_stream(c, c->ev_nearest, h, launch_nearest, [&] {
        const size_t n = (size_t)h.num_points, nk = n * (size_t)h.k;
        if (h.count) HIPCHK(c, hipMemsetAsync(h.count, 0, n * sizeof(int32_t), c->stream));
        if (h.tri) HIPCHK(c, hipMemsetAsync(h.tri, 0xff, nk * sizeof(int32_t), c->stream));
        if (h.dist) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h.dist, 0x7f800000, nk, c->stream));
        if (h.point) HIPCHK(c, hipMemsetAsync(h.point, 0, nk * 3 * sizeof(float), c->stream));
        if (h.bary) HIPCHK(c, hipMemsetAsync(h.bary, 0, nk * 2 * sizeof(float), c->stream));
        return (int)PTK_OK;
    });
}

extern "C" {

int ptk_nearest_triangles_device(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, int32_t k, int32_t* d_count,
                                 int32_t* d_tri, float* d_dist, float* d_point, float* d_bary)
{
    bool nothing;
    const int rc = check_nearest_args(c, "ptk_nearest_triangles", num_points, d_points, k, d_count || d_tri || d_dist || d_point || d_bary, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    NearestParams h = {};
    h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points; h.k = k;
    h.count = d_count; h.tri = d_tri; h.dist = d_dist; h.point = d_point; h.bary = d_bary;
    return nearest_on_stream(c, h);
}

// The host entry: the points, the radii and the requested outputs staged for the length of the call
int ptk_nearest_triangles(ptk_ctx* c, int32_t num_points, const float* points, const float* max_dist, int32_t k, int32_t* count, int32_t* tri,
                          float* dist, float* point, float* bary)
{
    bool nothing;
    const int rc = check_nearest_args(c, "ptk_nearest_triangles", num_points, points, k, count || tri || dist || point || bary, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_points, nk = n * (size_t)k;
    Stage s(c);
    const auto d_points = s.in(points, 3 * n), d_max_dist = s.in(max_dist, n);
    const auto d_count = s.out(count, n), d_tri = s.out(tri, nk);
    const auto d_dist = s.out(dist, nk), d_point = s.out(point, 3 * nk), d_bary = s.out(bary, 2 * nk);
    return s.run([&] { return ptk_nearest_triangles_device(c, num_points, d_points, d_max_dist, k, d_count, d_tri, d_dist, d_point, d_bary); });
}

int ptk_last_nearest_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_nearest, ms); }

int ptk_nearest_stats(ptk_ctx* c, int32_t num_points, const float* d_points, const float* d_max_dist, int32_t k, uint64_t* node_visits,
                      uint64_t* tri_tests)
{
    bool nothing;
    const int rc = check_nearest_args(c, "ptk_nearest_stats", num_points, d_points, k, node_visits || tri_tests, &nothing);
    if (rc != PTK_OK) return rc;
    unsigned long long got[2] = { 0, 0 };
    NearestParams h = {};
    h.points = d_points; h.max_dist = d_max_dist; h.num_points = num_points; h.k = k;
    if (const int rs = query_stats(c, nothing, c->d_nearest_stats, h, launch_nearest, got); rs != PTK_OK) return rs;
    if (node_visits) *node_visits = got[0];
    if (tri_tests) *tri_tests = got[1];
    return PTK_OK;
}

}  // extern "C"
