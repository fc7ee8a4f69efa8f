// Host side of the ptk C-ABI: overlap queries for caller-supplied boxes and spheres (ptk.h ptk_overlap_boxes).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_overlap.h"

using namespace ptk;

// The argument checks the entries share: check_query_args, k and the outputs that k asks for.
static int check_overlap_args(ptk_ctx* c, const char* who, int32_t num, const void* a, const void* b, int32_t k, const void* count, const void* list,
                              bool* nothing)
{
    const std::string range = "k must be in 0 .. " + std::to_string(PTK_OVERLAP_MAX_K);
    const char* also = (k < 0 || k > PTK_OVERLAP_MAX_K) ? range.c_str() : ((k > 0 && !list) ? "k > 0 needs tris" : nullptr);
    return check_query_args(c, who, "query count", num, a, b, k > 0 ? (count || list) : count != nullptr, nothing, also);
}

// The call proper (query_on_stream): h holds the queries and the outputs; the fills are the zeros and -1s
static int overlap_on_stream(ptk_ctx* c, OverlapParams& h)
{
    return query_on_stream(c, c->ev_overlap, h, launch_overlap, [&] {
        const size_t n = (size_t)h.num;
        if (h.count) HIPCHK(c, hipMemsetAsync(h.count, 0, n * sizeof(int32_t), c->stream));
        if (h.list && h.k > 0) HIPCHK(c, hipMemsetAsync(h.list, 0xff, n * (size_t)h.k * sizeof(int32_t), c->stream));
        return (int)PTK_OK;
    });
}

static int overlap_device(ptk_ctx* c, const char* who, int shape, int32_t num, const float* d_a, const float* d_b, const int32_t* d_tri_from, int32_t k,
                          int32_t* d_count, int32_t* d_tris)
{
    bool nothing;
    const int rc = check_overlap_args(c, who, num, d_a, d_b, k, d_count, d_tris, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    OverlapParams h = {};
    h.qa = d_a; h.qb = d_b; h.tri_from = d_tri_from; h.num = num; h.k = k; h.shape = shape;
    h.count = d_count; h.list = k > 0 ? d_tris : nullptr;
    return overlap_on_stream(c, h);
}

// The host entries: the queries and the requested outputs staged for the length of the call (nb: floats of the second array per query)
static int overlap_host(ptk_ctx* c, const char* who, int shape, int32_t num, const float* a, const float* b, const int32_t* tri_from, int32_t k,
                        int32_t* count, int32_t* tris)
{
    bool nothing;
    const int rc = check_overlap_args(c, who, num, a, b, k, count, tris, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num, nb = shape == OVERLAP_BOX ? 3 : 1;
    Stage s(c);
    const auto d_a = s.in(a, 3 * n), d_b = s.in(b, nb * n);
    const auto d_from = s.in(tri_from, n);
    const auto d_count = s.out(count, n), d_tris = s.out(k > 0 ? tris : nullptr, n * (size_t)k);
    return s.run([&] { return overlap_device(c, who, shape, num, d_a, d_b, d_from, k, d_count, d_tris); });
}

extern "C" {

int ptk_overlap_boxes_device(ptk_ctx* c, int32_t num, const float* d_lo, const float* d_hi, const int32_t* d_tri_from, int32_t k, int32_t* d_count,
                             int32_t* d_tris)
{
    return overlap_device(c, "ptk_overlap_boxes", OVERLAP_BOX, num, d_lo, d_hi, d_tri_from, k, d_count, d_tris);
}

int ptk_overlap_spheres_device(ptk_ctx* c, int32_t num, const float* d_centers, const float* d_radius, const int32_t* d_tri_from, int32_t k,
                               int32_t* d_count, int32_t* d_tris)
{
    return overlap_device(c, "ptk_overlap_spheres", OVERLAP_SPHERE, num, d_centers, d_radius, d_tri_from, k, d_count, d_tris);
}

int ptk_overlap_boxes(ptk_ctx* c, int32_t num, const float* lo, const float* hi, const int32_t* tri_from, int32_t k, int32_t* count, int32_t* tris)
{
    return overlap_host(c, "ptk_overlap_boxes", OVERLAP_BOX, num, lo, hi, tri_from, k, count, tris);
}

int ptk_overlap_spheres(ptk_ctx* c, int32_t num, const float* centers, const float* radius, const int32_t* tri_from, int32_t k, int32_t* count,
                        int32_t* tris)
{
    return overlap_host(c, "ptk_overlap_spheres", OVERLAP_SPHERE, num, centers, radius, tri_from, k, count, tris);
}

int ptk_last_overlap_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_overlap, ms); }

int ptk_overlap_stats(ptk_ctx* c, int32_t shape, int32_t num, const float* d_a, const float* d_b, const int32_t* d_tri_from, uint64_t stats[4])
{
    bool nothing;
    const int rc = check_query_args(c, "ptk_overlap_stats", "query count", num, d_a, d_b, stats != nullptr, &nothing,
                                    (shape != PTK_OVERLAP_BOX && shape != PTK_OVERLAP_SPHERE) ? "unknown shape" : nullptr);
    if (rc != PTK_OK) return rc;
    unsigned long long got[4] = { 0, 0, 0, 0 };
    OverlapParams h = {};
    h.qa = d_a; h.qb = d_b; h.tri_from = d_tri_from; h.num = num; h.shape = shape == PTK_OVERLAP_BOX ? OVERLAP_BOX : OVERLAP_SPHERE;
    if (const int rs = query_stats(c, nothing, c->d_overlap_stats, h, launch_overlap, got); rs != PTK_OK) return rs;
    for (int j = 0; j < 4; j++) stats[j] = got[j];
    return PTK_OK;
}

}  // extern "C"
