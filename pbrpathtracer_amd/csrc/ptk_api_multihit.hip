// Host side of the ptk C-ABI: ordered multi-hit ray queries (ptk.h ptk_multihit_rays).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_multihit.h"

using namespace ptk;

// The shared argument checks (check_query_args) and max_hits
static int check_multihit_args(ptk_ctx* c, int32_t num, const void* origins, const void* dirs, int32_t max_hits, bool have_out, bool* nothing)
{
    const std::string range = "max_hits must be in 1 .. " + std::to_string(PTK_MULTIHIT_MAX);
    return check_query_args(c, "ptk_multihit_rays", "count", num, origins, dirs, have_out, nothing,
                            (max_hits < 1 || max_hits > PTK_MULTIHIT_MAX) ? range.c_str() : nullptr);
}

// The call proper, on the context's stream, every pointer into this GPU's memory.  The kernel between the two events; a scene
// without triangles has no tree to walk and gets its unused-slot values from fills.
static int multihit_on_stream(ptk_ctx* c, MultihitParams& h)
{
    c->ev_multihit.begin();
    const size_t n = (size_t)h.num, nk = n * (size_t)h.max_hits;
    if (c->num_nodes == 0)
    {
        if (h.count) HIPCHK(c, hipMemsetAsync(h.count, 0, n * sizeof(int32_t), c->stream));
        if (h.tri) HIPCHK(c, hipMemsetAsync(h.tri, 0xff, nk * sizeof(int32_t), c->stream));
        if (h.t) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h.t, 0x7f800000, nk, c->stream));
        if (h.bary) HIPCHK(c, hipMemsetAsync(h.bary, 0, nk * 2 * sizeof(float), c->stream));
        if (h.side) HIPCHK(c, hipMemsetAsync(h.side, 0, nk, c->stream));
        return PTK_OK;
    }
    h.nodes = c->d_nodes; h.tris = c->d_tris; h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound; h.tri_thr = c->opt_tri_thr;
    if (const int rc = c->ev_multihit.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch_multihit(h, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rc = c->ev_multihit.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_multihit.done();
    return PTK_OK;
}

extern "C" {

int ptk_multihit_rays_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, const float* d_tmax, int32_t max_hits,
                             int32_t* d_count, int32_t* d_tri, float* d_t, float* d_bary, int8_t* d_side)
{
    bool nothing;
    const int rc = check_multihit_args(c, num_rays, d_origins, d_dirs, max_hits, d_count || d_tri || d_t || d_bary || d_side, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    MultihitParams h = {};
    h.origins = d_origins; h.dirs = d_dirs; h.tmax = d_tmax; h.num = num_rays; h.max_hits = max_hits;
    h.count = d_count; h.tri = d_tri; h.t = d_t; h.bary = d_bary; h.side = d_side;
    return multihit_on_stream(c, h);
}

int ptk_multihit_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, const float* tmax, int32_t max_hits, int32_t* count,
                      int32_t* tri, float* t, float* bary, int8_t* side)
{
    bool nothing;
    const int rc = check_multihit_args(c, num_rays, origins, dirs, max_hits, count || tri || t || bary || side, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_rays, nk = n * (size_t)max_hits;
    Stage s(c);
    const auto d_origins = s.in(origins, 3 * n), d_dirs = s.in(dirs, 3 * n), d_tmax = s.in(tmax, n);
    const auto d_count = s.out(count, n), d_tri = s.out(tri, nk);
    const auto d_t = s.out(t, nk), d_bary = s.out(bary, 2 * nk);
    const auto d_side = s.out(side, nk);
    return s.run([&] { return ptk_multihit_rays_device(c, num_rays, d_origins, d_dirs, d_tmax, max_hits, d_count, d_tri, d_t, d_bary, d_side); });
}

int ptk_last_multihit_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_multihit, ms); }

}  // extern "C"
