// Host side of the ptk C-ABI: geometry updates after ptk_upload_scene - staging, record repack and BVH refit (ptk.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstring>

#include "ptk_ctx.h"
#include "ptk_refit.h"

using namespace ptk;

namespace {

static double* geo_cost_ptr(ptk_ctx* c) { return reinterpret_cast<double*>(c->d_geo_red + GEO_RED_WORDS); }

// the refit, deepest level first, then the SAH sum; each level is one launch and stream order is the barrier between them
static void queue_refit(ptk_ctx* c, float pad, int write_nodes, hipStream_t stream)
{
    for (int l = (int)c->level_start.size() - 2; l >= 0; l--)
        launch_refit_level(c->d_level_nodes + c->level_start[l], c->level_start[l + 1] - c->level_start[l], c->d_nodes, c->d_tris, c->d_verts_res,
                           c->d_refit_side, pad, write_nodes, stream);
    launch_refit_cost(c->d_refit_side, c->num_nodes, c->d_refit_partial, geo_cost_ptr(c), stream);
}

// Once per topology: each node's level and the per-level node lists (from a one-off download of the links: both builders number
// children after their parents, so one ascending sweep assigns every level), the inverse of the leaf order (on the device) and
// the SAH cost of the tree as built (a refit pass over the uploaded vertices that writes no node).
static int ensure_refit_topology(ptk_ctx* c)
{
    if (c->d_level_nodes) return PTK_OK;
    const int nn = c->num_nodes, nt = c->num_tris;
    if (nn <= 0 || nt <= 0 || !c->d_verts_res) return fail(c, PTK_ERR_BAD_ARG, "the uploaded scene has no triangles");
    std::vector<float> nodes((size_t)nn * NODE_F4 * 4);
    HIPCHK(c, hipStreamSynchronize(c->stream));
    HIPCHK(c, hipMemcpy(nodes.data(), c->d_nodes, nodes.size() * sizeof(float), hipMemcpyDeviceToHost));
    std::vector<int32_t> level((size_t)nn, -1);
    level[0] = 0;
    int levels = 1;
    for (int id = 0; id < nn; id++)
    {
        if (level[id] < 0) return fail(c, PTK_ERR_LIMIT, "refit: a node no parent links to");
        int32_t link[4];
        std::memcpy(link, &nodes[(size_t)id * 16 + 6], sizeof(link));
        bool open = true;
        for (int k = 0; k < 4; k++)
        {
            const int32_t l = link[k];
            if (l == NODE_EXIT) { open = false; continue; }
            if (!open) return fail(c, PTK_ERR_LIMIT, "refit: child slots not filled from the first");
            if (l >= 0)
            {
                if (l <= id || l >= nn || level[l] >= 0) return fail(c, PTK_ERR_LIMIT, "refit: a link that does not point forward to a node of its own");
                level[l] = level[id] + 1;
                levels = std::max(levels, level[l] + 1);
            }
            else if ((int64_t)((~l) >> 3) + ((~l) & 7) + 1 > (int64_t)nt) return fail(c, PTK_ERR_LIMIT, "refit: a leaf outside the triangle records");
        }
    }
    std::vector<int> start((size_t)levels + 1, 0);
    for (int id = 0; id < nn; id++) start[(size_t)level[id] + 1]++;
    for (int l = 0; l < levels; l++) start[(size_t)l + 1] += start[l];
    std::vector<int32_t> list((size_t)nn);
    {
        std::vector<int> fill(start.begin(), start.end() - 1);
        for (int id = 0; id < nn; id++) list[(size_t)fill[level[id]]++] = id;
    }
    hipError_t e = hipMalloc(&c->d_level_nodes.p, (size_t)nn * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&c->d_refit_partial.p, ((size_t)nn + 255) / 256 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&c->d_tri_pos.p, (size_t)nt * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&c->d_refit_side.p, (size_t)nn * 2 * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(c->d_level_nodes, list.data(), (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(c->d_tri_pos, 0, (size_t)nt * sizeof(int32_t), c->stream);
    if (e != hipSuccess)
    {
        c->d_level_nodes.release(); c->d_tri_pos.release(); c->d_refit_side.release(); c->d_refit_partial.release();
        return fail(c, PTK_ERR_HIP, std::string("refit tables: ") + hipGetErrorString(e));
    }
    c->level_start = start;
    launch_inverse_order(c->d_tris, c->d_tri_pos, nt, c->stream);
    queue_refit(c, c->bvh_pad, 0, c->stream);
    HIPCHK(c, hipGetLastError());
    double cost = 0.0;
    HIPCHK(c, hipMemcpyAsync(&cost, geo_cost_ptr(c), sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->sah_built = c->sah_now = cost;
    c->sah_now_pending = false;
    return PTK_OK;
}

static inline float geo_dec(uint32_t e) { const uint32_t u = (e & 0x80000000u) ? (e & 0x7fffffffu) : ~e; float f; std::memcpy(&f, &u, 4); return f; }

static int update_geometry(ptk_ctx* c, int32_t first, int32_t count, const float* verts, const float* normals, const float* tbn, bool on_device)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (first < 0 || count < 0 || (int64_t)first + (int64_t)count > (int64_t)c->num_tris)
        return fail(c, PTK_ERR_BAD_ARG, "triangle range outside the uploaded scene");
    if ((normals == nullptr) != (tbn == nullptr)) return fail(c, PTK_ERR_BAD_ARG, "normals and tbn go together: both, or neither to move vertices only");
    if (count == 0) return PTK_OK;
    if (!verts) return fail(c, PTK_ERR_BAD_ARG, "null vertex array");
    const char* limit_msg = "vertex coordinate is not finite or exceeds 2^61: the scene is unchanged";
    const size_t per = (size_t)count * 9;
    if (!on_device)
        for (size_t i = 0; i < per; i++)
            if (!(std::fabs(verts[i]) < 2.305843e18f)) return fail(c, PTK_ERR_LIMIT, limit_msg);
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_refit_topology(c);
    if (rc != PTK_OK) return rc;

    // 1. stage the arrays and find the bounds the scene WOULD have, on a stream of their own: nothing resident is written yet
    const size_t floats = per * (normals ? 3 : 1);
    if (floats > c->d_geo_stage.cap)
    {
        if (c->ev_geo_t.timed) HIPCHK(c, hipEventSynchronize(c->ev_geo_t.ev[4]));    // (the previous update's repack reads the old buffer)
        if (rc = c->d_geo_stage.alloc(c, floats); rc != PTK_OK) return rc;
    }
    float* sv = c->d_geo_stage; float* sn = normals ? sv + per : nullptr; float* st = normals ? sv + 2 * per : nullptr;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (c->ev_geo_t.timed) HIPCHK(c, hipStreamWaitEvent(c->geo_stream, c->ev_geo_t.ev[4], 0));
    HIPCHK(c, hipEventRecord(c->ev_geo_t.ev[0], c->geo_stream));
    HIPCHK(c, hipMemcpyAsync(sv, verts, per * sizeof(float), kind, c->geo_stream));
    if (normals)
    {
        HIPCHK(c, hipMemcpyAsync(sn, normals, per * sizeof(float), kind, c->geo_stream));
        HIPCHK(c, hipMemcpyAsync(st, tbn, per * sizeof(float), kind, c->geo_stream));
    }
    HIPCHK(c, hipMemsetAsync(c->d_geo_red, 0, GEO_RED_WORDS * sizeof(uint32_t), c->geo_stream));
    launch_geometry_bounds(c->d_verts_res, sv, first, count, c->num_tris, c->d_geo_red, c->geo_stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(c->h_geo_red, c->d_geo_red, GEO_RED_WORDS * sizeof(uint32_t), hipMemcpyDeviceToHost, c->geo_stream));
    HIPCHK(c, hipEventRecord(c->ev_geo_t.ev[1], c->geo_stream));
    // the one host wait of an update: for the staging stream, which stands behind the PREVIOUS update only - renders queued
    // since then are not waited for; the caller's arrays are free again from here on
    HIPCHK(c, hipStreamSynchronize(c->geo_stream));
    const uint32_t* red = c->h_geo_red;
    if (red[7]) return fail(c, PTK_ERR_LIMIT, limit_msg);
    float vmax; std::memcpy(&vmax, &red[6], 4);

    // 2. rewrite on the context's stream: behind every render already queued - their accumulate kernels are on this stream,
    // each behind its trace kernel on the internal streams, so no trace still reads the old records - and ahead of every
    // later one (inputs_dirty re-anchors the trace streams behind these kernels)
    HIPCHK(c, hipEventRecord(c->ev_geo_t.ev[2], c->stream));
    launch_repack_geometry(sv, sn, st, first, count, c->d_verts_res, c->d_tri_pos, c->d_tris, c->d_flat_tris, c->d_shade, c->stream);
    launch_repack_lights(c->d_verts_res, first, count, c->d_lights, c->num_lights, c->stream);
    if (c->d_flat_tris && sn) launch_flat_frames(c->d_shade, c->d_flat_tris, first, count, c->stream);     // (vertices only: the normals stay)
    if (c->d_flat_tris) launch_flat_classes(c->d_flat_tris, c->num_tris, c->opt_flat_zero_classes, c->opt_flat_rect_pairs, c->stream);   // the records' new zero words and pairs
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_geo_t.ev[3], c->stream));
    c->bvh_pad = 1e-5f * std::max(vmax, 1.0f);
    queue_refit(c, c->bvh_pad, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_geo_t.ev[4], c->stream));
    c->ev_geo_t.done();

    c->scene_bound = 3.1f * (1.01f * vmax + 1e-3f);
    for (int a = 0; a < 3; a++) { c->scene_lo[a] = geo_dec(~red[a]); c->scene_hi[a] = geo_dec(red[3 + a]); }
    if (c->num_lights > 0) c->lights_stale = true;
    c->geo_updates++;
    c->sah_now_pending = true;
    c->surf_valid = false;                       // (ptk_sample_surface rebuilds its table behind these kernels)
    c->view_generation++;
    c->primary_hit_dirty = true;
    c->out_full_next = true;
    c->inputs_dirty = true;
    return PTK_OK;
}

}  // namespace

extern "C" {

int ptk_update_geometry(ptk_ctx* c, int32_t first_tri, int32_t num_tris, const float* verts, const float* normals, const float* tbn)
{
    return update_geometry(c, first_tri, num_tris, verts, normals, tbn, false);
}

int ptk_update_geometry_device(ptk_ctx* c, int32_t first_tri, int32_t num_tris, const float* d_verts, const float* d_normals, const float* d_tbn)
{
    return update_geometry(c, first_tri, num_tris, d_verts, d_normals, d_tbn, true);
}

int ptk_geometry_info(ptk_ctx* c, uint32_t* updates, int* refitted, double* sah_built, double* sah_now)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    if ((sah_built || sah_now) && c->num_tris > 0)
    {
        const int rc = ensure_refit_topology(c);
        if (rc != PTK_OK) return rc;
        if (c->sah_now_pending)
        {
            double cost = 0.0;
            HIPCHK(c, hipMemcpyAsync(&cost, geo_cost_ptr(c), sizeof(double), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->sah_now = cost; c->sah_now_pending = false;
        }
    }
    if (updates) *updates = c->geo_updates;
    if (refitted) *refitted = c->geo_updates > 0 ? 1 : 0;
    if (sah_built) *sah_built = c->sah_built;
    if (sah_now) *sah_now = c->sah_now;
    return PTK_OK;
}

int ptk_geometry_timing(ptk_ctx* c, float* ms3)
{
    if (!c || !ms3) return PTK_ERR_BAD_ARG;
    if (!c->ev_geo_t.timed) return fail(c, PTK_ERR_BAD_ARG, "no geometry update yet");
    // (the last interval first: its end is the newest event, behind which the others have happened)
    int rc = c->ev_geo_t.elapsed(c, 3, 4, &ms3[2]);
    if (rc == PTK_OK) rc = c->ev_geo_t.elapsed(c, 0, 1, &ms3[0]);
    if (rc == PTK_OK) rc = c->ev_geo_t.elapsed(c, 2, 3, &ms3[1]);
    return rc;
}

}  // extern "C"
