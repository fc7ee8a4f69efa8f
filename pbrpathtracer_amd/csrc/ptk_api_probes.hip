// Host side of the ptk C-ABI: irradiance probes - the SH9 bake and the lookup (ptk.h), the depth moments and the
// lookup that weights the probes by them.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_probes.h"
#include "ptk_hits.h"

using namespace ptk;

extern "C" {

static int check_probes_args(ptk_ctx* c, int32_t num_probes, const float* positions, int32_t num_dirs, const float* dirs, uint32_t flags, float weight,
                             const float* radiance, const float* coefs, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (flags & ~PTK_PROBES_ACCUMULATE) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: unknown flag bits");
    if (num_probes < 0 || num_dirs < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: negative count");
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!std::isfinite(weight)) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: weight must be finite");
    if ((flags & PTK_PROBES_ACCUMULATE) && !radiance) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: PTK_PROBES_ACCUMULATE needs a radiance table");
    if (num_probes > 0)
    {
        if (num_dirs < 1 || num_dirs > 65536) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: num_dirs must be in 1..65536");
        if ((uint64_t)num_probes * (uint64_t)num_dirs >= (1ull << 31)) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: 2^31 rays or more");
        if (!positions || !dirs || !coefs) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probes: null array");
    }
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num_probes == 0;
    return PTK_OK;
}

// The bake proper, on the context's stream, every pointer into this GPU's memory: the basis table, then block by block of whole
// probes the rays and their trace into the block's slice of the radiance table, then the projection of the whole table.
static int probes_on_stream(ptk_ctx* c, int32_t num_probes, const float* d_positions, int32_t num_dirs, const float* d_dirs, int max_depth,
                            uint32_t first_sample, uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float weight, float* d_radiance,
                            float* d_coefs)
{
    c->ev_probes.begin(); c->ev_probe_blocks.begin();
    const size_t D = (size_t)num_dirs, rays = (size_t)num_probes * D;
    // a block holds at most max(D, pass_bytes / 256) rays, in whole probes: the rays are never all materialised
    const size_t block_probes = std::min<size_t>((size_t)num_probes, std::max<size_t>(1, c->opt_pass_bytes / 256 / D));
    int rc = c->d_probe_basis.grow(c, D, PTK_PROBE_COEFS * sizeof(float));
    if (rc == PTK_OK) rc = c->d_probe_rays.grow(c, block_probes * D, 6 * sizeof(float));
    if (rc == PTK_OK && !d_radiance) rc = c->d_probe_table.grow(c, rays, 3 * sizeof(float));
    if (rc != PTK_OK) return rc;
    float* const table = d_radiance ? d_radiance : c->d_probe_table;
    float* const origins = c->d_probe_rays, * const ray_dirs = origins + c->d_probe_rays.cap * 3;
    if (const int rm = c->ev_probes.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    launch_probe_basis(d_dirs, num_dirs, c->d_probe_basis, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_probes.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    for (size_t p0 = 0; p0 < (size_t)num_probes; p0 += block_probes)
    {
        const size_t np = std::min(block_probes, (size_t)num_probes - p0), ray0 = p0 * D;
        const int bi = c->ev_probe_blocks.passes < ptk_ctx::kMaxTimedPasses ? c->ev_probe_blocks.passes : -1;
        if (rc = c->ev_probe_blocks.reserve(c, bi + 1); rc != PTK_OK) return rc;
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_blocks.at(bi, 0), c->stream));
        launch_probe_rays(d_positions + p0 * 3, d_dirs, (int)np, num_dirs, origins, ray_dirs, c->stream);
        HIPCHK(c, hipGetLastError());
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_blocks.at(bi, 1), c->stream));
        // (contiguous keys: plain rays_kernel)
        rc = trace_rays_on_stream(c, (int32_t)(np * D), origins, ray_dirs, max_depth, first_sample, spp, seed, key_base + (uint32_t)ray0,
                                  (flags & PTK_PROBES_ACCUMULATE) ? PTK_RAYS_ACCUMULATE : 0u, table + ray0 * 3);
        if (rc != PTK_OK) return rc;
        if (bi >= 0) { HIPCHK(c, hipEventRecord(c->ev_probe_blocks.at(bi, 2), c->stream)); c->ev_probe_blocks.passes = bi + 1; }
    }
    if (const int rm = c->ev_probes.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    launch_probe_project(table, c->d_probe_basis, num_probes, num_dirs, weight, d_coefs, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_probes.mark(c, 3, c->stream); rm != PTK_OK) return rm;
    c->ev_probes.done();
    return PTK_OK;
}

int ptk_bake_probes_device(ptk_ctx* c, int32_t num_probes, const float* d_positions, int32_t num_dirs, const float* d_dirs, int max_depth,
                           uint32_t first_sample, uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float weight, float* d_radiance,
                           float* d_coefs)
{
    bool nothing;
    const int rc = check_probes_args(c, num_probes, d_positions, num_dirs, d_dirs, flags, weight, d_radiance, d_coefs, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return probes_on_stream(c, num_probes, d_positions, num_dirs, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, weight, d_radiance, d_coefs);
}

int ptk_bake_probes(ptk_ctx* c, int32_t num_probes, const float* positions, int32_t num_dirs, const float* dirs, int max_depth, uint32_t first_sample,
                    uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float weight, float* radiance, float* coefs)
{
    bool nothing;
    const int rc = check_probes_args(c, num_probes, positions, num_dirs, dirs, flags, weight, radiance, coefs, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)num_probes, nd = (size_t)num_dirs;
    Stage s(c);
    const auto d_positions = s.in(positions, np * 3), d_dirs = s.in(dirs, nd * 3), d_coefs = s.out(coefs, np * PTK_PROBE_COEFS * 3);
    const auto d_radiance = s.inout(radiance, np * nd * 3, (flags & PTK_PROBES_ACCUMULATE) != 0);      // (where the caller wants the table)
    return s.run([&] {
        return probes_on_stream(c, num_probes, d_positions, num_dirs, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, weight, d_radiance, d_coefs);
    });
}

static int check_irradiance_args(ptk_ctx* c, const int32_t* dims, const float* origin, const float* spacing, const float* coefs, int32_t num_points,
                                 const float* points, const float* normals, const float* out, ProbeGrid* grid, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (!dims || !origin || !spacing) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: null dims, origin or spacing");
    if (num_points < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: negative point count");
    uint64_t probes = 1;
    for (int a = 0; a < 3; a++)
    {
        if (dims[a] < 1) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: dims must be at least 1");
        if (!std::isfinite(spacing[a]) || !(spacing[a] > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: spacing must be finite and > 0");
        if (!std::isfinite(origin[a])) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: origin must be finite");
        probes *= (uint64_t)dims[a];
        if (probes >= (1ull << 31)) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: 2^31 probes or more");
        grid->dims[a] = dims[a]; grid->origin[a] = origin[a]; grid->spacing[a] = spacing[a];
    }
    if (num_points > 0 && (!coefs || !points || !normals || !out)) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance: null array");
    *nothing = num_points == 0;
    return PTK_OK;
}

int ptk_probes_irradiance_device(ptk_ctx* c, const int32_t dims[3], const float origin[3], const float spacing[3], const float* d_coefs,
                                 int32_t num_points, const float* d_points, const float* d_normals, float* d_out)
{
    ProbeGrid g; bool nothing;
    const int rc = check_irradiance_args(c, dims, origin, spacing, d_coefs, num_points, d_points, d_normals, d_out, &g, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    launch_probe_irradiance(g, d_coefs, num_points, d_points, d_normals, d_out, c->stream);
    HIPCHK(c, hipGetLastError());
    return PTK_OK;
}

int ptk_probes_irradiance(ptk_ctx* c, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int32_t num_points,
                          const float* points, const float* normals, float* out)
{
    ProbeGrid g; bool nothing;
    const int rc = check_irradiance_args(c, dims, origin, spacing, coefs, num_points, points, normals, out, &g, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)num_points * 3;
    Stage s(c);
    const auto d_coefs = s.in(coefs, (size_t)dims[0] * dims[1] * dims[2] * PTK_PROBE_COEFS * 3), d_points = s.in(points, n3), d_normals = s.in(normals, n3);
    const auto d_out = s.out(out, n3);
    return s.run([&] {
        launch_probe_irradiance(g, d_coefs, num_points, d_points, d_normals, d_out, c->stream);
        return s.launched();
    });
}

int ptk_last_probes_ms(ptk_ctx* c, float* raygen_ms, float* trace_ms, float* project_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float gen = 0.0f, trace = 0.0f, project = 0.0f;
    int rc = c->ev_probes.elapsed(c, 2, 3, &project);
    if (rc == PTK_OK) rc = c->ev_probes.elapsed(c, 0, 1, &gen);                        // (the basis table counts as ray generation)
    const int blocks = c->ev_probes.timed ? c->ev_probe_blocks.passes : 0;
    for (int i = 0; i < blocks && rc == PTK_OK; i++) rc = c->ev_probe_blocks.add(c, i, &gen, &trace);
    if (raygen_ms) *raygen_ms = gen;
    if (trace_ms) *trace_ms = trace;
    if (project_ms) *project_ms = project;
    return rc;
}

// ---- probe visibility (ptk.h) ------------------------------------------------------------------------------------
static int check_visibility_args(ptk_ctx* c, int32_t num_probes, const float* positions, int32_t num_dirs, const float* dirs, int res, float max_dist,
                                 const float* moments, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (num_probes < 0 || num_dirs < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: negative count");
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (res < 1 || res > PTK_PROBE_VIS_MAX_RES) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: res must be in 1..16");
    if (!std::isfinite(max_dist) || !(max_dist > 0.0f) || max_dist > 1e18f)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: max_dist must be finite, > 0 and at most 1e18");
    if (num_probes > 0)
    {
        if (num_dirs < 1 || num_dirs > 65536) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: num_dirs must be in 1..65536");
        if ((uint64_t)num_probes * (uint64_t)num_dirs >= (1ull << 31)) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: 2^31 rays or more");
        if (!positions || !dirs || !moments) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_probe_visibility: null array");
    }
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num_probes == 0;
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory: block by block of whole probes - probes_on_stream's
// blocks and ray buffer - the rays and hits_kernel with only t requested, into the block's slice of the depth table; then the
// moments of the whole table.  A scene without triangles has no tree to walk: its table is filled with +inf.
static int visibility_on_stream(ptk_ctx* c, int32_t num_probes, const float* d_positions, int32_t num_dirs, const float* d_dirs, int res, float max_dist,
                                uint32_t sample, uint64_t seed, uint32_t key_base, float* d_depth, float* d_moments)
{
    c->ev_probe_vis.begin(); c->ev_probe_vis_blocks.begin();
    const size_t D = (size_t)num_dirs, rays = (size_t)num_probes * D;
    const size_t block_probes = std::min<size_t>((size_t)num_probes, std::max<size_t>(1, c->opt_pass_bytes / 256 / D));
    int rc = c->d_probe_rays.grow(c, block_probes * D, 6 * sizeof(float));
    if (rc == PTK_OK && !d_depth) rc = c->d_probe_depth.grow(c, rays, sizeof(float));
    if (rc != PTK_OK) return rc;
    float* const table = d_depth ? d_depth : c->d_probe_depth;
    float* const origins = c->d_probe_rays, * const ray_dirs = origins + c->d_probe_rays.cap * 3;
    for (size_t p0 = 0; p0 < (size_t)num_probes; p0 += block_probes)
    {
        const size_t np = std::min(block_probes, (size_t)num_probes - p0), ray0 = p0 * D;
        const int bi = c->ev_probe_vis_blocks.passes < ptk_ctx::kMaxTimedPasses ? c->ev_probe_vis_blocks.passes : -1;
        if (rc = c->ev_probe_vis_blocks.reserve(c, bi + 1); rc != PTK_OK) return rc;
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_vis_blocks.at(bi, 0), c->stream));
        if (c->num_nodes > 0) launch_probe_rays(d_positions + p0 * 3, d_dirs, (int)np, num_dirs, origins, ray_dirs, c->stream);
        HIPCHK(c, hipGetLastError());
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_vis_blocks.at(bi, 1), c->stream));
        if (c->num_nodes > 0)
        {
            HitsParams h = {};
            h.nodes = c->d_nodes; h.tris = c->d_tris; h.shade = c->d_shade; h.texinfo = c->d_texinfo; h.texels = c->d_texels;
            h.origins = origins; h.dirs = ray_dirs; h.t = table + ray0; h.num_rays = (int)(np * D);
            h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound; h.tri_thr = c->opt_tri_thr;
            h.seed_lo = (uint32_t)seed; h.seed_hi = (uint32_t)(seed >> 32); h.sample = sample; h.key_base = key_base + (uint32_t)ray0;
            launch_hits(h, c->stream);
            HIPCHK(c, hipGetLastError());
        }
        else HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)(table + ray0), 0x7f800000, np * D, c->stream));
        if (bi >= 0) { HIPCHK(c, hipEventRecord(c->ev_probe_vis_blocks.at(bi, 2), c->stream)); c->ev_probe_vis_blocks.passes = bi + 1; }
    }
    if (const int rm = c->ev_probe_vis.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    launch_probe_moments(table, d_dirs, num_probes, num_dirs, res, max_dist, d_moments, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_probe_vis.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    c->ev_probe_vis.done();
    return PTK_OK;
}

int ptk_bake_probe_visibility_device(ptk_ctx* c, int32_t num_probes, const float* d_positions, int32_t num_dirs, const float* d_dirs, int res,
                                     float max_dist, uint32_t sample, uint64_t seed, uint32_t key_base, float* d_depth, float* d_moments)
{
    bool nothing;
    const int rc = check_visibility_args(c, num_probes, d_positions, num_dirs, d_dirs, res, max_dist, d_moments, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return visibility_on_stream(c, num_probes, d_positions, num_dirs, d_dirs, res, max_dist, sample, seed, key_base, d_depth, d_moments);
}

int ptk_bake_probe_visibility(ptk_ctx* c, int32_t num_probes, const float* positions, int32_t num_dirs, const float* dirs, int res, float max_dist,
                              uint32_t sample, uint64_t seed, uint32_t key_base, float* depth, float* moments)
{
    bool nothing;
    const int rc = check_visibility_args(c, num_probes, positions, num_dirs, dirs, res, max_dist, moments, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t np = (size_t)num_probes, nd = (size_t)num_dirs;
    Stage s(c);
    const auto d_positions = s.in(positions, np * 3), d_dirs = s.in(dirs, nd * 3), d_moments = s.out(moments, np * (size_t)(res * res) * 2);
    const auto d_depth = s.out(depth, np * nd);                                                         // (where the caller wants the table)
    return s.run([&] {
        return visibility_on_stream(c, num_probes, d_positions, num_dirs, d_dirs, res, max_dist, sample, seed, key_base, d_depth, d_moments);
    });
}

static int check_visible_args(ptk_ctx* c, int res, const float* moments, float normal_bias, int32_t num_points)
{
    if (res < 1 || res > PTK_PROBE_VIS_MAX_RES) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance_visible: res must be in 1..16");
    if (!std::isfinite(normal_bias)) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance_visible: normal_bias must be finite");
    if (num_points > 0 && !moments) return fail(c, PTK_ERR_BAD_ARG, "ptk_probes_irradiance_visible: null array");
    return PTK_OK;
}

int ptk_probes_irradiance_visible_device(ptk_ctx* c, const int32_t dims[3], const float origin[3], const float spacing[3], const float* d_coefs, int res,
                                         const float* d_moments, float normal_bias, int32_t num_points, const float* d_points,
                                         const float* d_normals, float* d_out)
{
    ProbeGrid g; bool nothing;
    int rc = check_irradiance_args(c, dims, origin, spacing, d_coefs, num_points, d_points, d_normals, d_out, &g, &nothing);
    if (rc == PTK_OK) rc = check_visible_args(c, res, d_moments, normal_bias, num_points);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    launch_probe_irradiance_visible(g, d_coefs, res, d_moments, normal_bias, num_points, d_points, d_normals, d_out, c->stream);
    HIPCHK(c, hipGetLastError());
    return PTK_OK;
}

int ptk_probes_irradiance_visible(ptk_ctx* c, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int res,
                                  const float* moments, float normal_bias, int32_t num_points, const float* points, const float* normals,
                                  float* out)
{
    ProbeGrid g; bool nothing;
    int rc = check_irradiance_args(c, dims, origin, spacing, coefs, num_points, points, normals, out, &g, &nothing);
    if (rc == PTK_OK) rc = check_visible_args(c, res, moments, normal_bias, num_points);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)num_points * 3, probes = (size_t)dims[0] * dims[1] * dims[2];
    Stage s(c);
    const auto d_coefs = s.in(coefs, probes * PTK_PROBE_COEFS * 3), d_moments = s.in(moments, probes * (size_t)(res * res) * 2);
    const auto d_points = s.in(points, n3), d_normals = s.in(normals, n3);
    const auto d_out = s.out(out, n3);
    return s.run([&] {
        launch_probe_irradiance_visible(g, d_coefs, res, d_moments, normal_bias, num_points, d_points, d_normals, d_out, c->stream);
        return s.launched();
    });
}

int ptk_last_probe_visibility_ms(ptk_ctx* c, float* raygen_ms, float* hits_ms, float* moments_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float gen = 0.0f, hits = 0.0f, moments = 0.0f;
    int rc = c->ev_probe_vis.elapsed(c, 0, 1, &moments);
    const int blocks = c->ev_probe_vis.timed ? c->ev_probe_vis_blocks.passes : 0;
    for (int i = 0; i < blocks && rc == PTK_OK; i++) rc = c->ev_probe_vis_blocks.add(c, i, &gen, &hits);
    if (raygen_ms) *raygen_ms = gen;
    if (hits_ms) *hits_ms = hits;
    if (moments_ms) *moments_ms = moments;
    return rc;
}

}  // extern "C"
