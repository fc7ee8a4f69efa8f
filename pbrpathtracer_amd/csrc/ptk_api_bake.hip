// Host side of the ptk C-ABI: lightmap coverage, bake, adaptive bake (its round loop: ptk_api_rays.hip) and dilation.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_bake.h"
#include "ptk_rays.h"
#include "ptk_rays_adaptive.h"

using namespace ptk;

extern "C" {

static int check_bake_map(ptk_ctx* c, const char* who, int width, int height)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (width < 1 || height < 1 || width > 16384 || height > 16384)
        return fail(c, PTK_ERR_BAD_ARG, (std::string(who) + ": width and height must be in 1..16384").c_str());
    return PTK_OK;
}

static int check_lightmap_args(ptk_ctx* c, int width, int height, float offset, uint32_t flags, const float* out)
{
    const int rc = check_bake_map(c, "ptk_bake_lightmap", width, height);
    if (rc != PTK_OK) return rc;
    if (flags & ~(PTK_BAKE_ACCUMULATE | PTK_BAKE_BACK)) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_lightmap: unknown flag bits");
    if (!std::isfinite(offset) || !(offset > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_lightmap: offset must be finite and > 0");
    if (!out) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_lightmap: null out");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    return PTK_OK;
}

// The front half of a bake on the context's stream: coverage and - with want_rays - the covered count (the one host wait) and the
// compacted rays of the covered texels in b (their sums loaded from acc_out where that is not null: PTK_BAKE_ACCUMULATE).
static int bake_rays_on_stream(ptk_ctx* c, int width, int height, const float* d_uvs, float offset, uint32_t key_base, uint32_t flags, bool want_rays,
                               const float* acc_out, int32_t* d_owner, float* d_bary, float* d_pos, BakeParams& b, uint32_t& covered)
{
    const size_t texels = (size_t)width * height, blocks = (texels + 255) / 256;
    c->ev_bake.begin();
    // the plane, then one count per block of 256 texels and the total
    int rc = c->d_bake_plane.grow(c, texels, sizeof(int), (blocks + 1) * sizeof(int));
    if (rc != PTK_OK) return rc;
    b = BakeParams{};
    b.uvs = d_uvs; b.shade = c->d_shade; b.verts = c->d_verts_res; b.num_tris = c->d_verts_res ? c->num_tris : 0;
    b.width = width; b.height = height; b.offset = offset; b.back = (flags & PTK_BAKE_BACK) ? 1 : 0; b.key_base = key_base;
    b.plane = c->d_bake_plane; b.block_counts = (uint32_t*)(c->d_bake_plane + c->d_bake_plane.cap);
    b.owner = d_owner; b.bary = d_bary; b.pos = d_pos;
    if (const int rm = c->ev_bake.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.plane, PTK_BAKE_UNOWNED, texels, c->stream));
    launch_bake_cover(b, c->stream);
    HIPCHK(c, hipGetLastError());
    covered = 0;
    if (want_rays)
    {
        // the covered count sizes the compacted arrays and the trace: the one host wait of a bake
        HIPCHK(c, c->h_bake_total.alloc(1));
        uint32_t* d_total = b.block_counts + blocks;
        launch_bake_count(b, d_total, c->stream);
        HIPCHK(c, hipGetLastError());
        if (const int rm = c->ev_bake.mark(c, 1, c->stream); rm != PTK_OK) return rm;
        HIPCHK(c, hipMemcpyAsync(c->h_bake_total, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        covered = *c->h_bake_total;
        if (covered > texels) return fail(c, PTK_ERR_HIP, "ptk_bake_lightmap: covered count exceeds the map");
        if (rc = c->d_bake_compact.grow(c, covered, 11 * sizeof(float)); rc != PTK_OK) return rc;
        if (covered)
        {
            const size_t cap = c->d_bake_compact.cap;
            b.origins = c->d_bake_compact; b.dirs = b.origins + cap * 3; b.sums = b.dirs + cap * 3;
            b.keys = (uint32_t*)(b.sums + cap * 3); b.texel = b.keys + cap;
            b.out = acc_out;
        }
    }
    else if (const int rm = c->ev_bake.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    if (const int rm = c->ev_bake.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    launch_bake_rays(b, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_bake.mark(c, 3, c->stream); rm != PTK_OK) return rm;
    return PTK_OK;
}

// Coverage - and, with d_out, the bake - on the context's stream, every pointer into this GPU's memory.
static int bake_on_stream(ptk_ctx* c, int width, int height, const float* d_uvs, float offset, int max_depth, uint32_t first_sample, uint32_t spp,
                          uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, int32_t* d_owner, float* d_bary, float* d_pos)
{
    const size_t texels = (size_t)width * height;
    BakeParams b;
    uint32_t covered = 0;
    int rc = bake_rays_on_stream(c, width, height, d_uvs, offset, key_base, flags, d_out != nullptr, (flags & PTK_BAKE_ACCUMULATE) ? d_out : nullptr,
                                 d_owner, d_bary, d_pos, b, covered);
    if (rc != PTK_OK) return rc;
    if (d_out)
    {
        if (covered)
        {
            rc = trace_rays_on_stream(c, (int32_t)covered, b.origins, b.dirs, max_depth, first_sample, spp, seed, 0u,
                                                (flags & PTK_BAKE_ACCUMULATE) ? PTK_RAYS_ACCUMULATE : 0u, b.sums, b.keys);
            if (rc != PTK_OK) return rc;
        }
        if (const int rm = c->ev_bake.mark(c, 4, c->stream); rm != PTK_OK) return rm;
        if (!(flags & PTK_BAKE_ACCUMULATE)) HIPCHK(c, hipMemsetAsync(d_out, 0, texels * 3 * sizeof(float), c->stream));     // uncovered texels
        launch_bake_scatter(b.sums, b.texel, covered, d_out, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    else if (const int rm = c->ev_bake.mark(c, 4, c->stream); rm != PTK_OK) return rm;
    if (const int rm = c->ev_bake.mark(c, 5, c->stream); rm != PTK_OK) return rm;
    c->ev_bake.done();
    return PTK_OK;
}

// Host entries: uvs, out, owner, bary and pos staged for the length of the call.
static int bake_staged(ptk_ctx* c, int width, int height, const float* uvs, float offset, int max_depth, uint32_t first_sample, uint32_t spp,
                       uint64_t seed, uint32_t key_base, uint32_t flags, float* out, int32_t* owner, float* bary, float* pos)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    Stage s(c);
    const auto d_uvs = s.in(uvs, (size_t)c->num_tris * 6), d_out = s.inout(out, texels * 3, (flags & PTK_BAKE_ACCUMULATE) != 0);
    const auto d_owner = s.out(owner, texels);
    const auto d_bary = s.out(bary, texels * 2), d_pos = s.out(pos, texels * 3);
    return s.run([&] {
        return bake_on_stream(c, width, height, d_uvs, offset, max_depth, first_sample, spp, seed, key_base, flags, d_out, d_owner, d_bary, d_pos);
    });
}

int ptk_bake_coverage(ptk_ctx* c, int width, int height, const float* uvs, int32_t* owner, float* bary, float* pos)
{
    const int rc = check_bake_map(c, "ptk_bake_coverage", width, height);
    if (rc != PTK_OK) return rc;
    return bake_staged(c, width, height, uvs, 0.0f, 0, 0, 0, 0, 0, 0, nullptr, owner, bary, pos);
}

int ptk_bake_lightmap(ptk_ctx* c, int width, int height, const float* uvs, float offset, int max_depth, uint32_t first_sample, uint32_t spp,
                      uint64_t seed, uint32_t key_base, uint32_t flags, float* out, int32_t* owner)
{
    const int rc = check_lightmap_args(c, width, height, offset, flags, out);
    if (rc != PTK_OK) return rc;
    return bake_staged(c, width, height, uvs, offset, max_depth, first_sample, spp, seed, key_base, flags, out, owner, nullptr, nullptr);
}

int ptk_bake_lightmap_device(ptk_ctx* c, int width, int height, const float* d_uvs, float offset, int max_depth, uint32_t first_sample, uint32_t spp,
                             uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, int32_t* d_owner)
{
    const int rc = check_lightmap_args(c, width, height, offset, flags, d_out);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return bake_on_stream(c, width, height, d_uvs, offset, max_depth, first_sample, spp, seed, key_base, flags, d_out, d_owner, nullptr, nullptr);
}

static int check_lightmap_adaptive_args(ptk_ctx* c, int width, int height, float offset, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp,
                                        uint32_t flags, const float* out, const uint32_t* counts)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (flags & PTK_BAKE_ACCUMULATE) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_lightmap_adaptive: an adaptive bake starts at sample 0, it cannot accumulate");
    int rc = check_lightmap_args(c, width, height, offset, flags, out);
    if (rc != PTK_OK) return rc;
    if (!counts) return fail(c, PTK_ERR_BAD_ARG, "ptk_bake_lightmap_adaptive: null counts");
    return check_adaptive_args(c, "ptk_bake_lightmap_adaptive", threshold, min_spp, step, max_spp);
}

int ptk_bake_lightmap_adaptive_device(ptk_ctx* c, int width, int height, const float* d_uvs, float offset, int max_depth, float threshold, uint32_t min_spp,
                                      uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, uint32_t* d_counts,
                                      int32_t* d_owner, ptk_rays_adaptive_result* res)
{
    int rc = check_lightmap_adaptive_args(c, width, height, offset, threshold, min_spp, step, max_spp, flags, d_out, d_counts);
    if (rc != PTK_OK) return rc;
    if (res) std::memset(res, 0, sizeof(*res));
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    BakeParams b;
    uint32_t covered = 0;
    rc = bake_rays_on_stream(c, width, height, d_uvs, offset, key_base, flags, true, nullptr, d_owner, nullptr, nullptr, b, covered);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipMemsetAsync(d_out, 0, texels * 3 * sizeof(float), c->stream));                 // uncovered texels
    HIPCHK(c, hipMemsetAsync(d_counts, 0, texels * sizeof(uint32_t), c->stream));
    if (covered)
    {
        rc = rays_adaptive_on_stream(c, covered, b.origins, b.dirs, b.keys, 0u, max_depth, threshold, min_spp, step, max_spp, seed, 0u, b.sums, nullptr,
                                     nullptr, b.texel, width, height, res);
        if (rc != PTK_OK) return rc;
        launch_bake_scatter(b.sums, b.texel, covered, d_out, c->stream);
        launch_bake_scatter_counts(radapt_buffers(c).counts, b.texel, covered, d_counts, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_bake_lightmap_adaptive(ptk_ctx* c, int width, int height, const float* uvs, float offset, int max_depth, float threshold, uint32_t min_spp,
                               uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* out, uint32_t* counts, int32_t* owner,
                               ptk_rays_adaptive_result* res)
{
    const int rc = check_lightmap_adaptive_args(c, width, height, offset, threshold, min_spp, step, max_spp, flags, out, counts);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    Stage s(c);
    const auto d_uvs = s.in(uvs, (size_t)c->num_tris * 6), d_out = s.out(out, texels * 3);
    const auto d_counts = s.out(counts, texels);
    const auto d_owner = s.out(owner, texels);
    return s.run([&] {
        return ptk_bake_lightmap_adaptive_device(c, width, height, d_uvs, offset, max_depth, threshold, min_spp, step, max_spp, seed, key_base, flags, d_out,
                                                 d_counts, d_owner, res);
    });
}

static int check_dilate_args(ptk_ctx* c, int width, int height, int passes, const float* image, const int32_t* owner)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (width < 1 || height < 1 || width > 16384 || height > 16384) return fail(c, PTK_ERR_BAD_ARG, "ptk_lightmap_dilate: width and height must be in 1..16384");
    if (passes < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_lightmap_dilate: negative passes");
    if (!image || !owner) return fail(c, PTK_ERR_BAD_ARG, "ptk_lightmap_dilate: null array");
    return PTK_OK;
}

int ptk_lightmap_dilate_device(ptk_ctx* c, int width, int height, int passes, float* d_image, int32_t* d_owner)
{
    const int rc = check_dilate_args(c, width, height, passes, d_image, d_owner);
    if (rc != PTK_OK || passes == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    if (const int rg = c->d_bake_dilate.grow(c, texels, 4 * sizeof(float)); rg != PTK_OK) return rg;
    // ping-pong between the caller's arrays and the context's; an odd number of passes ends in the latter and is copied back
    float* img[2] = { d_image, c->d_bake_dilate };
    int32_t* own[2] = { d_owner, (int32_t*)(c->d_bake_dilate + texels * 3) };
    for (int i = 0; i < passes; i++)
    {
        launch_dilate(img[i & 1], own[i & 1], img[(i + 1) & 1], own[(i + 1) & 1], width, height, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (passes & 1)
    {
        HIPCHK(c, hipMemcpyAsync(d_image, img[1], texels * 3 * sizeof(float), hipMemcpyDeviceToDevice, c->stream));
        HIPCHK(c, hipMemcpyAsync(d_owner, own[1], texels * sizeof(int32_t), hipMemcpyDeviceToDevice, c->stream));
    }
    return PTK_OK;
}

int ptk_lightmap_dilate(ptk_ctx* c, int width, int height, int passes, float* image, int32_t* owner)
{
    const int rc = check_dilate_args(c, width, height, passes, image, owner);
    if (rc != PTK_OK || passes == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    Stage s(c);
    const auto d_image = s.inout(image, texels * 3, true);
    const auto d_owner = s.inout(owner, texels, true);
    return s.run([&] { return ptk_lightmap_dilate_device(c, width, height, passes, d_image, d_owner); });
}

int ptk_last_bake_ms(ptk_ctx* c, float* coverage_ms, float* raygen_ms, float* trace_ms, float* scatter_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float t[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    int rc = c->ev_bake.elapsed(c, 0, 1, &t[0]);
    if (rc == PTK_OK) rc = c->ev_bake.spans(c, 2, 3, &t[1]);
    if (coverage_ms) *coverage_ms = t[0];
    if (raygen_ms) *raygen_ms = t[1];
    if (trace_ms) *trace_ms = t[2];
    if (scatter_ms) *scatter_ms = t[3];
    return rc;
}

}  // extern "C"
