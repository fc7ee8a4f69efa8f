// Host side of the ptk C-ABI: queries for caller-supplied rays - radiance (ptk_trace_rays), closest hit and occlusion, and the adaptive
// radiance query with the round loop it shares with the adaptive lightmap bake (ptk.h).
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>
#include <functional>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_rays.h"
#include "ptk_rays_adaptive.h"
#include "ptk_hits.h"

using namespace ptk;

// ---- radiance along caller-supplied rays (ptk.h) ---------------------------------------------------------------------------
// The argument checks both entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_rays_args(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, uint32_t flags, const float* out, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (flags & ~(PTK_RAYS_ACCUMULATE | PTK_RAYS_LENS_DRAWS)) return fail(c, PTK_ERR_BAD_ARG, "ptk_trace_rays: unknown flag bits");
    if (num_rays < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_trace_rays: negative ray count");
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (num_rays > 0 && (!origins || !dirs || !out)) return fail(c, PTK_ERR_BAD_ARG, "ptk_trace_rays: null array");
    // (max_depth: ptk_set_frame takes every value - a limit <= 0 ends each path at its first interaction -, and so does this call)
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num_rays == 0;
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory.  Cut into passes over the sample range - and,
// where even one sample of every ray exceeds the budget, into blocks of rays - so that no pass's sample buffer exceeds
// "pass_bytes" or half of the free device memory; a later pass folds onto what the earlier ones left in out.
// fold(ray0, rays, chunk, num_chunks, samples of the pass, samples of the earlier passes) queues what takes the pass's samples
// out of c->d_rays_samples: rays_fold_kernel for a plain query, rays_fold_moments_kernel for an adaptive round.  spp > 0, and the
// scene has a tree.
using RaysFold = std::function<void(size_t ray0, int rays, int chunk, int num_chunks, uint32_t samples, uint32_t samples_before)>;
static int trace_rays_passes(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, uint32_t first_sample,
                             uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, const uint32_t* d_keys, const RaysFold& fold)
{
    c->ev_rays.passes = 0;
    if (!c->d_rays_block) HIPCHK(c, hipMalloc(&c->d_rays_block.p, sizeof(RaysBlock)));
    RenderParams p;
    fill_params(c, p, first_sample, spp, seed);
    p.max_depth = max_depth;
    p.exit_flag = nullptr;                       // ptk_request_exit does not cut a ray query
    const size_t groups = ((size_t)num_rays + 63) / 64, group_bytes = 64 * sizeof(float4);      // one sample of one group of rays
    // samples per work item, by trace_kernel's rule (run_passes)
    const uint32_t chunk_opt = c->opt_chunk > 0 ? (uint32_t)c->opt_chunk : ((double)spp * (double)groups / 8.0 >= 49152.0 ? 8u : 4u);
    // (sample slots are 32-bit indices: 2^31 float4 at most)
    size_t budget = std::min<size_t>(std::max<size_t>(c->opt_pass_bytes, group_bytes), (size_t)1 << 35);
    {
        const size_t want = std::min(budget, groups * group_bytes * ((size_t)spp + chunk_opt));
        size_t free_b = 0, total_b = 0;
        if (want > c->d_rays_samples.cap)        // (only a call that has to allocate asks the driver)
        {
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max(std::max(free_b / 2, c->d_rays_samples.cap), group_bytes));
            else (void)hipGetLastError();
        }
    }
    // The largest pass is the first one: the buffer is brought to its size here, the budget halved while the device refuses.
    size_t block_groups; uint32_t max_pass;
    for (;;)
    {
        block_groups = std::min(groups, budget / group_bytes);
        max_pass = (uint32_t)std::min<size_t>(0x40000000u, budget / (block_groups * group_bytes));
        if (max_pass > chunk_opt) max_pass -= max_pass % chunk_opt;             // whole chunks
        // (the first pass's sample slots: its chunks, the last of which may be partly used)
        const uint32_t n0 = std::min(spp, max_pass), slots = n0 <= chunk_opt ? n0 : (n0 + chunk_opt - 1) / chunk_opt * chunk_opt;
        const size_t need = block_groups * group_bytes * slots;
        if (need <= c->d_rays_samples.cap) break;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (c->d_rays_samples.try_alloc(need, need) == hipSuccess) break;
        (void)hipGetLastError();
        if (budget <= group_bytes) return fail(c, PTK_ERR_HIP, "hipMalloc: no memory for the sample buffer of even one sample of 64 rays");
        budget = std::max(group_bytes, budget / 2);
    }
    RaysParams r = {};
    r.lens_draws = (flags & PTK_RAYS_LENS_DRAWS) ? 1 : 0;
    p.samples = c->d_rays_samples;
    for (size_t g0 = 0; g0 < groups; g0 += block_groups)
    {
        const size_t ray0 = g0 * 64, nr = std::min((size_t)num_rays - ray0, block_groups * 64), nb = (nr + 63) / 64;
        r.origins = d_origins + ray0 * 3; r.dirs = d_dirs + ray0 * 3;
        r.num_rays = (int)nr; r.key_base = key_base + (uint32_t)ray0;
        r.keys = d_keys ? d_keys + ray0 : nullptr;      // (a key per ray: ptk_bake_lightmap)
        for (uint32_t done = 0; done < spp;)
        {
            const uint32_t n = std::min(spp - done, max_pass);
            p.first_sample = first_sample + done; p.spp = n;
            p.chunk = (int)std::min(n, chunk_opt); p.num_chunks = (int)((n + p.chunk - 1) / p.chunk);
            p.num_items = (int)(nb * (size_t)p.num_chunks);
            const int pi = c->ev_rays.passes < ptk_ctx::kMaxTimedPasses ? c->ev_rays.passes : -1;
            if (const int rc = c->ev_rays.reserve(c, pi + 1); rc != PTK_OK) return rc;
            if (pi >= 0) HIPCHK(c, hipEventRecord(c->ev_rays.at(pi, 0), c->stream));
            launch_rays(p, r, c->d_rays_block, c->resident_waves, c->stream);
            HIPCHK(c, hipGetLastError());
            if (pi >= 0) HIPCHK(c, hipEventRecord(c->ev_rays.at(pi, 1), c->stream));
            fold(ray0, (int)nr, p.chunk, p.num_chunks, n, done);
            HIPCHK(c, hipGetLastError());
            if (pi >= 0) { HIPCHK(c, hipEventRecord(c->ev_rays.at(pi, 2), c->stream)); c->ev_rays.passes = pi + 1; }
            done += n;
        }
    }
    return PTK_OK;
}

int ptk::trace_rays_on_stream(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, uint32_t first_sample,
                              uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, const uint32_t* d_keys)
{
    c->ev_rays.passes = 0;
    // (a scene without triangles has no tree to walk: every path is black)
    if (spp == 0 || c->num_nodes == 0)
    {
        if (!(flags & PTK_RAYS_ACCUMULATE)) HIPCHK(c, hipMemsetAsync(d_out, 0, (size_t)num_rays * 3 * sizeof(float), c->stream));
        return PTK_OK;
    }
    return trace_rays_passes(c, num_rays, d_origins, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, d_keys,
                             [&](size_t ray0, int nr, int chunk, int num_chunks, uint32_t n, uint32_t done) {
                                 launch_rays_fold(c->d_rays_samples, d_out + ray0 * 3, nr, chunk, num_chunks, n,
                                                  ((flags & PTK_RAYS_ACCUMULATE) || done > 0) ? 1 : 0, c->stream);
                             });
}

// ---- adaptive ray queries and lightmap bakes (ptk.h) -------------------------------------------------------------------------
int ptk::check_adaptive_args(ptk_ctx* c, const char* who, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp)
{
    if (step < 2 || min_spp == 0 || min_spp % step != 0 || max_spp % step != 0 || min_spp > max_spp)
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": need step >= 2 dividing min_spp and max_spp, 0 < min_spp <= max_spp");
    if (!std::isfinite(threshold) || threshold < 0.0f) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": threshold must be finite and >= 0");
    return PTK_OK;
}

// The argument checks the ray, point and surface query entries share.  `count_word` names the count in the entry's error text ("ray
// count", "point count", "count"); `a`, `b`: the arrays a count > 0 needs (b may be the same as a); `also`: a complaint about an
// argument of the entry's own, reported in this place.  PTK_OK with *nothing = true: the call is legal and has nothing to do.
int ptk::check_query_args(ptk_ctx* c, const char* who, const char* count_word, int32_t num, const void* a, const void* b, bool have_out, bool* nothing,
                          const char* also)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (num < 0) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": negative " + count_word);
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!have_out) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": no output array");
    if (also) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": " + also);
    if (num > 0 && (!a || !b)) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null array");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num == 0;
    return PTK_OK;
}

RaysAdaptiveBuffers ptk::radapt_buffers(ptk_ctx* c)
{
    const size_t cap = c->d_radapt.cap;
    RaysAdaptiveBuffers a;
    a.origins = c->d_radapt; a.dirs = a.origins + cap * 3; a.s2 = a.dirs + cap * 3;
    a.keys = (uint32_t*)(a.s2 + cap * 3); a.src = a.keys + cap; a.list = a.src + cap; a.keep = a.list + cap; a.counts = a.keep + cap;
    a.block_counts = a.counts + cap; a.total = a.block_counts + (cap + 255) / 256;
    return a;
}

// The round loop on the context's stream, every pointer into this GPU's memory; n > 0.  s2 / counts null: the context's own.
// texel not null: a lightmap's covered texels (keys = their RNG pixels; the 3x3 rule over the width x height map).  Synchronous:
// every round ends with the host reading the next round's ray count.
int ptk::rays_adaptive_on_stream(ptk_ctx* c, uint32_t n, const float* d_origins, const float* d_dirs, const uint32_t* d_keys, uint32_t key_base,
                                 int max_depth, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t rays_flags,
                                 float* s1, float* s2, uint32_t* counts, const uint32_t* texel, int width, int height, ptk_rays_adaptive_result* res)
{
    const auto t0 = std::chrono::steady_clock::now();
    c->radapt_ms[0] = c->radapt_ms[1] = c->radapt_ms[2] = 0.0f;
    int rc = c->d_radapt.grow(c, n, 14 * sizeof(float), (((size_t)n + 255) / 256 + 1) * sizeof(float));
    if (rc != PTK_OK) return rc;
    HIPCHK(c, c->h_radapt_total.alloc(1));
    const RaysAdaptiveBuffers a = radapt_buffers(c);
    if (!s2) s2 = a.s2;
    if (!counts) counts = a.counts;
    uint8_t* need = nullptr;
    if (texel)
    {
        const size_t texels = (size_t)width * height;
        if (rc = c->d_radapt_need.grow(c, texels, 1); rc != PTK_OK) return rc;
        need = c->d_radapt_need;
        HIPCHK(c, hipMemsetAsync(need, 0, texels, c->stream));
    }
    HIPCHK(c, hipMemsetAsync(s1, 0, (size_t)n * 3 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(s2, 0, (size_t)n * 3 * sizeof(float), c->stream));
    uint32_t rounds = 0, done = 0, active = n;
    uint64_t ray_samples = 0;
    if (c->num_nodes == 0)
    {
        // a scene without triangles has no tree to walk: every sample is black, and the rule decides at the first test - for all
        // rays alike - whether black has converged (it has, unless the tolerance's square is not above 0)
        const float tol = threshold * (0.0f + 1.0f / 256.0f);
        const float tol2 = tol * tol;
        done = 0.0f < tol2 ? min_spp : max_spp;
        HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)counts, (int)done, n, c->stream));
        rounds = done / step; ray_samples = (uint64_t)n * done;
        active = 0.0f < tol2 ? 0u : n;
    }
    else
    {
        HIPCHK(c, hipMemsetAsync(counts, 0, (size_t)n * sizeof(uint32_t), c->stream));
        const uint32_t* list = nullptr;              // round 0: every ray, in index order
        while (active > 0 && done < max_spp)
        {
            // no test before min_spp samples: the rounds up to there are traced as one
            const uint32_t take = done == 0 ? min_spp : step;
            c->ev_radapt.begin();
            if (rc = c->ev_radapt.mark(c, 0, c->stream); rc != PTK_OK) return rc;
            launch_rays_gather(list, active, d_origins, d_dirs, d_keys, key_base, a.origins, a.dirs, a.keys, a.src, c->stream);
            HIPCHK(c, hipGetLastError());
            rc = trace_rays_passes(c, (int32_t)active, a.origins, a.dirs, max_depth, done, take, seed, 0u, rays_flags, a.keys,
                                   [&](size_t ray0, int nr, int chunk, int num_chunks, uint32_t ns, uint32_t before) {
                                       // (the last pass of a block of rays counts the round's samples)
                                       launch_rays_fold_moments(c->d_rays_samples, a.src + ray0, s1, s2, counts, nr, chunk, num_chunks, ns,
                                                                before + ns == take ? take : 0u, c->stream);
                                   });
            if (rc != PTK_OK) return rc;
            done += take; rounds += take / step; ray_samples += (uint64_t)active * take;
            launch_rays_converge(a.src, active, s1, s2, counts, threshold, a.keep, need, texel, c->stream);
            if (texel) launch_bake_keep(a.src, active, texel, need, width, height, a.keep, c->stream);
            launch_rays_compact(a.src, a.keep, active, a.block_counts, a.total, a.list, c->stream);
            HIPCHK(c, hipGetLastError());
            HIPCHK(c, hipMemcpyAsync(c->h_radapt_total, a.total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
            if (rc = c->ev_radapt.mark(c, 1, c->stream); rc != PTK_OK) return rc;
            c->ev_radapt.done();
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (*c->h_radapt_total > active) return fail(c, PTK_ERR_HIP, "adaptive rays: the active list grew");
            float all = 0.0f, trace = 0.0f;
            rc = c->ev_radapt.elapsed(c, 0, 1, &all);
            for (int i = 0; i < c->ev_rays.passes && rc == PTK_OK; i++) rc = c->ev_rays.add(c, i, &trace, nullptr);
            if (rc != PTK_OK) return rc;
            c->radapt_ms[1] += trace; c->radapt_ms[2] += all - trace;
            active = *c->h_radapt_total;
            list = a.list;
        }
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->radapt_ms[0] = std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (res)
    {
        res->rounds = rounds; res->max_count = done;
        res->ray_samples = ray_samples; res->active_rays = active;
    }
    return PTK_OK;
}

extern "C" {

int ptk_trace_rays_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, uint32_t first_sample, uint32_t spp,
                          uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out)
{
    bool nothing;
    const int rc = check_rays_args(c, num_rays, d_origins, d_dirs, flags, d_out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return trace_rays_on_stream(c, num_rays, d_origins, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, d_out);
}

int ptk_trace_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, int max_depth, uint32_t first_sample, uint32_t spp,
                   uint64_t seed, uint32_t key_base, uint32_t flags, float* out)
{
    bool nothing;
    const int rc = check_rays_args(c, num_rays, origins, dirs, flags, out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)num_rays * 3;
    Stage s(c);
    const auto d_origins = s.in(origins, n3), d_dirs = s.in(dirs, n3), d_out = s.inout(out, n3, (flags & PTK_RAYS_ACCUMULATE) != 0);
    return s.run([&] { return trace_rays_on_stream(c, num_rays, d_origins, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, d_out); });
}

int ptk_last_rays_ms(ptk_ctx* c, float* trace_ms, float* fold_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float t = 0.0f, f = 0.0f;
    for (int i = 0; i < c->ev_rays.passes; i++)
        if (const int rc = c->ev_rays.add(c, i, &t, &f); rc != PTK_OK) return rc;
    if (trace_ms) *trace_ms = t;
    if (fold_ms) *fold_ms = f;
    return PTK_OK;
}

// ---- closest-hit and occlusion queries for caller-supplied rays (ptk.h) --------------------------------------------------------
// The argument checks the entries share: check_query_args (above) with the word of these entries' texts.
static int check_hits_args(ptk_ctx* c, const char* who, int32_t num_rays, const float* origins, const float* dirs, bool have_out, bool* nothing)
{
    return check_query_args(c, who, "ray count", num_rays, origins, dirs, have_out, nothing);
}

// The call proper, on the context's stream, every pointer into this GPU's memory: h holds the rays and the outputs, the scene
// half is filled in here.  One kernel between the two events; a scene without triangles has no tree to walk and gets its misses
// from fills.
static int hits_on_stream(ptk_ctx* c, HitsParams& h, uint32_t sample, uint64_t seed, uint32_t key_base, bool occlusion)
{
    c->ev_hits.begin();
    const size_t n = (size_t)h.num_rays;
    if (c->num_nodes == 0)
    {
        if (occlusion) HIPCHK(c, hipMemsetAsync(h.occluded, 0, n, c->stream));
        if (h.tri) HIPCHK(c, hipMemsetAsync(h.tri, 0xff, n * sizeof(int32_t), c->stream));
        if (h.t) HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)h.t, 0x7f800000, n, c->stream));
        if (h.bary) HIPCHK(c, hipMemsetAsync(h.bary, 0, n * 2 * sizeof(float), c->stream));
        if (h.material) HIPCHK(c, hipMemsetAsync(h.material, 0xff, n * sizeof(int32_t), c->stream));
        return PTK_OK;
    }
    h.nodes = c->d_nodes; h.tris = c->d_tris; h.shade = c->d_shade; h.texinfo = c->d_texinfo; h.texels = c->d_texels;
    h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound; h.tri_thr = c->opt_tri_thr;
    h.seed_lo = (uint32_t)seed; h.seed_hi = (uint32_t)(seed >> 32); h.sample = sample; h.key_base = key_base;
    if (const int rc = c->ev_hits.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    if (occlusion) launch_occluded(h, c->stream); else launch_hits(h, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rc = c->ev_hits.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_hits.done();
    return PTK_OK;
}

int ptk_intersect_rays_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, uint32_t sample, uint64_t seed,
                              uint32_t key_base, int32_t* d_tri, float* d_t, float* d_bary, int32_t* d_material)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_intersect_rays", num_rays, d_origins, d_dirs, d_tri || d_t || d_bary || d_material, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HitsParams h = {};
    h.origins = d_origins; h.dirs = d_dirs; h.num_rays = num_rays;
    h.tri = d_tri; h.t = d_t; h.bary = d_bary; h.material = d_material;
    return hits_on_stream(c, h, sample, seed, key_base, false);
}

int ptk_occluded_rays_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, const float* d_tmax, uint32_t sample,
                             uint64_t seed, uint32_t key_base, uint8_t* d_occluded)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_occluded_rays", num_rays, d_origins, d_dirs, num_rays == 0 || d_occluded, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    HitsParams h = {};
    h.origins = d_origins; h.dirs = d_dirs; h.tmax = d_tmax; h.num_rays = num_rays; h.occluded = d_occluded;
    return hits_on_stream(c, h, sample, seed, key_base, true);
}

// The host entries: origins, dirs, tmax and the requested outputs staged for the length of the call
int ptk_intersect_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, uint32_t sample, uint64_t seed, uint32_t key_base,
                       int32_t* tri, float* t, float* bary, int32_t* material)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_intersect_rays", num_rays, origins, dirs, tri || t || bary || material, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_rays;
    Stage s(c);
    const auto d_origins = s.in(origins, 3 * n), d_dirs = s.in(dirs, 3 * n);
    const auto d_tri = s.out(tri, n);
    const auto d_t = s.out(t, n), d_bary = s.out(bary, 2 * n);
    const auto d_material = s.out(material, n);
    return s.run([&] { return ptk_intersect_rays_device(c, num_rays, d_origins, d_dirs, sample, seed, key_base, d_tri, d_t, d_bary, d_material); });
}

int ptk_occluded_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample, uint64_t seed,
                      uint32_t key_base, uint8_t* occluded)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_occluded_rays", num_rays, origins, dirs, num_rays == 0 || occluded, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_rays;
    Stage s(c);
    const auto d_origins = s.in(origins, 3 * n), d_dirs = s.in(dirs, 3 * n), d_tmax = s.in(tmax, n);
    const auto d_occluded = s.out(occluded, n);
    return s.run([&] { return ptk_occluded_rays_device(c, num_rays, d_origins, d_dirs, d_tmax, sample, seed, key_base, d_occluded); });
}

int ptk_last_hits_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_hits, ms); }

static int check_rays_adaptive_args(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, float threshold, uint32_t min_spp, uint32_t step,
                                    uint32_t max_spp, uint32_t flags, const float* sum, const uint32_t* counts, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (flags & PTK_RAYS_ACCUMULATE) return fail(c, PTK_ERR_BAD_ARG, "ptk_trace_rays_adaptive: an adaptive query starts at sample 0, it cannot accumulate");
    int rc = check_rays_args(c, num_rays, origins, dirs, flags, sum, nothing);
    if (rc != PTK_OK) return rc;
    *nothing = false;
    if (num_rays > 0 && !counts) return fail(c, PTK_ERR_BAD_ARG, "ptk_trace_rays_adaptive: null counts");
    rc = check_adaptive_args(c, "ptk_trace_rays_adaptive", threshold, min_spp, step, max_spp);
    if (rc != PTK_OK) return rc;
    *nothing = num_rays == 0;
    return PTK_OK;
}

int ptk_trace_rays_adaptive_device(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, float threshold,
                                   uint32_t min_spp, uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* d_sum,
                                   float* d_sumsq, uint32_t* d_counts, ptk_rays_adaptive_result* res)
{
    bool nothing;
    const int rc = check_rays_adaptive_args(c, num_rays, d_origins, d_dirs, threshold, min_spp, step, max_spp, flags, d_sum, d_counts, &nothing);
    if (rc != PTK_OK) return rc;
    if (res) std::memset(res, 0, sizeof(*res));
    if (nothing) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return rays_adaptive_on_stream(c, (uint32_t)num_rays, d_origins, d_dirs, nullptr, key_base, max_depth, threshold, min_spp, step, max_spp, seed, flags,
                                   d_sum, d_sumsq, d_counts, nullptr, 0, 0, res);
}

int ptk_trace_rays_adaptive(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, int max_depth, float threshold, uint32_t min_spp,
                            uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* sum, float* sumsq, uint32_t* counts,
                            ptk_rays_adaptive_result* res)
{
    bool nothing;
    const int rc = check_rays_adaptive_args(c, num_rays, origins, dirs, threshold, min_spp, step, max_spp, flags, sum, counts, &nothing);
    if (rc != PTK_OK) return rc;
    if (res) std::memset(res, 0, sizeof(*res));
    if (nothing) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)num_rays * 3;
    Stage s(c);
    const auto d_origins = s.in(origins, n3), d_dirs = s.in(dirs, n3), d_sum = s.out(sum, n3), d_sumsq = s.out(sumsq, n3);
    const auto d_counts = s.out(counts, (size_t)num_rays);
    return s.run([&] {
        return rays_adaptive_on_stream(c, (uint32_t)num_rays, d_origins, d_dirs, nullptr, key_base, max_depth, threshold, min_spp, step, max_spp, seed, flags,
                                       d_sum, d_sumsq, d_counts, nullptr, 0, 0, res);
    });
}

int ptk_last_rays_adaptive_ms(ptk_ctx* c, float* total_ms, float* trace_ms, float* other_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (total_ms) *total_ms = c->radapt_ms[0];
    if (trace_ms) *trace_ms = c->radapt_ms[1];
    if (other_ms) *other_ms = c->radapt_ms[2];
    return PTK_OK;
}

}  // extern "C"
