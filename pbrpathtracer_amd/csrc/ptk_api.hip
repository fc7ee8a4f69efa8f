// Host side of the ptk C-ABI (include/ptk.h), the core: context (ptk_ctx.h), scene staging into the device record layouts of
// ptk_device.h, BVH build, the render loop and its kernel launches, feature planes, hand-off copies, options.  The other entries live
// beside it by feature, in ptk_api_{geometry,rays,bake,probes,exchange,debug}.hip; host entries stage their arrays through ptk_stage.h.
//
// Reference behaviour restated here (PathTracing/src/pathtracer.cpp): BuildBVH + light list :260-274,
// setters :297-360, frame set-up arithmetic of RenderFrame :755-766, reset :745-751.
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>
#include <dlfcn.h>

#include <algorithm>
#include <chrono>
#include <cmath>
#include <cstring>

#include "bvh_build.h"
#include "bvh_device.h"
#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_device_fn.h"
#include "ptk_adaptive.h"
#include "ptk_refit.h"
#include "ptk_flat_mt.h"
#include "ptk_table_offset.h"

using namespace ptk;

namespace {

inline float as_float(int32_t i) { float f; std::memcpy(&f, &i, 4); return f; }

void normalize3(const float* in, float* out)
{
    // glm::normalize = x * (1 / sqrt(dot(x, x)))   (pathtracer.cpp:336-337)
    float sqr = in[0] * in[0] + in[1] * in[1] + in[2] * in[2];
    float inv = 1.0f / std::sqrt(sqr);
    out[0] = in[0] * inv; out[1] = in[1] * inv; out[2] = in[2] * inv;
}

// device material record (ptk_device.h) from the boundary's ptk_material
void pack_material(const ptk_material& m, const std::vector<int32_t>& texmap, float* q)
{
    q[0] = m.diffuse[0]; q[1] = m.diffuse[1]; q[2] = m.diffuse[2]; q[3] = as_float(m.type != 0 ? 1 : 0);
    q[4] = m.specular[0]; q[5] = m.specular[1]; q[6] = m.specular[2]; q[7] = m.emissive_intensity;
    q[8] = m.emissive[0]; q[9] = m.emissive[1]; q[10] = m.emissive[2]; q[11] = m.roughness;
    // Russian-roulette probability, pathtracer.cpp:589: glm::min(0.95f, glm::max(glm::max(d.x, d.y), d.z))
    float mx = m.diffuse[0] < m.diffuse[1] ? m.diffuse[1] : m.diffuse[0];
    mx = mx < m.diffuse[2] ? m.diffuse[2] : mx;
    float prob = 0.95f < mx ? 0.95f : mx;
    q[12] = m.reflectiveness; q[13] = m.translucency; q[14] = m.ior; q[15] = prob;
    int any = 0;
    for (int k = 0; k < 6; k++)
    {
        int32_t t = m.tex[k] >= 0 ? texmap[m.tex[k]] : -1;
        q[16 + k] = as_float(t);
        if (t >= 0) any = 1;
    }
    q[22] = as_float(any); q[23] = 0.0f;
}

// image-plane set-up of RenderFrame, pathtracer.cpp:755-766 (host, once per camera/resolution change)
// ... at any size: the context is only read, the camera's right vector goes into pp alone (the guide planes' view, ptk_render_guides)
void frame_setup_at(const ptk_ctx* c, int width, int height, PrimaryParams& pp)
{
    const float* pos = c->cam_pos; const float* dir = c->cam_dir; const float* up = c->cam_up;
    float center[3] = { pos[0] + dir[0] * c->focal, pos[1] + dir[1] * c->focal, pos[2] + dir[2] * c->focal };
    float img_h = (float)((double)(2.0f * c->focal) * std::tan((double)(c->fovy / 2.0f) * 3.14159265358979323846 / (double)180.0f));
    float aspect = (float)width / (float)height;
    float img_w = img_h * aspect;
    pp.delta_x = img_w / (float)width;
    pp.delta_y = img_h / (float)height;
    // camRight = normalize(cross(up, dir))
    float cr[3] = { up[1] * dir[2] - dir[1] * up[2], up[2] * dir[0] - dir[2] * up[0], up[0] * dir[1] - dir[0] * up[1] };
    float right[3];
    normalize3(cr, right);
    float hw = img_w * 0.5f, hh = img_h * 0.5f;
    for (int a = 0; a < 3; a++)
    {
        float tl = center[a] - right[a] * hw;
        tl = tl + up[a] * hh;
        pp.top_left[a] = tl;
        pp.cam_pos[a] = pos[a]; pp.cam_right[a] = right[a]; pp.cam_up[a] = up[a];
    }
    pp.primary = nullptr; pp.width = width; pp.height = height;
}

void frame_setup(ptk_ctx* c, PrimaryParams& pp)
{
    frame_setup_at(c, c->width, c->height, pp);
    for (int a = 0; a < 3; a++) c->cam_right[a] = pp.cam_right[a];
    pp.primary = c->d_primary;
}

// on-image pixels of the tiles this rank owns (same tile -> rank map as the kernels)
unsigned long long owned_pixels(const ptk_ctx* c)
{
    const int tiles_x = (c->width + PTK_TILE - 1) / PTK_TILE, tiles_y = (c->height + PTK_TILE - 1) / PTK_TILE;
    unsigned long long n = 0;
    for (int tile = c->rank; tile < tiles_x * tiles_y; tile += c->world)
    {
        int tx, ty; tile_origin(tile, tiles_x, tx, ty);
        const int w = std::min(PTK_TILE, c->width - tx * PTK_TILE), h = std::min(PTK_TILE, c->height - ty * PTK_TILE);
        n += (unsigned long long)w * h;
    }
    return n;
}

// The scene-table half of "plain" (ptk.h ptk_scene_is_plain): few enough triangles for the FLAT kernel, every material opaque and
// without a texture in its five shading slots, no triangle smoothed or of a material with an opacity texture.  Such a scene cannot
// reach anything the PLAIN variant of the FLAT trace kernel leaves out, whatever its materials' other fields hold.
bool plain_tables(int32_t n, const uint8_t* smoothing, const int32_t* material, int32_t num_materials, const ptk_material* mats)
{
    if (n <= 0 || n > 16 || !smoothing || !material || !mats) return false;
    for (int32_t i = 0; i < num_materials; i++)
    {
        if (mats[i].type != 0) return false;
        for (int k = 0; k < 5; k++)
            if (mats[i].tex[k] >= 0) return false;
    }
    for (int32_t i = 0; i < n; i++)
    {
        if (smoothing[i]) return false;
        if (material[i] < 0 || material[i] >= num_materials || mats[material[i]].tex[5] >= 0) return false;
    }
    return true;
}

// "Lambert" (ptk.h ptk_scene_is_lambert): a plain scene no material of which has reflectiveness > 0.  The specular draw of the
// opaque route, `draw < reflectiveness` with draw in [0, 1), is then false whatever is drawn - for zeros of either sign, negatives
// and NaN alike - so the LAMBERT level of the PLAIN kernel keeps the draw's advance of the stream and the diffuse route alone.
// Untextured by plainness: the table's value is the one the kernel compares.
bool lambert_tables(int32_t n, const uint8_t* smoothing, const int32_t* material, int32_t num_materials, const ptk_material* mats)
{
    if (!plain_tables(n, smoothing, material, num_materials, mats)) return false;
    for (int32_t i = 0; i < num_materials; i++)
        if (mats[i].reflectiveness > 0.0f) return false;
    return true;
}

bool primary_cacheable(const ptk_ctx* c)
{
    return c->opt_primary_cache && c->aperture == 0.0f && !c->scene_has_opacity && c->have_scene && c->d_primary_hit;
}

// keep_gl: a new resolution lets host and device buffers go (the caller reallocates them) but keeps an OpenGL buffer object
// registered - unregistering talks to the OpenGL driver and belongs to the thread that owns the context (ptk_bind_gl_buffer);
// the buffer's size is checked each time it is mapped
void unbind_out_image(ptk_ctx* c, bool keep_gl = false)
{
    if (c->out_registered && c->out_host) { (void)hipHostUnregister(c->out_host); (void)hipGetLastError(); }
    c->out_host = nullptr; c->out_host_dev = nullptr; c->out_registered = false; c->out_full_next = true;
    c->out_device = nullptr;
    if (keep_gl) return;
    if (c->gl_res) { (void)hipGraphicsUnregisterResource(c->gl_res); (void)hipGetLastError(); }
    c->gl_res = nullptr; c->gl_buffer = 0;
}

// An OpenGL buffer object is HIP's for the length of a render only: mapped before the first pass, unmapped (on the render
// stream, so behind the accumulate kernel that writes it) on every way out of run_passes.
struct GlMapping
{
    ptk_ctx* c; bool mapped = false;
    ~GlMapping() { if (mapped) { (void)hipGraphicsUnmapResources(1, &c->gl_res, c->stream); (void)hipGetLastError(); } }
};

// channels and element type of the feature planes (ptk.h PTK_FEAT_*)
const int kFeatChannels[NUM_FEATURES] = { 1, 1, 1, 2, 3, 3, 3, 3, 3, 2 };
const int kFeatIsInt[NUM_FEATURES] = { 0, 1, 1, 0, 0, 0, 0, 0, 0, 0 };

void free_features(ptk_ctx* c)
{
    for (auto& b : c->d_feat) b.release();
    c->feat_w = c->feat_h = 0; c->feat_mask = 0;
    c->d_denoised.release(); c->den_w = c->den_h = 0;      // the denoised frame goes with the planes that guided it
    c->d_temporal.release(); c->temporal_w = c->temporal_h = 0;      // ... and so does the temporal history
    c->d_motion.release(); c->motion_w = c->motion_h = 0;            // ... and the motion planes
    c->d_temporal_mm.release(); c->temporal_moments = c->temporal_variance = false;      // ... and the moments and the variance
    c->d_display.release(); c->disp_w = c->disp_h = 0;               // ... and the display image (the exposure state stays)
    // ... and the guide planes with the upsampled frame
    for (auto& b : c->d_guide) b.release();
    c->d_guide_primary.release();
    c->guide_w = c->guide_h = 0; c->guide_mask = 0;
    c->d_upsampled.release(); c->ups_w = c->ups_h = 0;
}

// Brings the primary-visibility cache up to date where it is valid and hands it to p; else p keeps walking from the camera.
int use_primary_cache(ptk_ctx* c, RenderParams& p)
{
    if (!primary_cacheable(c)) return PTK_OK;
    if (c->primary_hit_dirty)
    {
        launch_primary_hits(p, c->d_primary_hit, c->d_primary_rd, c->stream);
        HIPCHK(c, hipGetLastError());
        c->primary_hit_dirty = false;
        c->hit_generation++;
        c->out_full_next = true;
        c->inputs_dirty = true;
    }
    p.primary_hit = c->d_primary_hit; p.primary_rd = c->d_primary_rd;
    return PTK_OK;
}

// the plane `feature` of the last ptk_render_features, or null with the reason in the context's error text
void* feature_plane(ptk_ctx* c, int feature, size_t* bytes)
{
    if (feature < 0 || feature >= NUM_FEATURES) { fail(c, PTK_ERR_BAD_ARG, "unknown feature id"); return nullptr; }
    if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
    { fail(c, PTK_ERR_BAD_ARG, "no feature planes for the current resolution: ptk_render_features first"); return nullptr; }
    if (!((c->feat_mask >> feature) & 1u) || !c->d_feat[feature])
    { fail(c, PTK_ERR_BAD_ARG, "this feature was not in the mask of the last ptk_render_features"); return nullptr; }
    *bytes = (size_t)c->feat_w * c->feat_h * kFeatChannels[feature] * 4;
    return c->d_feat[feature];
}

// what the first geometry update derives from a tree's topology; dropped with the tree
void free_geometry_cache(ptk_ctx* c)
{
    c->d_tri_pos.release(); c->d_level_nodes.release(); c->d_refit_side.release(); c->d_refit_partial.release();
    c->level_start.clear();
    c->geo_updates = 0; c->sah_built = c->sah_now = 0.0; c->sah_now_pending = false;
}

void free_adaptive(ptk_ctx* c)
{
    c->d_counts.release(); c->d_moments.release(); c->d_adapt_active.release(); c->d_adapt_traced.release(); c->d_adapt_list.release();
    c->d_adapt_stats.release();
    c->adapt_capacity = 0;
    c->adaptive_accum = false;
}

int owned_tiles(const RenderParams& p)
{
    // tiles t with t % world == rank
    if (p.num_tiles <= p.rank) return 0;
    return (p.num_tiles - p.rank + p.world - 1) / p.world;
}

// One round of an adaptive render (ptk_render_adaptive): the trace kernels are fed the round's traced mask and list, the adaptive
// accumulate kernel folds S1 / S2 and counts for the active set.  init: before the first round, converge_kernel sets the active
// set to every owned pixel and derives the traced mask from the live mask of a plain render (which run_passes brings up to date).
struct AdaptiveRound
{
    AdaptiveParams a;
    ConvergeParams cp;
    bool init;
};

// One pass = trace_kernel over (owned tiles x 4 quadrants x chunks) + accumulate_kernel.  The pass
// size is bounded by the sample-buffer budget; chunk boundaries never change results (the RNG is
// keyed on the absolute sample index and the accumulate kernel adds in sample order).
int run_passes(ptk_ctx* c, uint32_t first, uint32_t spp, uint64_t seed, bool stats, float* accum, uint8_t* rgb8,
               const uint32_t* exit_flag, bool timed, const AdaptiveRound* ad = nullptr)
{
    RenderParams p;
    fill_params(c, p, first, spp, seed);
    p.accum = accum; p.rgb8 = rgb8; p.exit_flag = exit_flag;
    if (const int rc = use_primary_cache(c, p); rc != PTK_OK) return rc;
    // decided per render from the staged state: a material edit, a new scene or an opened aperture since the last one is seen here
    p.plain = (c->opt_plain_kernel && c->scene_plain && p.flat_count > 0 && p.primary_hit != nullptr) ? 1 : 0;
    // the exact build's pair-pass unit, or the cycle unit around the same pass (launch_trace; the contracted builds have neither) - the
    // cycle unit only while the tables its shade block reads by 32-bit byte offsets are below 2^32 bytes (ptk_table_offset.h)
    if (p.plain && c->opt_flat_rect_pairs) p.plain = (c->opt_flat_cycle && cycle_unit_tables_fit(c->width, c->height, (uint64_t)c->h_materials.size() * MAT_F4)) ? 3 : 2;
    p.lambert = (p.plain && c->opt_lambert_kernel && c->scene_lambert) ? 1 : 0;
    if (!c->pixel_rng_valid || c->pixel_rng_seed != seed)
    {
        launch_pixel_rng((uint32_t)seed, (uint32_t)(seed >> 32), c->width * c->height, c->d_pixel_rng, c->stream);
        HIPCHK(c, hipGetLastError());
        c->pixel_rng_seed = seed; c->pixel_rng_valid = true;
        c->inputs_dirty = true;
    }
    p.pixel_rng = c->d_pixel_rng;
    GlMapping glmap{ c };
    uint8_t* handoff = nullptr;
    if (rgb8 == c->d_rgb8)
    {
        handoff = c->out_host_dev ? c->out_host_dev : c->out_device;
        if (!handoff && c->gl_res)
        {
            HIPCHK(c, hipGraphicsMapResources(1, &c->gl_res, c->stream));
            glmap.mapped = true;
            void* ptr = nullptr; size_t bytes = 0;
            HIPCHK(c, hipGraphicsResourceGetMappedPointer(&ptr, &bytes, c->gl_res));
            if (!ptr || bytes < (size_t)c->width * c->height * 3)
                return fail(c, PTK_ERR_BAD_ARG, "the bound OpenGL buffer holds fewer than width * height * 3 bytes");
            handoff = (uint8_t*)ptr;
        }
    }
    if (handoff)
    {
        // (after the primary-hit cache has been brought up to date: a recomputed cache changes which pixels are always black)
        p.rgb8_host = handoff; p.rgb8_host_full = c->out_full_next.exchange(false) ? 1 : 0;
    }
    const int tiles = owned_tiles(p);
    c->last_passes = 0; c->last_launches = 0;
    if (tiles == 0) return PTK_OK;
    {
        // the list of quadrants with live pixels: rebuilt when the frame, the tile ownership or the cached camera hits change
        const int subtiles = tiles * 4;
        if (subtiles > c->live_capacity)
        {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            c->d_live_mask.release(); c->d_live_list.release(); c->live_capacity = 0;
            if (const int rc = c->d_live_mask.alloc(c, (size_t)subtiles); rc != PTK_OK) return rc;
            if (const int rc = c->d_live_list.alloc(c, (size_t)subtiles + 1); rc != PTK_OK) return rc;
            c->live_capacity = subtiles;
            c->live_key.rank = -1;
        }
        // (uncached cameras: the mask holds the pixels whose lens rays can reach the scene at all - it follows camera, frame and scene)
        const ptk_ctx::LiveKey key = { c->width, c->height, c->rank, c->world, p.primary_hit ? 1 : (p.lens_cull ? 2 : 0),
                                       p.primary_hit ? c->hit_generation : (p.lens_cull ? c->view_generation : 0ull) };
        const ptk_ctx::LiveKey& o = c->live_key;
        if (key.width != o.width || key.height != o.height || key.rank != o.rank || key.world != o.world || key.cached != o.cached ||
            key.generation != o.generation)
        {
            launch_live_list(p, subtiles, c->d_live_mask, c->d_live_list, c->d_live_list + c->live_capacity, c->stream);
            HIPCHK(c, hipGetLastError());
            c->live_key = key;
            c->inputs_dirty = true;
        }
        p.live_mask = c->d_live_mask; p.live_list = c->d_live_list; p.live_count = c->d_live_list + c->live_capacity;
        if (ad)
        {
            // (kept apart from the cached list above: a plain render after this one finds it as it was)
            unsigned* count = c->d_adapt_list + c->adapt_capacity;
            if (ad->init)
            {
                ConvergeParams cp = ad->cp;
                cp.base = c->d_live_mask; cp.init = 1; cp.test = 0;
                launch_converge(p, cp, tiles, c->stream);
                HIPCHK(c, hipGetLastError());
                launch_compact_list(c->d_adapt_traced, subtiles, c->d_adapt_list, count, c->stream);
                HIPCHK(c, hipGetLastError());
            }
            p.live_mask = c->d_adapt_traced; p.live_list = c->d_adapt_list; p.live_count = count;
        }
    }
    const size_t per_sample = (size_t)tiles * 4 * 64 * sizeof(float4);
    // Samples per work item.  The waves are persistent and lanes take units from item after item, so short items
    // cost no SIMD utilisation any more; what they buy is balance at the end of the launch (the last items are
    // the tail) and concurrency on the same pixels.  8 is the measured optimum for whole frames (C2, C4); a rank
    // that owns 1/4 or 1/8 of the tiles does better with 4.  Each item costs one queue pop (~2 us of latency).
    int chunk_opt = c->opt_chunk;
    if (chunk_opt <= 0)
        chunk_opt = (double)spp * (double)tiles * 4.0 / 8.0 >= 49152.0 ? 8 : 4;
    // (a bound hand-off buffer means the caller waits for every frame: nothing to overlap, and one stream is two event
    // hops per frame less)
    // (nor in an adaptive render: each round depends on the one before)
    const bool overlap = c->opt_overlap != 0 && c->trace_stream[0].s != nullptr && !handoff && !ad;
    // The pass size: what the sample-buffer budget allows - and what the device can actually give.  When an allocation of that
    // size fails (memory shared with the caller's framework, a huge scene, a 144-megapixel frame) the pass is halved and tried
    // again instead of failing the render: more passes, the same image (chunk boundaries never change a bit).
    size_t budget = c->opt_pass_bytes;
    {
        const size_t have = overlap ? std::min(c->d_samples2[0].cap, c->d_samples2[1].cap) : c->d_samples.cap;
        const size_t want = std::min(budget, per_sample * ((size_t)spp + (size_t)chunk_opt));      // (what this render asks for at most)
        size_t free_b = 0, total_b = 0;
        if (want > have)             // (only a render that has to allocate asks the driver: the interactive loop never does)
        {
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess)
            {
                // the buffers still to be allocated may take at most half of what is free now (there are two of them when overlapping)
                const size_t share = free_b / (overlap ? 4 : 2);
                if (budget > std::max(share, have)) budget = std::max(share, have);
            }
            else (void)hipGetLastError();
        }
    }
    uint32_t max_pass = (uint32_t)std::max<size_t>(1, budget / per_sample);
    if (max_pass > (uint32_t)chunk_opt) max_pass -= max_pass % (uint32_t)chunk_opt;
    // grows buf to `need` bytes; false (nothing allocated, capacity 0) when the device refuses
    auto grow = [&](Buf<float4>& buf, size_t need) -> bool {
        if (buf.try_alloc(need, need) == hipSuccess) return true;
        (void)hipGetLastError();
        return false;
    };
    uint32_t done = 0;
    while (done < spp)
    {
        uint32_t n = std::min(spp - done, max_pass);
        int chunk = (int)std::min<uint32_t>(n, (uint32_t)chunk_opt);
        int num_chunks = (int)((n + chunk - 1) / chunk);
        size_t need = per_sample * (size_t)chunk * num_chunks;
        const int b = (int)(c->pass_counter & 1u);
        hipStream_t tstream = overlap ? c->trace_stream[b] : c->stream;
        for (;;)
        {
            bool ok = true;
            if (overlap)
            {
                // BOTH buffers are brought to size together: the second one would otherwise be allocated - a blocking call of tens of
                // milliseconds for gigabytes - in the middle of the second render (BENCH_r03: C3's first timed steps)
                if (need > c->d_samples2[0].cap || need > c->d_samples2[1].cap)
                {
                    HIPCHK(c, hipStreamSynchronize(c->trace_stream[0]));
                    HIPCHK(c, hipStreamSynchronize(c->trace_stream[1]));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    for (int k = 0; k < 2 && ok; k++)
                        if (need > c->d_samples2[k].cap) ok = grow(c->d_samples2[k], need);
                }
            }
            else if (need > c->d_samples.cap)
            {
                HIPCHK(c, hipStreamSynchronize(c->stream));
                ok = grow(c->d_samples, need);
            }
            if (ok) break;
            if (n <= (uint32_t)chunk && chunk <= 1) return fail(c, PTK_ERR_HIP, "hipMalloc: no memory for the sample buffer of even one sample per pixel");
            // halve the pass (whole chunks while there are several, then the chunk itself) and try again
            if (n > (uint32_t)chunk) { n = std::max<uint32_t>((uint32_t)chunk, (n / 2) / (uint32_t)chunk * (uint32_t)chunk); }
            else { chunk = std::max(1, chunk / 2); n = (uint32_t)chunk; }
            max_pass = n;
            num_chunks = (int)((n + chunk - 1) / chunk);
            need = per_sample * (size_t)chunk * num_chunks;
        }
        if (overlap)
        {
            p.samples = c->d_samples2[b];
            if (c->inputs_dirty || !c->inputs_recorded)
            {
                HIPCHK(c, hipEventRecord(c->ev_inputs, c->stream));
                c->inputs_dirty = false; c->inputs_recorded = true;
            }
            HIPCHK(c, hipStreamWaitEvent(tstream, c->ev_inputs, 0));
            if (c->acc_pending[b]) HIPCHK(c, hipStreamWaitEvent(tstream, c->ev_acc_done[b], 0));   // buffer b was last read by pass k-2's accumulate
        }
        else p.samples = c->d_samples;
        p.first_sample = first + done; p.spp = n;
        p.chunk = chunk; p.num_chunks = num_chunks;
        p.resolve_samples = (float)(first + done + n);
        const long long items = (long long)tiles * 4 * num_chunks;
        if (items > (1ll << 30)) return fail(c, PTK_ERR_LIMIT, "too many work items in one pass");
        p.num_items = (int)items;
        const int pi = c->last_passes < ptk_ctx::kMaxTimedPasses ? c->last_passes : -1;
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev.at(pi, 0), tstream));
        const int kl = (!stats && (size_t)(2 * c->klog_n + 1) < c->klog_ev.size()) ? c->klog_n : -1;
        if (kl >= 0) HIPCHK(c, hipEventRecord(c->klog_ev[2 * kl], tstream));
        p.queues = overlap ? c->d_queues2[b] : c->d_queues;
        if (c->opt_contract == 1 && !stats) fma::launch_trace(p, tiles * 4, c->resident_waves, tstream, false);
        else if (c->opt_contract == 2 && !stats) fast::launch_trace(p, tiles * 4, c->resident_waves, tstream, false);
        else launch_trace(p, tiles * 4, c->resident_waves, tstream, stats);
        HIPCHK(c, hipGetLastError());
        c->last_trace_variant = p.flat_count <= 0 ? PTK_TRACE_BVH : ((p.plain && !stats) ? PTK_TRACE_FLAT_PLAIN : PTK_TRACE_FLAT);
        c->last_trace_lambert = p.flat_count > 0 && p.plain && p.lambert && !stats;
        c->last_trace_unit = (p.flat_count > 0 && p.plain && !stats && c->opt_contract == 0) ? (p.plain == 3 ? PTK_UNIT_CYCLE : p.plain == 2 ? PTK_UNIT_RECT : PTK_UNIT_PLAIN) : PTK_UNIT_NONE;
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev.at(pi, 1), tstream));
        if (kl >= 0) { HIPCHK(c, hipEventRecord(c->klog_ev[2 * kl + 1], tstream)); c->klog_n = kl + 1; }
        if (overlap)
        {
            HIPCHK(c, hipEventRecord(c->ev_trace_done[b], tstream));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_trace_done[b], 0));
        }
        if (ad) launch_accumulate_adaptive(p, ad->a, tiles, c->stream);
        else launch_accumulate(p, tiles, c->stream);
        HIPCHK(c, hipGetLastError());
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev.at(pi, 2), c->stream));
        if (overlap)
        {
            HIPCHK(c, hipEventRecord(c->ev_acc_done[b], c->stream));
            c->acc_pending[b] = true;
            c->pass_counter++;
        }
        c->last_passes++; c->last_launches += 3;            // queue_init_kernel (queue + parameter block), trace, accumulate
        done += n;
    }
    return PTK_OK;
}

}  // namespace

int ptk::ensure_primary(ptk_ctx* c)
{
    if (!c->primary_dirty) return PTK_OK;
    if (!c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    PrimaryParams pp;
    frame_setup(c, pp);
    launch_primary(pp, c->stream);
    HIPCHK(c, hipGetLastError());
    c->primary_dirty = false;
    c->view_generation++;
    c->primary_hit_dirty = true;
    c->inputs_dirty = true;
    return PTK_OK;
}

void ptk::frame_view(ptk_ctx* c, PrimaryParams& pp) { frame_setup(c, pp); }
void ptk::frame_view_at(const ptk_ctx* c, int width, int height, PrimaryParams& pp) { frame_setup_at(c, width, height, pp); }

void ptk::fill_params(ptk_ctx* c, RenderParams& p, uint32_t first, uint32_t spp, uint64_t seed)
{
    std::memset(&p, 0, sizeof(p));
    p.nodes = c->d_nodes; p.tris = c->d_tris; p.flat_tris = c->d_flat_tris; p.shade = c->d_shade; p.mats = c->d_mats; p.lights = c->d_lights;
    p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.primary = c->d_primary;
    p.primary_hit = nullptr;
    p.samples = c->d_samples;
    // shallow trees give short, uniform walks: waiting for stragglers is cheap and re-synchronises the
    // wave (lambda 25); deep trees have heavy-tailed walks: shade small batches early (lambda 5)
    // lambda of the ski-rental rule = cost(shade block) / cost(one walk iteration), in eighths: a walk iteration of a tree far
    // larger than the L2 waits for memory and costs more, so the shade block is run for smaller batches there (measured
    // optimum: ~72 for 10-20 k nodes, ~46 for 370 k nodes; flat within 1 % around either)
    p.shade_thr = c->opt_shade_thr > 0 ? c->opt_shade_thr : (c->bvh_depth <= 4 ? 200 : (c->num_nodes >= 131072 ? 46 : 68));
    p.gen_thr = c->opt_gen_thr;
    p.tri_thr = c->opt_tri_thr;
    p.max_batch = c->opt_max_batch;
    p.persistent = c->opt_persistent;
    p.generations = c->opt_generations > 0 ? c->opt_generations : (c->world > 1 ? 2 : 1);
    p.rgb8_host = nullptr; p.rgb8_host_full = 1;
    p.accum = accum_ptr(c); p.rgb8 = c->d_rgb8; p.exit_flag = c->d_exit; p.exit_gen = c->render_gen.load(); p.stats = c->d_stats;
    p.num_nodes = c->num_nodes; p.num_lights = c->num_lights; p.scene_bound = c->scene_bound;
    for (int a = 0; a < 3; a++) { p.scene_lo[a] = c->scene_lo[a]; p.scene_hi[a] = c->scene_hi[a]; }
    p.lens_cull = c->opt_lens_cull;
    p.flat_count = (c->opt_flat && c->num_tris <= 16 && c->d_flat_tris) ? c->num_tris : 0;
    p.flat_shade_w = c->opt_flat_shade_w; p.flat_gen_w = c->opt_flat_gen_w;
    p.width = c->width; p.height = c->height; p.max_depth = c->max_depth;
    p.tiles_x = (c->width + PTK_TILE - 1) / PTK_TILE;
    p.num_tiles = p.tiles_x * ((c->height + PTK_TILE - 1) / PTK_TILE);
    p.rank = c->rank; p.world = c->world;
    p.first_sample = first; p.spp = spp;
    p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    for (int a = 0; a < 3; a++) { p.cam_pos[a] = c->cam_pos[a]; p.cam_right[a] = c->cam_right[a]; p.cam_up[a] = c->cam_up[a]; }
    p.focal_dist = c->focal_dist; p.aperture = c->aperture;
    p.resolve_samples = (float)(first + spp);
}

extern "C" {

int ptk_create(ptk_ctx** out, int device_ordinal)
{
    if (!out) return PTK_ERR_BAD_ARG;
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0) return PTK_ERR_HIP;
    if (device_ordinal < 0 || device_ordinal >= ndev) return PTK_ERR_BAD_ARG;
    if (hipSetDevice(device_ordinal) != hipSuccess) return PTK_ERR_HIP;
    ptk_ctx* c = new (std::nothrow) ptk_ctx();
    if (!c) return PTK_ERR_HIP;
    c->device = device_ordinal;
    if (c->stream_own.create(hipStreamNonBlocking) != hipSuccess) { delete c; return PTK_ERR_HIP; }
    c->stream = c->stream_own; c->own_stream = true;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0)
            c->resident_waves = cus * 16;        // 4 SIMDs x 4 waves of the BVH trace kernel per CU (launch_trace scales it to x 5 for the FLAT kernel)
        if (cus > 0) c->num_cus = cus;
    }
    // (ptk_destroy copes with a context of which only some members were made)
    bool ok = c->d_exit.alloc(c, 1) == PTK_OK && hipMemset(c->d_exit, 0, sizeof(uint32_t)) == hipSuccess &&
              c->h_exit.alloc(1) == hipSuccess && c->d_stats.alloc(c, 16) == PTK_OK &&
              c->d_queues.alloc_bytes(c, PTK_QUEUE_BLOCK_BYTES, 0) == PTK_OK;
    if (ok) *c->h_exit = 0;
    ok = ok && c->ev.reserve(c, ptk_ctx::kMaxTimedPasses) == PTK_OK;
    for (int b = 0; b < 2; b++)
        ok = ok && c->trace_stream[b].create(hipStreamNonBlocking) == hipSuccess &&
             c->ev_trace_done[b].create(hipEventDisableTiming) == hipSuccess && c->ev_acc_done[b].create(hipEventDisableTiming) == hipSuccess &&
             c->d_queues2[b].alloc_bytes(c, PTK_QUEUE_BLOCK_BYTES, 0) == PTK_OK;
    ok = ok && c->ev_inputs.create(hipEventDisableTiming) == hipSuccess;
    ok = ok && c->geo_stream.create(hipStreamNonBlocking) == hipSuccess &&
         c->d_geo_red.alloc(c, GEO_RED_WORDS, sizeof(double)) == PTK_OK && c->h_geo_red.alloc(GEO_RED_WORDS) == hipSuccess;
    for (Event& e : c->ev_geo_t.ev) ok = ok && e.create() == hipSuccess;
    int lo = 0, hi = 0;                          // (numerically lowest = greatest priority)
    (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
    ok = ok && c->xstream.create(hipStreamNonBlocking, hi) == hipSuccess && c->exit_stream.create(hipStreamNonBlocking, hi) == hipSuccess &&
         c->ev_rendered.create(hipEventDisableTiming) == hipSuccess && c->ev_packed.create(hipEventDisableTiming) == hipSuccess &&
         c->ev_gathered.create(hipEventDisableTiming) == hipSuccess;
    if (!ok) { ptk_destroy(c); return PTK_ERR_HIP; }
    *out = c;
    return PTK_OK;
}

void ptk_destroy(ptk_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    for (const Stream* s : { &c->trace_stream[0], &c->trace_stream[1], &c->geo_stream, &c->xstream, &c->exit_stream }) s->sync();
    unbind_out_image(c);
    comm_release(c);                             // (before xstream goes)
    delete c;
}

const char* ptk_last_error(ptk_ctx* c)
{
    if (!c) return "null context";
    std::lock_guard<std::mutex> g(c->err_mu);
    return c->error.c_str();
}

int ptk_set_stream(ptk_ctx* c, void* s)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->own_stream) c->stream_own.release();
    else if ((hipStream_t)s != c->stream)
    {
        // from one caller stream to another, with no host wait: the new stream goes on behind everything queued on the old one
        // (accumulate kernels of the renders in flight, whose trace kernels run on the internal streams), so that the next
        // accumulate kernel adds to a finished accumulator and the caller's work on the new stream sees every batch, in order
        HIPCHK(c, hipEventRecord(c->ev_inputs, c->stream));
        HIPCHK(c, hipStreamWaitEvent((hipStream_t)s, c->ev_inputs, 0));
    }
    c->stream = (hipStream_t)s;
    c->own_stream = false;
    c->inputs_dirty = true;                      // re-anchor the trace streams behind the new stream
    return PTK_OK;
}

int ptk_upload_scene(ptk_ctx* c, const ptk_scene_desc* s)
{
    if (!c || !s) return PTK_ERR_BAD_ARG;
    const int32_t n = s->num_triangles;
    if (n < 0 || s->num_materials < 0 || s->num_textures < 0 || s->num_lights < 0)
        return fail(c, PTK_ERR_BAD_ARG, "negative count in scene description");
    if (n > 0 && (!s->verts || !s->normals || !s->uvs || !s->tbn || !s->smoothing || !s->material || !s->materials))
        return fail(c, PTK_ERR_BAD_ARG, "null triangle/material array");
    // (the walk addresses triangle and node records with 32-bit BYTE offsets from wave-uniform bases - ptk_device_fn.h
    // request_node / walk_step - so a record array ends below 4 GiB: 89 478 485 triangles of 48 bytes; checked before anything
    // reads the arrays.  The node array of such a scene, ~0.4 nodes of 64 bytes per triangle, stays below that by itself and is
    // checked once it exists)
    if ((uint64_t)n * (uint64_t)(TRI_F4 * sizeof(float4)) > 0xffffffffull)
        return fail(c, PTK_ERR_LIMIT, "more triangles than the kernels' 32-bit record offsets address (89 478 485)");
    if (s->num_lights > 0 && !s->lights) return fail(c, PTK_ERR_BAD_ARG, "null light array");
    // (a scene whose textures are ALL missing files - a .pts moved to another machine - has texture entries of zero extent and not
    // one texel: no atlas to point to)
    if (s->num_textures > 0 && (!s->textures || (!s->texels && s->texel_bytes > 0))) return fail(c, PTK_ERR_BAD_ARG, "null texture array");
    for (int32_t i = 0; i < n; i++)
        if (s->material[i] < 0 || s->material[i] >= s->num_materials)
            return fail(c, PTK_ERR_BAD_ARG, "triangle material index out of range");
    for (int32_t i = 0; i < s->num_lights; i++)
        if (s->lights[i] < 0 || s->lights[i] >= n) return fail(c, PTK_ERR_BAD_ARG, "light triangle index out of range");
    // the kernels' exact short reciprocal (ptk_device_fn.h rcp_ieee) covers determinants and lengths up to 2^126: coordinates
    // must stay below 2^61 in magnitude (the reference's own float arithmetic is long meaningless out there)
    float vmax = 0.0f;
    float vlo[3] = { INFINITY, INFINITY, INFINITY }, vhi[3] = { -INFINITY, -INFINITY, -INFINITY };
    for (size_t i = 0; i < (size_t)n * 9; i++)
    {
        const float v = s->verts[i];
        if (!(std::fabs(v) < 2.305843e18f)) return fail(c, PTK_ERR_LIMIT, "vertex coordinate is not finite or exceeds 2^61");
        vmax = std::max(vmax, std::fabs(v));
        const int a = (int)(i % 3);
        vlo[a] = std::min(vlo[a], v); vhi[a] = std::max(vhi[a], v);
    }
    // (node origins lie within the triangle boxes padded by 1e-5 x their extent plus the degenerate-box epsilon)
    const float scene_bound = 3.1f * (1.01f * vmax + 1e-3f);
    for (int32_t i = 0; i < s->num_textures; i++)
    {
        const ptk_texture& t = s->textures[i];
        if (t.width < 0 || t.height < 0 || t.offset < 0 || (t.offset & 3) ||
            t.offset + (int64_t)t.width * t.height * 4 > s->texel_bytes)
            return fail(c, PTK_ERR_BAD_ARG, "texture outside the texel atlas");
    }
    for (int32_t i = 0; i < s->num_materials; i++)
        for (int k = 0; k < 6; k++)
            if (s->materials[i].tex[k] >= s->num_textures) return fail(c, PTK_ERR_BAD_ARG, "material texture index out of range");

    HIPCHK(c, hipSetDevice(c->device));
    // The one wait before the resident scene is freed, and why the context's stream is enough.  Everything that reads scene
    // buffers is either on this stream or tied to it before its entry returns:
    //  - trace kernels on trace_stream[0 / 1] (run_passes): each is followed by ev_trace_done, which this stream waits for ahead
    //    of the pass's accumulate kernel - also for a render that ptk_request_exit cuts short: its kernels still run and stand
    //    down, and the accumulate kernels are queued all the same.  ptk_collect_stats drains both trace streams itself;
    //  - feature, guide, pick, query, bake, probe, surface, motion, denoise, temporal, display and upsample kernels: on this stream;
    //  - ptk_update_geometry: geo_stream only stages the caller's arrays and reduces bounds, and the update waits for it on the
    //    host before it returns; repack and refit are on this stream;
    //  - xstream (ptk_gather_accum) reads the accumulator and its own buffers, exit_stream writes d_exit: no scene buffer;
    //  - a caller's stream taken by ptk_set_stream stands behind the one it replaced (ev_inputs), so "this stream" is the newest.
    // So once this stream is idle nothing on the device still reads what is released below.
    HIPCHK(c, hipStreamSynchronize(c->stream));

    const auto t_begin = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    // BVH: on the device for scenes large enough to matter (replaces BVHNode::Construct, mesh.cpp:169-211), else - or when
    // the device build cannot meet the traversal-stack bound - by the host builder, which always can
    BuiltBvh bvh;
    DeviceBvh dbvh;
    bool on_device = false;
    // what a device build holds until the context takes it over or the call ends: the staged vertices, the builder's two arrays
    Buf<float> d_verts; Buf<float4> d_bvh_nodes; Buf<int32_t> d_bvh_order;
    if (c->opt_device_build && n >= 4096)
    {
        if (const int rc = d_verts.alloc(c, (size_t)n * 9); rc != PTK_OK) return rc;
        HIPCHK(c, hipMemcpyAsync(d_verts, s->verts, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        std::string derr;
        int leaf_max = 4;
        if (g_bvh_tuning.leaf_max > 0) leaf_max = g_bvh_tuning.leaf_max;                              // ptk_set_option "bvh_leaf_max"
        on_device = build_bvh_device(d_verts, n, PTK_MAX_BVH_DEPTH, leaf_max, c->stream, dbvh, &derr);
        if (on_device) { d_bvh_nodes.adopt(dbvh.d_nodes); d_bvh_order.adopt(dbvh.d_order); }
        if (on_device && dbvh.stack_need > PTK_MAX_BVH_DEPTH) { d_bvh_nodes.release(); d_bvh_order.release(); on_device = false; }
    }
    if (!on_device)
    {
        if (!build_bvh(s->verts, n, PTK_MAX_BVH_DEPTH, 4, bvh))
            return fail(c, PTK_ERR_LIMIT, "BVH exceeds the kernel's depth / index limits");
        if (bvh.stack_need > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    }
    if ((uint64_t)(on_device ? dbvh.num_nodes : bvh.num_nodes) * (uint64_t)(NODE_F4 * sizeof(float4)) > 0xffffffffull)
        return fail(c, PTK_ERR_LIMIT, "more BVH nodes than the kernels' 32-bit record offsets address");

    c->upload_ms[0] = ms_since(t_begin);
    const auto t_pack = std::chrono::steady_clock::now();
    // a texture with zero extent behaves like a missing image: tex2D returns 0 (image.cpp:65-66);
    // staged as a 1x1 black texel so the kernel needs no special case
    std::vector<int32_t> texmap(s->num_textures, -1);
    std::vector<int4> texinfo;
    std::vector<uint32_t> texels;
    texels.push_back(0u);                                   // texel 0: shared black texel
    for (int32_t i = 0; i < s->num_textures; i++)
    {
        const ptk_texture& t = s->textures[i];
        int4 ti;
        if (t.width == 0 || t.height == 0) { ti = make_int4(1, 1, 0, 0); }
        else
        {
            ti = make_int4(t.width, t.height, (int)texels.size(), 0);
            size_t cnt = (size_t)t.width * t.height;
            size_t base = texels.size();
            texels.resize(base + cnt);
            std::memcpy(texels.data() + base, s->texels + t.offset, cnt * 4);
        }
        texmap[i] = (int32_t)texinfo.size();
        texinfo.push_back(ti);
    }
    if (texels.size() >= (1ull << 31)) return fail(c, PTK_ERR_LIMIT, "texel atlas too large");

    std::vector<float> mats((size_t)s->num_materials * MAT_F4 * 4, 0.0f);
    for (int32_t i = 0; i < s->num_materials; i++) pack_material(s->materials[i], texmap, mats.data() + (size_t)i * MAT_F4 * 4);

    std::vector<float> tris, shade;
    c->num_leaf_tris = n;
    if (!on_device) tris.assign((size_t)n * TRI_F4 * 4, 0.0f);
    for (int32_t k = 0; k < n && !on_device; k++)
    {
        int32_t i = bvh.order[k];
        const float* v = s->verts + (size_t)i * 9;
        float* q = tris.data() + (size_t)k * TRI_F4 * 4;
        q[0] = v[0]; q[1] = v[1]; q[2] = v[2];
        q[3] = v[3] - v[0]; q[4] = v[4] - v[1]; q[5] = v[5] - v[2];      // edge1 = v2 - v1 (pathtracer.cpp:382)
        q[6] = v[6] - v[0]; q[7] = v[7] - v[1]; q[8] = v[8] - v[2];      // edge2 = v3 - v1 (pathtracer.cpp:383)
        q[9] = as_float(i);
        int32_t ot = s->materials[s->material[i]].tex[5];
        q[10] = as_float(ot >= 0 ? texmap[ot] : -1);
        q[11] = 0.0f;
    }
    if (!on_device) shade.assign((size_t)n * SHADE_F4 * 4, 0.0f);
    for (int32_t i = 0; i < n && !on_device; i++)
    {
        const float* nn = s->normals + (size_t)i * 9;
        const float* uv = s->uvs + (size_t)i * 6;
        const float* tb = s->tbn + (size_t)i * 9;
        float* q = shade.data() + (size_t)i * SHADE_F4 * 4;
        q[0] = tb[0]; q[1] = tb[1]; q[2] = tb[2];
        q[3] = as_float((int32_t)((uint32_t)s->material[i] | (s->smoothing[i] ? 0x80000000u : 0u)));
        q[4] = uv[0]; q[5] = uv[1]; q[6] = uv[2]; q[7] = uv[3];
        q[8] = uv[4]; q[9] = uv[5]; q[10] = nn[0]; q[11] = nn[1];
        q[12] = nn[2]; q[13] = nn[3]; q[14] = nn[4]; q[15] = nn[5];
        q[16] = nn[6]; q[17] = nn[7]; q[18] = nn[8]; q[19] = tb[3];
        q[20] = tb[4]; q[21] = tb[5]; q[22] = tb[6]; q[23] = tb[7];
        q[24] = tb[8];
    }
    std::vector<float> lights((size_t)s->num_lights * LIGHT_F4 * 4, 0.0f);
    for (int32_t k = 0; k < s->num_lights; k++)
    {
        int32_t i = s->lights[k];
        const float* v = s->verts + (size_t)i * 9;
        const ptk_material& m = s->materials[s->material[i]];
        float* q = lights.data() + (size_t)k * LIGHT_F4 * 4;
        q[0] = v[0]; q[1] = v[1]; q[2] = v[2]; q[3] = as_float(i);
        q[4] = v[3]; q[5] = v[4]; q[6] = v[5]; q[7] = m.emissive[0] * m.emissive_intensity;    // pathtracer.cpp:528
        q[8] = v[6]; q[9] = v[7]; q[10] = v[8]; q[11] = m.emissive[1] * m.emissive_intensity;
        q[12] = m.emissive[2] * m.emissive_intensity;
        q[13] = as_float(m.tex[5] >= 0 ? texmap[m.tex[5]] : -1);          // its opacity texture (the shadow walk tests the light triangle first)
    }

    c->upload_ms[1] = ms_since(t_pack);
    const auto t_copy = std::chrono::steady_clock::now();
    c->d_nodes.release(); c->d_tris.release(); c->d_shade.release(); c->d_mats.release(); c->d_lights.release();
    c->d_texinfo.release(); c->d_texels.release();
    c->d_verts_res.release(); free_geometry_cache(c);
    c->d_verts_prev.release(); c->have_snapshot = false;             // (ptk_geometry_snapshot: of the scene that goes)
    surface_release(c);                                            // (ptk_sample_surface: its table and weights likewise)
    // ... and everything a frame entry derived from that scene - feature, guide and motion planes, the denoised, upsampled and
    // display frames, the temporal history with its moments and variance - exactly as ptk_set_frame at another resolution drops
    // it: triangle and material ids of the old scene mean nothing in the new one (ptk.h).  The exposure state stays
    free_features(c);
    c->lights_stale = false;
    c->have_scene = false;
    auto up = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
        size_t alloc = bytes ? bytes : 64;      // (never null: the walk reads node 0 unconditionally)
        hipError_t e = hipMalloc(dst, alloc);
        if (e != hipSuccess) return e;
        if (bytes) return hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice);
        return hipSuccess;
    };
    if (on_device)
    {
        c->d_flat_tris.release();
        // the records are packed on the device from the boundary's flat arrays (one pass each; no host-side copies)
        Buf<float> d_normals, d_uvs, d_tbn; Buf<uint8_t> d_smooth; Buf<int32_t> d_material, d_optex;       // (freed on the way out)
        std::vector<int32_t> optex(std::max<int32_t>(s->num_materials, 1), -1);
        for (int32_t i = 0; i < s->num_materials; i++) { const int32_t ot = s->materials[i].tex[5]; optex[i] = ot >= 0 ? texmap[ot] : -1; }
        auto tup = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
            hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
            if (e != hipSuccess) return e;
            return bytes ? hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
        };
        HIPCHK(c, tup((void**)&d_normals.p, s->normals, (size_t)n * 9 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_uvs.p, s->uvs, (size_t)n * 6 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_tbn.p, s->tbn, (size_t)n * 9 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_smooth.p, s->smoothing, (size_t)n));
        HIPCHK(c, tup((void**)&d_material.p, s->material, (size_t)n * sizeof(int32_t)));
        HIPCHK(c, tup((void**)&d_optex.p, optex.data(), optex.size() * sizeof(int32_t)));
        HIPCHK(c, hipMalloc(&c->d_tris.p, (size_t)n * TRI_F4 * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_shade.p, (size_t)n * SHADE_F4 * sizeof(float4)));
        launch_pack_tris(d_verts, d_bvh_order, d_material, d_optex, c->d_tris, n, c->stream);
        launch_pack_shade(d_normals, d_uvs, d_tbn, d_smooth, d_material, c->d_shade, n, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->d_nodes.adopt(d_bvh_nodes.p); d_bvh_nodes.p = nullptr;
        c->d_verts_res.adopt(d_verts.p); d_verts.p = nullptr;      // the builder's input stays resident (ptk_update_geometry)
        bvh.num_nodes = dbvh.num_nodes; bvh.depth = dbvh.depth; bvh.stack_need = dbvh.stack_need;
    }
    else
    {
        HIPCHK(c, up((void**)&c->d_nodes.p, bvh.nodes.data(), bvh.nodes.size() * 4));
        HIPCHK(c, up((void**)&c->d_tris.p, tris.data(), tris.size() * 4));
        c->d_flat_tris.release();
        if (n > 0 && n <= 16)
        {
            std::vector<float> flat((size_t)FLAT_TABLE_F4 * 4);     // records, room up to FLAT_MAX_TRIS, frame table, class table
            for (int32_t k = 0; k < n; k++)             // record of leaf position k holds triangle bvh.order[k]
                std::memcpy(flat.data() + (size_t)bvh.order[k] * TRI_F4 * 4, tris.data() + (size_t)k * TRI_F4 * 4, TRI_F4 * 16);
            HIPCHK(c, up((void**)&c->d_flat_tris.p, flat.data(), flat.size() * 4));
        }
        HIPCHK(c, up((void**)&c->d_shade.p, shade.data(), shade.size() * 4));
        if (c->d_flat_tris)                             // the frame table behind the flat records, from the normals just written
        {
            launch_flat_frames(c->d_shade, c->d_flat_tris, 0, n, c->stream);
            launch_flat_classes(c->d_flat_tris, n, c->opt_flat_zero_classes, c->opt_flat_rect_pairs, c->stream);     // ... and the class table and the pair word, from the records
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, up((void**)&c->d_verts_res.p, s->verts, (size_t)n * 9 * sizeof(float)));
    }
    c->built_on_device = on_device;
    HIPCHK(c, up((void**)&c->d_mats.p, mats.data(), mats.size() * 4));
    HIPCHK(c, up((void**)&c->d_lights.p, lights.data(), lights.size() * 4));
    HIPCHK(c, up((void**)&c->d_texinfo.p, texinfo.data(), texinfo.size() * sizeof(int4)));
    HIPCHK(c, up((void**)&c->d_texels.p, texels.data(), texels.size() * 4));
    c->num_nodes = bvh.num_nodes; c->num_tris = n; c->num_lights = s->num_lights; c->bvh_depth = bvh.depth; c->bvh_stack = bvh.stack_need;
    c->scene_bound = scene_bound;
    c->bvh_pad = 1e-5f * std::max(vmax, 1.0f);                     // bvh_build.cpp / bvh_device.hip: 1e-5 x max(1, largest |coordinate|)
    for (int a = 0; a < 3; a++) { c->scene_lo[a] = n > 0 ? vlo[a] : 0.0f; c->scene_hi[a] = n > 0 ? vhi[a] : 0.0f; }
    c->view_generation++;
    c->scene_has_opacity = false;
    for (int32_t i = 0; i < n; i++)
        if (s->materials[s->material[i]].tex[5] >= 0) { c->scene_has_opacity = true; break; }
    c->upload_ms[2] = ms_since(t_copy); c->upload_ms[3] = ms_since(t_begin);
    c->h_materials.assign(s->materials, s->materials + s->num_materials);
    c->h_texmap = texmap;
    c->h_lights = lights;
    c->h_flat_smoothing.clear(); c->h_flat_material.clear();
    if (n > 0 && n <= 16) { c->h_flat_smoothing.assign(s->smoothing, s->smoothing + n); c->h_flat_material.assign(s->material, s->material + n); }
    c->scene_plain = plain_tables(n, s->smoothing, s->material, s->num_materials, s->materials);
    c->scene_lambert = lambert_tables(n, s->smoothing, s->material, s->num_materials, s->materials);
    c->h_light_material.resize(s->num_lights);
    for (int32_t k = 0; k < s->num_lights; k++) c->h_light_material[k] = s->material[s->lights[k]];
    c->primary_hit_dirty = true;
    c->have_scene = true;
    c->inputs_dirty = true;
    return PTK_OK;
}

// Material edits after BuildBVH: in the reference `Triangle::mat` points into mLoadedObjects, so a SetMaterial is seen by
// the very next RenderFrame() without a rebuild, while the light LIST stays the one BuildBVH collected
// (pathtracer.cpp:250-258, :267-273, :528).  Same here: the material table and the lights' colours are rewritten in
// place; geometry, BVH, textures and the light list are untouched.  Texture bindings must be the uploaded ones.
int ptk_update_materials(ptk_ctx* c, int32_t num_materials, const ptk_material* materials)
{
    if (!c || !materials) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (num_materials != (int32_t)c->h_materials.size()) return fail(c, PTK_ERR_BAD_ARG, "material count differs from the uploaded scene");
    for (int32_t i = 0; i < num_materials; i++)
        for (int k = 0; k < 6; k++)
            if (materials[i].tex[k] != c->h_materials[i].tex[k])
                return fail(c, PTK_ERR_BAD_ARG, "texture bindings changed: upload the scene again");
    HIPCHK(c, hipSetDevice(c->device));
    if (c->lights_stale && !c->h_lights.empty())
    {
        // a geometry update moved light triangles on the device: take their vertices back before the records are rewritten whole
        HIPCHK(c, hipMemcpyAsync(c->h_lights.data(), c->d_lights, c->h_lights.size() * 4, hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
    }
    c->lights_stale = false;
    std::vector<float> mats((size_t)num_materials * MAT_F4 * 4, 0.0f);
    for (int32_t i = 0; i < num_materials; i++) pack_material(materials[i], c->h_texmap, mats.data() + (size_t)i * MAT_F4 * 4);
    for (size_t k = 0; k < c->h_light_material.size(); k++)
    {
        const ptk_material& m = materials[c->h_light_material[k]];
        float* q = c->h_lights.data() + k * LIGHT_F4 * 4;
        q[7] = m.emissive[0] * m.emissive_intensity; q[11] = m.emissive[1] * m.emissive_intensity; q[12] = m.emissive[2] * m.emissive_intensity;
    }
    // behind everything already queued (stream-ordered): renders in flight keep the old table
    if (!mats.empty()) HIPCHK(c, hipMemcpyAsync(c->d_mats, mats.data(), mats.size() * 4, hipMemcpyHostToDevice, c->stream));
    if (!c->h_lights.empty()) HIPCHK(c, hipMemcpyAsync(c->d_lights, c->h_lights.data(), c->h_lights.size() * 4, hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));          // the host vectors above go out of scope
    c->h_materials.assign(materials, materials + num_materials);
    c->scene_plain = plain_tables((int32_t)c->h_flat_material.size(), c->h_flat_smoothing.data(), c->h_flat_material.data(), num_materials, materials);
    c->scene_lambert = lambert_tables((int32_t)c->h_flat_material.size(), c->h_flat_smoothing.data(), c->h_flat_material.data(), num_materials, materials);
    c->inputs_dirty = true;
    return PTK_OK;
}

int ptk_scene_is_plain(const ptk_scene_desc* s)
{
    if (!s) return 0;
    return plain_tables(s->num_triangles, s->smoothing, s->material, s->num_materials, s->materials) ? 1 : 0;
}

int ptk_scene_is_lambert(const ptk_scene_desc* s)
{
    if (!s) return 0;
    return lambert_tables(s->num_triangles, s->smoothing, s->material, s->num_materials, s->materials) ? 1 : 0;
}

int ptk_flat_zero_class(const float edges[6])
{
    return edges ? ptk_mt::flat_zero_class(edges) : 0;          // the function classify_flat_kernel calls
}

int ptk_flat_zero_mask(int cls)
{
    return cls >= 0 && cls < ptk_mt::FLAT_ZERO_CLASSES ? (int)ptk_mt::flat_zero_mask(cls) : -1;
}

int ptk_flat_classes(ptk_ctx* c, int32_t out[16])
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!c->d_flat_tris) return fail(c, PTK_ERR_BAD_ARG, "the scene has no flat triangle list (more than 16 triangles, or built on the device)");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long word = 0ull;
    HIPCHK(c, hipMemcpyAsync(&word, (const char*)(c->d_flat_tris + FLAT_CLASSES_AT) + 8, sizeof(word), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < FLAT_MAX_TRIS; k++) out[k] = k < c->num_tris ? (int32_t)((word >> (k * 4)) & 15ull) : -1;
    return PTK_OK;
}

int ptk_flat_rect_pair(const float rec_a[9], const float rec_b[9])
{
    return rec_a && rec_b ? ptk_mt::flat_rect_pair(rec_a, rec_b) : 0;          // the function classify_flat_kernel calls
}

int ptk_flat_rect_pairs(ptk_ctx* c, int32_t out[8], int32_t* num_pairs)
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!c->d_flat_tris) return fail(c, PTK_ERR_BAD_ARG, "the scene has no flat triangle list (more than 16 triangles, or built on the device)");
    HIPCHK(c, hipSetDevice(c->device));
    unsigned long long word = 0ull;
    HIPCHK(c, hipMemcpyAsync(&word, (const char*)(c->d_flat_tris + FLAT_PAIRS_AT) + 8, sizeof(word), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (int k = 0; k < FLAT_MAX_TRIS / 2; k++) out[k] = (int32_t)((word >> (k * 4)) & 15ull);
    if (num_pairs) *num_pairs = (int32_t)((word >> 32) & 15ull);
    return PTK_OK;
}

int ptk_trace_variant(ptk_ctx* c, int* variant)
{
    if (!c || !variant) return PTK_ERR_BAD_ARG;
    *variant = c->last_trace_variant;
    return PTK_OK;
}

int ptk_trace_is_lambert(ptk_ctx* c, int* lambert)
{
    if (!c || !lambert) return PTK_ERR_BAD_ARG;
    *lambert = c->last_trace_lambert ? 1 : 0;
    return PTK_OK;
}

int ptk_trace_unit(ptk_ctx* c, int* unit)
{
    if (!c || !unit) return PTK_ERR_BAD_ARG;
    *unit = c->last_trace_unit;
    return PTK_OK;
}

int ptk_set_camera(ptk_ctx* c, const float pos[3], const float dir[3], const float up[3],
                   float focal, float fovy_deg, float focal_dist, float aperture)
{
    if (!c || !pos || !dir || !up) return PTK_ERR_BAD_ARG;
    // the same bound as for scene coordinates (ptk_upload_scene): the kernels' short reciprocal and the implied u > 1 test
    // of the triangle intersection hold while ray origins stay below 2^61
    for (int a = 0; a < 3; a++)
        if (!(std::fabs(pos[a]) < 2.305843e18f)) return fail(c, PTK_ERR_LIMIT, "camera position is not finite or exceeds 2^61");
    for (int a = 0; a < 3; a++) c->cam_pos[a] = pos[a];
    normalize3(dir, c->cam_dir);                           // pathtracer.cpp:336
    normalize3(up, c->cam_up);                             // pathtracer.cpp:337
    c->focal = focal;                                      // SetProjection, pathtracer.cpp:340-350
    if (c->focal <= 0.0f) c->focal = 0.1f;
    c->fovy = fovy_deg;
    if (c->fovy <= 0.0f) c->fovy = 0.1f;
    else if (c->fovy >= 180.0f) c->fovy = 179.5;
    c->focal_dist = focal_dist;
    c->aperture = aperture;
    c->primary_dirty = true;
    return PTK_OK;
}

int ptk_set_frame(ptk_ctx* c, int width, int height, int max_depth)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (width <= 0 || height <= 0 || (int64_t)width * height > (1ll << 28)) return fail(c, PTK_ERR_BAD_ARG, "bad resolution");
    HIPCHK(c, hipSetDevice(c->device));
    c->max_depth = max_depth;
    if (width != c->width || height != c->height || !c->d_accum)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->d_primary.release(); c->d_primary_hit.release(); c->d_primary_rd.release(); c->d_accum.release(); c->d_rgb8.release(); c->d_pixel_rng.release();
        c->pixel_rng_valid = false;
        size_t px = (size_t)width * height;
        HIPCHK(c, hipMalloc(&c->d_primary.p, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_primary_hit.p, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_primary_rd.p, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_pixel_rng.p, px * sizeof(uint2)));
        HIPCHK(c, hipMalloc(&c->d_accum.p, px * 3 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_rgb8.p, px * 3));
        free_adaptive(c);
        free_features(c);
        c->width = width; c->height = height;
        c->d_accum_bound = nullptr;
        unbind_out_image(c, true);               // another resolution: the caller's buffer has another size (main.cpp:3425-3446)
        HIPCHK(c, hipMemsetAsync(c->d_accum, 0, px * 3 * sizeof(float), c->stream));
        HIPCHK(c, hipMemsetAsync(c->d_rgb8, 0, px * 3, c->stream));
        c->samples = 0;
        c->primary_dirty = true;
    }
    return PTK_OK;
}

int ptk_set_tile(ptk_ctx* c, int rank, int world)
{
    if (!c || world < 1 || rank < 0 || rank >= world) return PTK_ERR_BAD_ARG;
    if (rank != c->rank || world != c->world) c->out_full_next = true;      // other tiles: a bound hand-off buffer is rewritten whole
    c->rank = rank; c->world = world;
    return PTK_OK;
}

int ptk_reset(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    size_t px = (size_t)c->width * c->height;
    HIPCHK(c, hipMemsetAsync(accum_ptr(c), 0, px * 3 * sizeof(float), c->stream));     // pathtracer.cpp:745-751
    HIPCHK(c, hipMemsetAsync(c->d_rgb8, 0, px * 3, c->stream));
    c->samples = 0;
    c->adaptive_accum = false;
    if (c->out_host_dev)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memset(c->out_host, 0, px * 3);
    }
    if (c->out_device) HIPCHK(c, hipMemsetAsync(c->out_device, 0, px * 3, c->stream));
    c->out_full_next = true;                     // (a bound OpenGL buffer is rewritten whole by the next render)
    return PTK_OK;
}

int ptk_render(ptk_ctx* c, uint32_t first_sample, uint32_t spp_count, uint64_t seed)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!accum_ptr(c) || !c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    if (c->adaptive_accum)
        return fail(c, PTK_ERR_BAD_ARG, "the accumulator holds an adaptive render (per-pixel sample counts): ptk_reset, ptk_write_accum or a new resolution first");
    HIPCHK(c, hipSetDevice(c->device));
    c->last_launches = 0;
    c->ev.timed = false;
    if (spp_count == 0) return PTK_OK;
    // RenderFrame() begins with mExit = false (pathtracer.cpp:742): an Exit() only cuts the frame(s) in flight, the next
    // call renders again.
    // (an Exit() names the generation of the render it interrupts; this render gets a new one, so nothing needs clearing
    // and consecutive renders stay free to overlap)
    c->render_gen.fetch_add(1);
    int rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;
    rc = run_passes(c, first_sample, spp_count, seed, false, accum_ptr(c), c->d_rgb8, c->d_exit, true);
    if (rc != PTK_OK) return rc;
    c->ev.timed = true;
    c->samples = (int)(first_sample + spp_count);
    return PTK_OK;
}

// Adaptive render: rounds of `step` samples; after each, converge_kernel decides which pixels go on (include/ptk.h).  Every
// round is queued on the context's stream (trace + adaptive accumulate per pass, converge_kernel, live_compact_kernel, a copy
// of the active count to page-locked memory, an event); the host learns that a round left no pixel active ONE ROUND LATE, by
// polling that round's event while the next round is already queued - so the stream never drains between rounds, and at most
// one round is issued that finds the active set empty (it traces, adds and counts nothing).
int ptk_render_adaptive(ptk_ctx* c, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, uint64_t seed,
                        ptk_adaptive_result* out)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (out) std::memset(out, 0, sizeof(*out));
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!accum_ptr(c) || !c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    if (step < 2 || min_spp % step != 0 || max_spp % step != 0 || min_spp > max_spp)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_render_adaptive: need step >= 2 dividing min_spp and max_spp, min_spp <= max_spp");
    if (!std::isfinite(threshold) || threshold < 0.0f) return fail(c, PTK_ERR_BAD_ARG, "ptk_render_adaptive: threshold must be finite and >= 0");
    HIPCHK(c, hipSetDevice(c->device));
    c->last_launches = 0;
    c->ev.timed = false;
    const size_t px = (size_t)c->width * c->height;
    const int tiles_x = (c->width + PTK_TILE - 1) / PTK_TILE;
    const int capacity = tiles_x * ((c->height + PTK_TILE - 1) / PTK_TILE) * 4;
    if (c->adapt_capacity != capacity || !c->d_counts)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_adaptive(c);
        HIPCHK(c, hipMalloc(&c->d_counts.p, px * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc(&c->d_moments.p, px * 3 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_adapt_active.p, (size_t)capacity * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(&c->d_adapt_traced.p, (size_t)capacity * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(&c->d_adapt_list.p, ((size_t)capacity + 1) * sizeof(unsigned)));
        HIPCHK(c, hipMalloc(&c->d_adapt_stats.p, 4 * sizeof(unsigned long long)));
        c->adapt_capacity = capacity;
    }
    if (!c->h_adapt_count)
    {
        HIPCHK(c, c->h_adapt_count.alloc(2));
        for (int b = 0; b < 2; b++) HIPCHK(c, c->ev_adapt[b].create(hipEventDisableTiming));
    }
    // the accumulator starts from zero: ResetImage, plus the counts, S2 and the counters of this render
    int rc = ptk_reset(c);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_counts, 0, px * sizeof(uint32_t), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_moments, 0, px * 3 * sizeof(float), c->stream));
    HIPCHK(c, hipMemsetAsync(c->d_adapt_stats, 0, 4 * sizeof(unsigned long long), c->stream));
    c->adaptive_accum = true;
    c->inputs_dirty = true;
    if (max_spp == 0) return ptk_synchronize(c);
    c->render_gen.fetch_add(1);                  // (one generation for all rounds: an Exit() cuts the whole render)
    const uint32_t gen = c->render_gen.load();
    rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;

    AdaptiveRound ad;
    ad.a.active = c->d_adapt_active; ad.a.counts = c->d_counts; ad.a.moments = c->d_moments; ad.a.stats = c->d_adapt_stats;
    std::memset(&ad.cp, 0, sizeof(ad.cp));
    ad.cp.active = c->d_adapt_active; ad.cp.traced = c->d_adapt_traced; ad.cp.base = c->d_live_mask;
    ad.cp.accum = accum_ptr(c); ad.cp.moments = c->d_moments; ad.cp.counts = c->d_counts;
    ad.cp.active_count = (unsigned*)(c->d_adapt_stats + 2);
    ad.cp.threshold = threshold;
    const uint32_t rounds_max = max_spp / step;
    uint32_t rounds = 0, issued = 0;
    bool converged = false;
    for (uint32_t r = 0; r < rounds_max; r++)
    {
        ad.init = r == 0;
        rc = run_passes(c, r * step, step, seed, false, accum_ptr(c), c->d_rgb8, c->d_exit, false, &ad);
        if (rc != PTK_OK) return rc;
        if (c->last_passes == 0) break;          // (no owned pixel)
        RenderParams p;
        fill_params(c, p, r * step, step, seed);
        p.exit_flag = c->d_exit; p.exit_gen = gen;
        ConvergeParams cp = ad.cp;
        cp.base = c->d_live_mask;
        cp.test = (r + 1) * step >= min_spp ? 1 : 0;
        const int tiles = owned_tiles(p);
        HIPCHK(c, hipMemsetAsync(cp.active_count, 0, sizeof(unsigned), c->stream));
        launch_converge(p, cp, tiles, c->stream);
        HIPCHK(c, hipGetLastError());
        launch_compact_list(c->d_adapt_traced, tiles * 4, c->d_adapt_list, c->d_adapt_list + c->adapt_capacity, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(c->h_adapt_count + (r & 1), cp.active_count, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipEventRecord(c->ev_adapt[r & 1], c->stream));
        c->last_launches += 2;
        issued = r + 1;
        rounds = issued;
        if (r >= 1)
        {
            // round r is queued: now wait for round r - 1's count (polled for a while, then the runtime's blocking wait)
            const auto t0 = std::chrono::steady_clock::now();
            hipError_t q;
            while ((q = hipEventQuery(c->ev_adapt[(r - 1) & 1])) == hipErrorNotReady &&
                   std::chrono::steady_clock::now() - t0 < std::chrono::milliseconds(2)) {}
            if (q == hipErrorNotReady) q = hipEventSynchronize(c->ev_adapt[(r - 1) & 1]);
            if (q != hipSuccess) return fail(c, PTK_ERR_HIP, std::string("hipEventSynchronize: ") + hipGetErrorString(q));
            if (c->h_adapt_count[(r - 1) & 1] == 0u) { converged = true; rounds = r; break; }     // round r found nothing to do
        }
        if (__atomic_load_n(c->h_exit.p, __ATOMIC_RELAXED) >= gen) break;                        // Exit(): the rest stands down anyway
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long st[3] = { 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(st, c->d_adapt_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t active = 0;
    const bool cut = __atomic_load_n(c->h_exit.p, __ATOMIC_RELAXED) >= gen;
    if (cut)
    {
        // the kernels that stood down left the active set as it was: count it
        const int tiles = (int)((capacity / 4 <= c->rank) ? 0 : (capacity / 4 - c->rank + c->world - 1) / c->world);
        std::vector<unsigned long long> m((size_t)tiles * 4);
        if (!m.empty())
        {
            HIPCHK(c, hipMemcpyAsync(m.data(), c->d_adapt_active, m.size() * sizeof(unsigned long long), hipMemcpyDeviceToHost, c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
        }
        for (unsigned long long w : m) active += (uint64_t)__builtin_popcountll(w);
    }
    else if (!converged && issued > 0) active = c->h_adapt_count[(issued - 1) & 1];
    c->samples = (int)st[1];
    if (out)
    {
        out->rounds = rounds; out->max_count = (uint32_t)st[1];
        out->pixel_samples = st[0]; out->active_pixels = active;
    }
    return PTK_OK;
}

// ---- first-hit feature planes (ptk.h) ------------------------------------------------------------------------------------
int ptk_feature_info(int feature, int* channels, int* is_int)
{
    if (feature < 0 || feature >= NUM_FEATURES) return PTK_ERR_BAD_ARG;
    if (channels) *channels = kFeatChannels[feature];
    if (is_int) *is_int = kFeatIsInt[feature];
    return PTK_OK;
}

int ptk_render_features(ptk_ctx* c, uint32_t sample, uint64_t seed, uint32_t mask)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (mask >> NUM_FEATURES) return fail(c, PTK_ERR_BAD_ARG, "unknown feature bit in the mask");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;
    RenderParams p;
    fill_params(c, p, sample, 1, seed);
    // the cache is brought up to date exactly as a render does it (run_passes), and taken in place of the walk where it is valid
    if (rc = use_primary_cache(c, p); rc != PTK_OK) return rc;
    const size_t px = (size_t)c->width * c->height;
    c->feat_mask = 0;
    for (int k = 0; k < NUM_FEATURES; k++)
        if (((mask >> k) & 1u) && !c->d_feat[k]) HIPCHK(c, hipMalloc(&c->d_feat[k].p, px * kFeatChannels[k] * 4));
    c->feat_w = c->width; c->feat_h = c->height;
    FeatureParams f = {};
    void** slot[NUM_FEATURES] = { (void**)&f.depth, (void**)&f.triangle, (void**)&f.material, (void**)&f.bary, (void**)&f.position,
                                  (void**)&f.normal_geom, (void**)&f.normal, (void**)&f.albedo, (void**)&f.emission, (void**)&f.gloss };
    for (int k = 0; k < NUM_FEATURES; k++)
    {
        if (!((mask >> k) & 1u)) continue;
        *slot[k] = c->d_feat[k];
        // a tile split writes the owned pixels only: the others hold the miss values (+inf, -1, 0)
        if (c->world > 1)
            HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)c->d_feat[k], k == 0 ? 0x7f800000 : (kFeatIsInt[k] ? -1 : 0), px * kFeatChannels[k], c->stream));
    }
    f.sample = sample; f.seed_lo = (uint32_t)seed; f.seed_hi = (uint32_t)(seed >> 32);
    if (mask) launch_features(p, f, owned_tiles(p), c->stream);
    HIPCHK(c, hipGetLastError());
    c->feat_mask = mask;
    return PTK_OK;
}

int ptk_read_feature(ptk_ctx* c, int feature, void* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    size_t bytes = 0;
    void* d = feature_plane(c, feature, &bytes);
    if (!d) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_feature_device_ptr(ptk_ctx* c, int feature, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    size_t b = 0;
    void* d = feature_plane(c, feature, &b);
    if (!d) return PTK_ERR_BAD_ARG;
    *dev_ptr = d;
    if (bytes) *bytes = b;
    return PTK_OK;
}

int ptk_pick(ptk_ctx* c, int x, int y_top_down, uint64_t seed, int32_t* tri, int32_t* material, float* t)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (x < 0 || y_top_down < 0 || x >= c->width || y_top_down >= c->height) return fail(c, PTK_ERR_BAD_ARG, "ptk_pick: pixel outside the frame");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;
    int32_t out[3] = { -1, -1, 0 };              // one ray: [0] the triangle, [1] its material index, [2] the bits of t
    Stage s(c);
    const auto d_out = s.out(out, 3);
    rc = s.run([&] {
        RenderParams p; FeatureParams f = {};
        fill_params(c, p, 0, 1, seed);
        f.sample = 0; f.seed_lo = (uint32_t)seed; f.seed_hi = (uint32_t)(seed >> 32);
        launch_pick(p, f, y_top_down * c->width + x, d_out, c->stream);
        return s.launched();
    });
    if (rc != PTK_OK) return rc;
    float th; std::memcpy(&th, &out[2], 4);
    if (tri) *tri = out[0];
    if (material) *material = out[1];
    if (t) *t = th;
    return PTK_OK;
}

int ptk_read_sample_counts(ptk_ctx* c, uint32_t* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->width * c->height;
    if (!c->d_counts || !c->adaptive_accum)
    {
        // no adaptive render in the accumulator: every owned pixel holds ptk_samples samples
        HIPCHK(c, hipStreamSynchronize(c->stream));
        std::memset(host_out, 0, px * sizeof(uint32_t));
        const int tiles_x = (c->width + PTK_TILE - 1) / PTK_TILE, tiles_y = (c->height + PTK_TILE - 1) / PTK_TILE;
        const uint32_t n = (uint32_t)c->samples.load();
        for (int tile = c->rank; tile < tiles_x * tiles_y; tile += c->world)
        {
            int tx, ty; tile_origin(tile, tiles_x, tx, ty);
            for (int y = ty * PTK_TILE; y < std::min(c->height, (ty + 1) * PTK_TILE); y++)
                for (int x = tx * PTK_TILE; x < std::min(c->width, (tx + 1) * PTK_TILE); x++)
                    host_out[(size_t)(c->height - 1 - y) * c->width + x] = n;
        }
        return PTK_OK;
    }
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_counts, px * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_read_moments(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_moments || !c->adaptive_accum) return fail(c, PTK_ERR_BAD_ARG, "ptk_read_moments: the accumulator holds no adaptive render");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_moments, (size_t)c->width * c->height * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_collect_stats(ptk_ctx* c, uint32_t first_sample, uint32_t spp_count, uint64_t seed, ptk_stats* out)
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    if (!c->have_scene || !c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "scene / frame not set");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;
    // untimed counters-enabled variant; renders into a scratch accumulator so the image is untouched
    size_t px = (size_t)c->width * c->height;
    Buf<float> scratch; Buf<uint8_t> scratch8;   // (freed on the way out, behind the wait for the stream)
    if (rc = scratch.alloc(c, px * 3); rc != PTK_OK) return rc;
    if (rc = scratch8.alloc(c, px * 3); rc != PTK_OK) return rc;
    (void)hipMemsetAsync(scratch, 0, px * 3 * sizeof(float), c->stream);
    (void)hipMemsetAsync(c->d_stats, 0, 16 * sizeof(unsigned long long), c->stream);
    c->inputs_dirty = true;                      // ... and the zeroed counters
    rc = run_passes(c, first_sample, spp_count, seed, true, scratch, scratch8, nullptr, false);
    c->ev.timed = false;
    unsigned long long h[16] = { 0 };
    hipError_t e = hipMemcpyAsync(h, c->d_stats, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    out->samples = owned_pixels(c) * (unsigned long long)spp_count; out->rays = h[1]; out->shadow_rays = h[2]; out->node_visits = h[3];
    out->tri_tests = h[4]; out->hits_shaded = h[5]; out->tex_fetches = h[6];
    out->walk_wave_iters = h[7]; out->walk_lane_iters = h[8]; out->shade_wave_execs = h[9]; out->shade_lanes = h[10];
    out->gen_wave_execs = h[11]; out->gen_lanes = h[12];
    out->tri_wave_execs = h[13]; out->tri_lanes = h[14];
    out->max_walk_nodes = h[15]; out->paths_started = h[0];
    return PTK_OK;
}

int ptk_bind_out_image(ptk_ctx* c, uint8_t* host_out)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    // (the same buffer again: nothing to do - unless this context page-locked it, see below: a block freed and allocated again at
    // the same address has other pages behind it than the ones that were locked)
    if (host_out == c->out_host && !c->out_registered && !c->out_device && !c->gl_res) return PTK_OK;
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));      // nothing may still be writing into the old buffer
    unbind_out_image(c);
    if (!host_out) return PTK_OK;
    if (c->width <= 0 || !c->d_rgb8) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    // Zero-copy needs memory the GPU can write.  A buffer that already IS such memory - ptk_host_alloc, or anything the caller
    // page-locked and mapped itself - is used as it stands.  FOREIGN pageable memory (the viewer's `new GLubyte[w * h * 3]`,
    // main.cpp:3435) is left alone by default: the reference's caller deletes texData BEFORE it hands over the next buffer
    // (InitializeFrame, main.cpp:3433-3445) and at exit without a word to the tracer (OnExit, :3622), and memory freed while
    // still registered with the runtime poisons what the allocator puts there next (tools/soak_api.py, round 3).
    // Such a buffer is simply not bound: ptk_resolve_rgb8 copies the frame into it, which is always correct.
    // ptk_set_option("register_out_image", 1) opts in to page-locking it in place (hipHostRegister) for callers that promise
    // to unbind - ptk_bind_out_image(ctx, NULL) - BEFORE they free it.
    void* dev = nullptr;
    if (hipHostGetDevicePointer(&dev, host_out, 0) == hipSuccess && dev) c->out_host_dev = (uint8_t*)dev;       // ptk_host_alloc / already page-locked
    else
    {
        (void)hipGetLastError();
        if (c->opt_register_out)
        {
            const size_t bytes = (size_t)c->width * c->height * 3;
            if (hipHostRegister(host_out, bytes, hipHostRegisterMapped) == hipSuccess)
            {
                if (hipHostGetDevicePointer(&dev, host_out, 0) == hipSuccess && dev) { c->out_host_dev = (uint8_t*)dev; c->out_registered = true; }
                else (void)hipHostUnregister(host_out);
            }
            (void)hipGetLastError();             // not lockable: ptk_resolve_rgb8 keeps copying
        }
    }
    if (!c->out_host_dev) return PTK_OK;         // not bound (see above)
    c->out_host = host_out;
    std::memset(host_out, 0, (size_t)c->width * c->height * 3);     // pixels that are black for every sample are written once at most
    c->out_full_next = true;
    return PTK_OK;
}

// The interactive loop waits for frames of a few hundred microseconds: poll the stream for a while before handing the wait to
// the runtime, whose blocking wait costs tens of microseconds to wake up.
static int wait_polled(ptk_ctx* c)
{
    const auto t0 = std::chrono::steady_clock::now();
    for (;;)
    {
        const hipError_t q = hipStreamQuery(c->stream);
        if (q == hipSuccess) return PTK_OK;
        if (q != hipErrorNotReady) return fail(c, PTK_ERR_HIP, std::string("hipStreamQuery: ") + hipGetErrorString(q));
        if (std::chrono::steady_clock::now() - t0 > std::chrono::milliseconds(2)) break;
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_bind_out_device(ptk_ctx* c, void* device_rgb8)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (device_rgb8 && device_rgb8 == c->out_device) return PTK_OK;
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    unbind_out_image(c);
    if (!device_rgb8) return PTK_OK;
    if (c->width <= 0 || !c->d_rgb8) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    hipPointerAttribute_t attr;
    if (hipPointerGetAttributes(&attr, device_rgb8) != hipSuccess || attr.type != hipMemoryTypeDevice || attr.device != c->device)
    {
        (void)hipGetLastError();
        return fail(c, PTK_ERR_BAD_ARG, "ptk_bind_out_device: not a device allocation of this context's GPU");
    }
    c->out_device = (uint8_t*)device_rgb8;
    HIPCHK(c, hipMemsetAsync(c->out_device, 0, (size_t)c->width * c->height * 3, c->stream));
    c->out_full_next = true;
    return PTK_OK;
}

int ptk_bind_gl_buffer(ptk_ctx* c, unsigned int gl_buffer)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (gl_buffer != 0 && gl_buffer == c->gl_buffer && c->gl_res) return PTK_OK;
    if (c->stream) HIPCHK(c, hipStreamSynchronize(c->stream));
    unbind_out_image(c);
    if (gl_buffer == 0) return PTK_OK;
    // (no frame needed yet: the buffer's size is checked against the frame each time it is mapped, run_passes)
    // Registration talks to the OpenGL driver through the calling thread's CURRENT context (the viewer's: main.cpp creates it
    // before the path tracer renders anything).  The library does not link OpenGL: the process that calls this has it loaded,
    // and a process without a current context gets an error here instead of a crash inside the runtime.
    typedef void* (*current_ctx_fn)(void);
    bool have_ctx = false;
    for (const char* name : { "glXGetCurrentContext", "eglGetCurrentContext", "wglGetCurrentContext" })
    {
        current_ctx_fn fn = (current_ctx_fn)dlsym(RTLD_DEFAULT, name);
        if (fn && fn() != nullptr) { have_ctx = true; break; }
    }
    if (!have_ctx) return fail(c, PTK_ERR_BAD_ARG, "ptk_bind_gl_buffer: no OpenGL context is current on the calling thread");
    hipGraphicsResource_t res = nullptr;
    const hipError_t e = hipGraphicsGLRegisterBuffer(&res, gl_buffer, hipGraphicsRegisterFlagsNone);
    if (e != hipSuccess || !res)
    {
        (void)hipGetLastError();
        return fail(c, PTK_ERR_HIP, std::string("hipGraphicsGLRegisterBuffer: ") + hipGetErrorString(e));
    }
    c->gl_res = res; c->gl_buffer = gl_buffer;
    c->out_full_next = true;
    return PTK_OK;
}

int ptk_resolve_rgb8(ptk_ctx* c, uint8_t* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_rgb8) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    if (host_out == c->out_host && c->out_host_dev && !c->out_full_next)
    {
        // bound: the accumulate kernel of the last render has written the frame there (out_full_next is only set while no
        // render has filled the buffer since it was bound / reset).  The interactive loop waits for a frame of a few hundred
        // microseconds: poll the stream for a while before handing the wait to the runtime, whose blocking wait costs
        // tens of microseconds to wake up
        return wait_polled(c);
    }
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_rgb8, (size_t)c->width * c->height * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

void* ptk_host_alloc(size_t bytes)
{
    void* p = nullptr;
    if (bytes == 0 || hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess) return nullptr;
    return p;
}
void ptk_host_free(void* p) { if (p) (void)hipHostFree(p); }

int ptk_read_accum(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, accum_ptr(c), (size_t)c->width * c->height * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_write_accum(ptk_ctx* c, const float* host_in, int samples)
{
    if (!c || !host_in || samples < 0) return PTK_ERR_BAD_ARG;
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(accum_ptr(c), host_in, (size_t)c->width * c->height * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    c->samples = samples;
    c->adaptive_accum = false;
    c->out_full_next = true;
    return PTK_OK;
}

int ptk_samples(ptk_ctx* c) { return c ? c->samples.load() : 0; }

int ptk_request_exit(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    // blocks that have not started yet read the flag and return (kernel prologue).  Written by an asynchronous copy on a
    // stream of its own, so it lands while renders are in flight: a blocking hipMemcpy may be held back by the runtime until
    // the queued renders have run to their end (it then cut nothing).  Generations only grow, so a copy that reads a later
    // store of the source word still names every render it was meant to cut.
    std::lock_guard<std::mutex> lk(c->exit_mu);
    uint32_t gen = c->render_gen.load();
    c->out_full_next = true;                     // a cut render may have skipped a full write of the bound hand-off buffer
    if (gen > __atomic_load_n(c->h_exit.p, __ATOMIC_RELAXED)) __atomic_store_n(c->h_exit.p, gen, __ATOMIC_RELAXED);
    (void)hipSetDevice(c->device);
    (void)hipMemcpyAsync(c->d_exit, c->h_exit, sizeof(uint32_t), hipMemcpyHostToDevice, c->exit_stream);
    return PTK_OK;
}

int ptk_synchronize(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->out_device || c->gl_res) return wait_polled(c);     // a frame of the interactive loop (device-resident hand-off)
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_accum_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    *dev_ptr = accum_ptr(c);
    if (bytes) *bytes = (size_t)c->width * c->height * 3 * sizeof(float);
    return *dev_ptr ? PTK_OK : fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
}

int ptk_rgb8_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    *dev_ptr = c->d_rgb8;
    if (bytes) *bytes = (size_t)c->width * c->height * 3;
    return *dev_ptr ? PTK_OK : fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
}

int ptk_bind_accum(ptk_ctx* c, void* dev_ptr)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->d_accum) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if ((float*)dev_ptr != c->d_accum_bound) c->out_full_next = true;       // another accumulator: pixels that were skipped as "always black" may hold light there
    c->d_accum_bound = (float*)dev_ptr;
    return PTK_OK;
}

int ptk_last_render_ms(ptk_ctx* c, float* ms, int* launches)
{
    if (!c || !ms) return PTK_ERR_BAD_ARG;
    float t = 0.0f, a = 0.0f;
    int rc = ptk_last_kernel_ms(c, &t, &a);
    *ms = t + a;
    if (launches) *launches = c->last_launches;
    return rc;
}

int ptk_kernel_log(ptk_ctx* c, int capacity)
{
    if (!c || capacity < 0 || capacity > (1 << 20)) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipDeviceSynchronize());
    c->klog_ev.clear(); c->klog_n = 0;
    for (int i = 0; i < 2 * capacity; i++) { Event e; HIPCHK(c, e.create()); c->klog_ev.push_back(std::move(e)); }
    return PTK_OK;
}

int ptk_kernel_log_read(ptk_ctx* c, float* trace_ms, int max_entries, int* num_entries)
{
    if (!c || !num_entries || (max_entries > 0 && !trace_ms)) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < 2; k++) if (c->trace_stream[k]) HIPCHK(c, hipStreamSynchronize(c->trace_stream[k]));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = std::min(c->klog_n, max_entries);
    for (int i = 0; i < n; i++)
        if (const int rc = event_ms(c, c->klog_ev[2 * i], c->klog_ev[2 * i + 1], &trace_ms[i]); rc != PTK_OK) return rc;
    *num_entries = n;
    c->klog_n = 0;
    return PTK_OK;
}

int ptk_last_kernel_ms(ptk_ctx* c, float* trace_ms, float* accumulate_ms)
{
    if (!c || !trace_ms || !accumulate_ms) return PTK_ERR_BAD_ARG;
    *trace_ms = 0.0f; *accumulate_ms = 0.0f;
    if (!c->ev.timed) return PTK_OK;
    const int n = std::min(c->last_passes, (int)ptk_ctx::kMaxTimedPasses);
    for (int i = 0; i < n; i++)
        if (const int rc = c->ev.add(c, i, trace_ms, accumulate_ms); rc != PTK_OK) return rc;
    return PTK_OK;
}

int ptk_set_option(ptk_ctx* c, const char* name, double value)
{
    if (!c || !name) return PTK_ERR_BAD_ARG;
    if (!std::strcmp(name, "chunk"))
    {
        if (!(value >= 0 && value <= 4096)) return fail(c, PTK_ERR_BAD_ARG, "chunk must be in [0, 4096] (0 = automatic)");
        c->opt_chunk = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "shade_threshold") || !std::strcmp(name, "gen_threshold"))
    {
        if (!(value >= 0 && value <= 4096)) return fail(c, PTK_ERR_BAD_ARG, "threshold (lambda in eighths) must be in [0, 4096]");
        (name[0] == 's' ? c->opt_shade_thr : c->opt_gen_thr) = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "overlap"))
    {
        c->opt_overlap = value != 0.0 ? 1 : 0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "comm_timeout_s"))
    {
        // bound of every wait of the exchange step (ptk_comm_init, ptk_gather_wait, ptk_read_gathered)
        if (!(value >= 0.05 && value <= 86400.0)) return fail(c, PTK_ERR_BAD_ARG, "comm_timeout_s must be in [0.05, 86400]");
        c->opt_comm_timeout_s = value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "lens_cull"))
    {
        // 0: uncached cameras trace every pixel of the frame (the cull is exact: same image either way; tests / A-B only)
        c->opt_lens_cull = value != 0.0 ? 1 : 0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "register_out_image"))
    {
        // 1: ptk_bind_out_image page-locks a pageable caller buffer in place (zero-copy hand-off; the caller unbinds before freeing it)
        c->opt_register_out = value != 0.0 ? 1 : 0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "bvh_leaf_max") || !std::strcmp(name, "bvh_trav_cost") || !std::strcmp(name, "bvh_verbose"))
    {
        // builder tuning (process-wide, takes effect at the next ptk_upload_scene; 0 = the builders' own choices)
        if (!(value >= 0 && value <= 64)) return fail(c, PTK_ERR_BAD_ARG, "builder tuning value must be in [0, 64]");
        if (name[4] == 'l') g_bvh_tuning.leaf_max = (int)value; else if (name[4] == 't') g_bvh_tuning.trav_cost = (float)value; else g_bvh_tuning.verbose = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "contract"))
    {
        if (!(value == 0.0 || value == 1.0 || value == 2.0)) return fail(c, PTK_ERR_BAD_ARG, "contract must be 0 (bit-exact), 1 (fused multiply-adds) or 2 (... and 1-ulp reciprocal / square root)");
        c->opt_contract = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "generations"))
    {
        if (!(value >= 0 && value <= 64)) return fail(c, PTK_ERR_BAD_ARG, "generations must be in [0, 64] (0 = automatic)");
        c->opt_generations = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "persistent"))
    {
        if (!(value >= -1 && value <= 1)) return fail(c, PTK_ERR_BAD_ARG, "persistent must be -1 (automatic), 0 or 1");
        c->opt_persistent = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "max_batch"))
    {
        if (!(value >= 1 && value <= 64)) return fail(c, PTK_ERR_BAD_ARG, "max_batch must be in [1, 64]");
        c->opt_max_batch = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "tri_threshold"))
    {
        if (!(value >= 0 && value <= 4096)) return fail(c, PTK_ERR_BAD_ARG, "tri_threshold (eighths) must be in [0, 4096]");
        c->opt_tri_thr = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "flat_shade_weight") || !std::strcmp(name, "flat_gen_weight"))
    {
        if (!(value >= 1 && value <= 4096)) return fail(c, PTK_ERR_BAD_ARG, "weight (eighths) must be in [1, 4096]");
        (name[5] == 's' ? c->opt_flat_shade_w : c->opt_flat_gen_w) = (int)value;
        return PTK_OK;
    }
    if (!std::strcmp(name, "flat"))
    {
        c->opt_flat = value != 0.0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "plain_kernel"))
    {
        c->opt_plain_kernel = value != 0.0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "lambert_kernel"))
    {
        c->opt_lambert_kernel = value != 0.0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "flat_zero_classes"))
    {
        const int use = value != 0.0 ? 1 : 0;
        if (use != c->opt_flat_zero_classes && c->have_scene && c->d_flat_tris)
        {
            // the word the pass reads is rewritten behind every render already queued and ahead of every later one, like a geometry update
            HIPCHK(c, hipSetDevice(c->device));
            launch_flat_classes(c->d_flat_tris, c->num_tris, use, c->opt_flat_rect_pairs, c->stream);
            HIPCHK(c, hipGetLastError());
            c->inputs_dirty = true;
        }
        c->opt_flat_zero_classes = use;
        return PTK_OK;
    }
    if (!std::strcmp(name, "flat_rect_pairs"))
    {
        const int use = value != 0.0 ? 1 : 0;
        if (use != c->opt_flat_rect_pairs && c->have_scene && c->d_flat_tris)
        {
            // (the word the pair pass reads, rewritten stream-ordered like the class word above)
            HIPCHK(c, hipSetDevice(c->device));
            launch_flat_classes(c->d_flat_tris, c->num_tris, c->opt_flat_zero_classes, use, c->stream);
            HIPCHK(c, hipGetLastError());
            c->inputs_dirty = true;
        }
        c->opt_flat_rect_pairs = use;
        return PTK_OK;
    }
    if (!std::strcmp(name, "surface_variant"))
    {
        c->opt_surface_variant = value != 0.0 ? 1 : 0;          // (which instantiation the next ptk_sample_surface launches: nothing on the device changes)
        return PTK_OK;
    }
    if (!std::strcmp(name, "flat_cycle"))
    {
        c->opt_flat_cycle = value != 0.0 ? 1 : 0;         // (which kernel the next render launches: nothing on the device changes)
        return PTK_OK;
    }
    if (!std::strcmp(name, "device_build"))
    {
        c->opt_device_build = value != 0.0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "primary_cache"))
    {
        c->opt_primary_cache = value != 0.0;
        return PTK_OK;
    }
    if (!std::strcmp(name, "pass_bytes"))
    {
        // upper bound: the kernel indexes the sample buffer (16-byte entries) with 32 bits
        if (!(value >= 1 << 20 && value <= 32.0 * 1073741824.0)) return fail(c, PTK_ERR_BAD_ARG, "pass_bytes must be in [1 MiB, 32 GiB]");
        c->opt_pass_bytes = (size_t)value;
        return PTK_OK;
    }
    return fail(c, PTK_ERR_BAD_ARG, std::string("unknown option ") + name);
}

int ptk_bvh_info(ptk_ctx* c, int32_t* num_nodes, int32_t* depth, int32_t* num_leaf_tris)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (num_nodes) *num_nodes = c->num_nodes;
    if (depth) *depth = c->bvh_depth;
    if (num_leaf_tris) *num_leaf_tris = c->num_leaf_tris;
    return PTK_OK;
}

int ptk_upload_timing(ptk_ctx* c, double* ms4, int* built_on_device)
{
    if (!c || !ms4) return PTK_ERR_BAD_ARG;
    for (int k = 0; k < 4; k++) ms4[k] = c->upload_ms[k];
    if (built_on_device) *built_on_device = c->built_on_device ? 1 : 0;
    return PTK_OK;
}

int ptk_bvh_layout(ptk_ctx* c, int32_t* node_width, int32_t* node_bytes, int32_t* stack_need)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (node_width) *node_width = 4;
    if (node_bytes) *node_bytes = NODE_F4 * 16;
    if (stack_need) *stack_need = c->bvh_stack;
    return PTK_OK;
}

int ptk_download_bvh(ptk_ctx* c, float* nodes16, int32_t* leaf_order)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (nodes16 && c->num_nodes > 0) HIPCHK(c, hipMemcpy(nodes16, c->d_nodes, (size_t)c->num_nodes * NODE_F4 * sizeof(float4), hipMemcpyDeviceToHost));
    if (leaf_order && c->num_tris > 0)
    {
        std::vector<float> t((size_t)c->num_tris * TRI_F4 * 4);
        HIPCHK(c, hipMemcpy(t.data(), c->d_tris, t.size() * sizeof(float), hipMemcpyDeviceToHost));
        for (int32_t k = 0; k < c->num_tris; k++) std::memcpy(&leaf_order[k], &t[(size_t)k * TRI_F4 * 4 + 9], 4);
    }
    return PTK_OK;
}

}  // extern "C"
