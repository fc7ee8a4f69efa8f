// Host side of the ptk C-ABI (include/ptk.h): context, scene staging into the device record layouts
// of ptk_device.h, BVH build, kernel launches, hand-off copies, RCCL exchange step.
//
// Reference behaviour restated here (PathTracing/src/pathtracer.cpp): BuildBVH + light list :260-274,
// setters :297-360, frame set-up arithmetic of RenderFrame :755-766, reset :745-751.
#include <hip/hip_runtime.h>
#include <hip/hip_gl_interop.h>
#include <rccl/rccl.h>
#include <dlfcn.h>

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <memory>
#include <string>
#include <thread>
#include <vector>

#include "bvh_build.h"
#include "bvh_device.h"
#include "ptk_device_fn.h"
#include "ptk_adaptive.h"
#include "ptk_features.h"
#include "ptk_rays.h"
#include "ptk_bake.h"
#include "ptk_probes.h"
#include "ptk_rays_adaptive.h"
#include "ptk_hits.h"
#include "ptk_refit.h"

using namespace ptk;

struct ptk_ctx {
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string error;
    std::mutex err_mu;

    // scene (device)
    float4* d_flat_tris = nullptr;      // <= 16 triangles: records in ascending triangle index for the FLAT kernel
    float4 *d_nodes = nullptr, *d_tris = nullptr, *d_shade = nullptr, *d_mats = nullptr, *d_lights = nullptr;
    int4* d_texinfo = nullptr;
    uint32_t* d_texels = nullptr;
    int num_nodes = 0, num_tris = 0, num_lights = 0, bvh_depth = 0, bvh_stack = 0, num_leaf_tris = 0;
    float scene_bound = 0.0f;           // 3.1 x (1.01 x the largest |vertex coordinate| + 1e-3): RenderParams::scene_bound
    float scene_lo[3] = { 0, 0, 0 }, scene_hi[3] = { 0, 0, 0 };     // the vertices' bounding box
    int opt_lens_cull = 1;              // uncached cameras: pixels whose whole bundle of lens rays misses that box are never traced
    unsigned long long view_generation = 0;      // bumped whenever camera, frame or scene change what an uncached pixel can see
    bool have_scene = false;
    double upload_ms[4] = { 0, 0, 0, 0 };       // last ptk_upload_scene: BVH build, record packing, device copies, total
    // host copies kept for ptk_update_materials: what was uploaded, the texture index map, the light records
    std::vector<ptk_material> h_materials;
    std::vector<int32_t> h_texmap, h_light_material;
    std::vector<float> h_lights;
    // FLAT scenes: each triangle's smoothing flag and material, for re-deciding scene_plain when the materials are edited
    std::vector<uint8_t> h_flat_smoothing;
    std::vector<int32_t> h_flat_material;
    // geometry updates (ptk_update_geometry): the world-space vertices stay resident beside the records (a refit needs the exact
    // v2, v3: fl(v1 + fl(v2 - v1)) is not v2); everything else is made by the first update and lives until the next upload
    float* d_verts_res = nullptr;                // [num_tris][9]
    int32_t* d_tri_pos = nullptr;                // triangle -> position of its record in the leaf order
    int32_t* d_level_nodes = nullptr;            // node indices sorted by level, the root's level first
    std::vector<int> level_start;                // [levels + 1] offsets into d_level_nodes
    double* d_refit_partial = nullptr;           // one partial SAH sum per 256 nodes
    float4* d_refit_side = nullptr;              // per node: union box + summed child half-area (ptk_refit.h)
    float* d_geo_stage = nullptr; size_t geo_stage_floats = 0;     // staged verts | normals | tbn of the update in progress
    uint32_t* d_geo_red = nullptr;               // GEO_RED_WORDS of the bounds reduction, then one double: the SAH cost
    uint32_t* h_geo_red = nullptr;               // page-locked target of its read-back
    hipStream_t geo_stream = nullptr;            // staging copies and the bounds reduction: the one host wait of an update is for this stream alone
    // events of the newest update: [0] [1] around staging + bounds on geo_stream; [2] before the repack, [3] behind it, [4] behind
    // the refit on the context's stream ([4] also orders the next update's staging behind this one's kernels)
    hipEvent_t ev_geo_t[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    bool geo_done_recorded = false, lights_stale = false;          // lights_stale: h_lights lacks the vertices an update moved
    uint32_t geo_updates = 0;
    double sah_built = 0.0, sah_now = 0.0; bool sah_now_pending = false;
    float bvh_pad = 0.0f;                        // the builders' box padding for the current scene extent
    bool scene_plain = false;           // plain_tables() of the staged scene: kept current by ptk_upload_scene and ptk_update_materials
    int opt_plain_kernel = 1;           // 0: plain scenes launch the generic FLAT kernel too (tests, A/B runs)
    int last_trace_variant = PTK_TRACE_NONE;     // of the newest trace launch (ptk_trace_variant)

    // camera (host copies, already normalised / clamped like the reference setters)
    float cam_pos[3] = { 0, 0, 0 }, cam_dir[3] = { 0, 0, 1 }, cam_up[3] = { 0, 1, 0 };
    float focal = 0.1f, fovy = 90.0f, focal_dist = 5.0f, aperture = 0.0f;   // pathtracer.cpp:17-22
    float cam_right[3] = { 1, 0, 0 };
    bool primary_dirty = true;

    // frame
    int width = 0, height = 0, max_depth = 3;                                 // pathtracer.cpp:15
    float4* d_primary = nullptr;
    float4* d_primary_hit = nullptr;  // primary-visibility cache (pinhole, no opacity textures)
    float4* d_primary_rd = nullptr;   // ... and the camera ray's direction per pixel
    uint2* d_pixel_rng = nullptr;     // per pixel: (pixel key, PCG increment) for pixel_rng_seed
    uint64_t pixel_rng_seed = 0; bool pixel_rng_valid = false;
    bool primary_hit_dirty = true, scene_has_opacity = false;
    int opt_primary_cache = 1;
    int opt_flat_shade_w = 8, opt_flat_gen_w = 64;
    int opt_flat = 1;                    // scenes of <= PTK_FLAT_MAX triangles: no BVH walk (trace_kernel<.., FLAT>)
    float* d_accum = nullptr;        // owned accumulator
    float* d_accum_bound = nullptr;  // caller-owned accumulator (ptk_bind_accum) or null
    uint8_t* d_rgb8 = nullptr;
    // hand-off buffer bound by ptk_bind_out_image: the caller's pointer, its device-visible alias, whether this context
    // page-locked it, and whether the next accumulate kernel must write every pixel (after binding, reset, a camera or
    // scene change: the set of always-black pixels may have changed)
    uint8_t* out_host = nullptr; uint8_t* out_host_dev = nullptr;
    bool out_registered = false;
    std::atomic<bool> out_full_next{ true };
    // ... or a DEVICE buffer bound by ptk_bind_out_device, or an OpenGL buffer object registered by ptk_bind_gl_buffer (mapped
    // for the length of each render: run_passes)
    uint8_t* out_device = nullptr;
    hipGraphicsResource_t gl_res = nullptr;
    unsigned gl_buffer = 0;
    int rank = 0, world = 1;

    std::atomic<int> samples{ 0 };
    std::atomic<uint32_t> render_gen{ 1 };       // generation of the newest render: Exit() names it and thereby every render still in flight (kernels stand down
                                                 // when the named generation >= their own); renders issued afterwards are not affected
    uint32_t* d_exit = nullptr;
    uint32_t* h_exit = nullptr;                  // page-locked source of the copy that writes d_exit (ptk_request_exit)
    hipStream_t exit_stream = nullptr;           // high priority, nothing else on it: the copy of the Exit() word never waits behind a render
    std::mutex exit_mu;                          // (Exit() may come from several threads: the source word never goes back)
    unsigned long long* d_stats = nullptr;
    unsigned* d_queues = nullptr;                // item queues of trace_kernel's persistent waves
    // live-quadrant list (which 8x8 quadrants of the owned tiles have pixels to trace) and what it was built for
    unsigned long long* d_live_mask = nullptr;
    unsigned* d_live_list = nullptr;             // [capacity] entries + 1 word: the count
    int live_capacity = 0;
    unsigned long long hit_generation = 0;       // bumped whenever the primary-hit cache is recomputed
    struct LiveKey { int width, height, rank, world, cached; unsigned long long generation; } live_key = { 0, 0, -1, 0, -1, 0 };
    int resident_waves = 4096;                   // one-wave workgroups the device holds at once (CUs x 16)

    // adaptive render (ptk_render_adaptive): allocated by the first one, freed by ptk_set_frame with another resolution
    uint32_t* d_counts = nullptr;                // [H][W] samples per pixel, rows bottom-up
    float* d_moments = nullptr;                  // [H][W][3] sums of squared samples (S2)
    unsigned long long* d_adapt_active = nullptr, * d_adapt_traced = nullptr;     // per quadrant of the frame: active set, active & live
    unsigned* d_adapt_list = nullptr;            // [adapt_capacity] entries + 1 word: the count (the traced mask's quadrants)
    unsigned long long* d_adapt_stats = nullptr; // [0] pixel samples, [1] largest count, [2] low word: active pixels after the last test
    int adapt_capacity = 0;                      // quadrants the buffers hold (every quadrant of the frame: any tile split fits)
    unsigned* h_adapt_count = nullptr;           // page-locked [2]: the active count of rounds r and r + 1, read one round behind
    hipEvent_t ev_adapt[2] = { nullptr, nullptr };
    bool adaptive_accum = false;                 // the accumulator holds an adaptive render: per-pixel counts, no single sample count

    // first-hit feature planes (ptk_render_features): allocated on first use, each for the frame feat_w x feat_h
    void* d_feat[NUM_FEATURES] = {};
    int feat_w = 0, feat_h = 0;                  // the frame the planes were allocated for and last rendered at
    uint32_t feat_mask = 0;                      // planes the last ptk_render_features wrote

    // radiance along caller-supplied rays (ptk_trace_rays): its own sample buffer between rays_kernel and rays_fold_kernel - renders
    // may still be in flight on the internal streams with theirs -, grown to the largest pass so far; the item counter and
    // parameter block of a launch; three events per pass of the last call: before rays_kernel, behind it, behind the fold
    float4* d_rays_samples = nullptr; size_t rays_samples_bytes = 0;
    RaysBlock* d_rays_block = nullptr;
    std::vector<hipEvent_t> ev_rays;
    int rays_passes = 0;                         // timed passes of the last call (at most kMaxTimedPasses)

    // lightmap baking (ptk_bake_lightmap), each grown to the largest bake so far: the owner plane (4 B per texel) with the covered
    // count per block of 256 texels behind it; the compacted rays of the covered texels (origins | dirs | sums | keys | texel
    // index, 44 B each); the second image + owner plane of ptk_lightmap_dilate (16 B per texel); the covered count's page-locked
    // read-back word; six events of the last bake: start, behind coverage + count, before and behind the ray generator, behind the
    // trace, behind the scatter
    int* d_bake_plane = nullptr; size_t bake_plane_texels = 0;
    float* d_bake_compact = nullptr; size_t bake_compact_rays = 0;
    float* d_bake_dilate = nullptr; size_t bake_dilate_texels = 0;
    uint32_t* h_bake_total = nullptr;
    hipEvent_t ev_bake[6] = { nullptr, nullptr, nullptr, nullptr, nullptr, nullptr };
    bool bake_timed = false, bake_traced = false;

    // adaptive ray queries and lightmap bakes (ptk_trace_rays_adaptive, ptk_bake_lightmap_adaptive), each grown to the largest call
    // so far: per ray 56 B - the round's compacted origins | dirs (24 B), keys, source indices, the next active list and the keep
    // flags (4 B each), S2 and the counts where the caller's arrays do not hold them (12 + 4 B) - with a count per 256 rays and the
    // total behind them; a lightmap's need plane (1 B per texel); the total's page-locked read-back word; two events around the
    // GPU work of a round; the last call's times (ptk_last_rays_adaptive_ms)
    float* d_radapt = nullptr; size_t radapt_rays = 0;
    uint8_t* d_radapt_need = nullptr; size_t radapt_need_texels = 0;
    uint32_t* h_radapt_total = nullptr;
    hipEvent_t ev_radapt[2] = { nullptr, nullptr };
    float radapt_ms[3] = { 0.0f, 0.0f, 0.0f };   // host wall time of the round loop; rays_keyed_kernel; the other kernels of the rounds

    // irradiance probe baking (ptk_bake_probes), each grown to the largest call so far: the basis table (36 B per direction), one
    // block of rays (origins | dirs, 24 B each) and, while the caller passes no table, the radiance table (12 B per ray); four
    // events of the last bake - around the basis table, around the projection - and three per block of probes (the first
    // kMaxTimedPasses of them): before the ray generator, behind it, behind the trace
    float* d_probe_basis = nullptr; size_t probe_basis_dirs = 0;
    float* d_probe_rays = nullptr; size_t probe_rays_cap = 0;
    float* d_probe_table = nullptr; size_t probe_table_rays = 0;
    hipEvent_t ev_probes[4] = { nullptr, nullptr, nullptr, nullptr };
    std::vector<hipEvent_t> ev_probe_blocks;
    int probe_blocks_timed = 0;
    bool probes_timed = false;

    // closest-hit and occlusion queries (ptk_intersect_rays, ptk_occluded_rays): two events around the last call's kernel, made
    // by the first call
    hipEvent_t ev_hits[2] = { nullptr, nullptr };
    bool hits_timed = false;

    // sample buffer between trace_kernel and accumulate_kernel (grown on demand, never shrunk)
    // Two sample buffers / queue blocks / trace streams: the trace kernel of pass k+1 runs on the other stream and
    // overlaps the tail of pass k's (a launch ends with the few waves that hold its longest paths - Russian roulette
    // lets one path in tens of millions live for 60+ bounces, ~0.4 ms with the rest of the chip idle) and pass k's
    // accumulate kernel.  The accumulate kernels stay on the context's stream, in order, each behind its trace kernel,
    // so everything the caller orders after ptk_render on that stream still sees the finished batch.
    float4* d_samples = nullptr;                 // (non-overlapped path)
    size_t samples_bytes = 0;
    float4* d_samples2[2] = { nullptr, nullptr };
    size_t samples_bytes2[2] = { 0, 0 };
    unsigned* d_queues2[2] = { nullptr, nullptr };
    hipStream_t trace_stream[2] = { nullptr, nullptr };
    hipEvent_t ev_trace_done[2] = { nullptr, nullptr }, ev_acc_done[2] = { nullptr, nullptr }, ev_inputs = nullptr;
    bool acc_pending[2] = { false, false }, inputs_recorded = false;
    bool inputs_dirty = true;                    // scene / camera tables were (re)written on the context's stream since ev_inputs
    unsigned pass_counter = 0;
    int opt_overlap = 1;
    int opt_register_out = 0;                    // 1: ptk_bind_out_image page-locks a pageable caller buffer in place (round 3's default; the caller must unbind before freeing)
    int opt_contract = 0;                        // 0: bit-exact kernels; 1: -ffp-contract=fast build; 2: ... with 1-ulp hardware rcp / sqrt
    int opt_chunk = 0;                           // samples per work item; 0 = automatic (8, or 4 for small shares)
    int num_cus = 256;
    int opt_generations = 0;                     // 0 automatic: 1 on a single GPU, 2 when the frame is split over ranks
    int opt_persistent = -1;                     // -1 automatic (by launch size), 0 one item per wave, 1 persistent waves
    int opt_max_batch = 1;                       // slots a persistent wave pops from its queue at once; > 1 measured slower everywhere
    int opt_device_build = 1;                    // scenes of >= 4096 triangles: BVH built and records packed on the GPU (bvh_device.hip)
    bool built_on_device = false;
    int opt_tri_thr = 6;                         // triangle arm of the walk runs when queued lanes >= tri_thr/8 x walking lanes
    int opt_shade_thr = 0, opt_gen_thr = 16;     // scheduling lambdas in eighths, see trace_kernel; 0 = by tree depth
    size_t opt_pass_bytes = (size_t)16 << 30;    // sample-buffer budget per pass (two such buffers at most, of the 288 GB: C4 traces its 256 spp in one launch, C5 its 1024 in two: +0.4 / +1.2 % over 4 GiB)

    // multi-GPU exchange step (ptk_gather_accum): packed gather of every rank's owned tiles to the root
    ncclComm_t comm = nullptr;                   // the context's own communicator (ptk_comm_init), or null
    int comm_rank = 0, comm_world = 1;
    hipStream_t xstream = nullptr;               // high priority: its kernels and the collective take wave slots ahead of queued trace waves
    hipEvent_t ev_rendered = nullptr, ev_packed = nullptr, ev_gathered = nullptr;
    float* d_packed = nullptr; size_t packed_floats = 0;      // non-root: this rank's packed tiles; root: every rank's, back to back
    float* d_gathered = nullptr; size_t gathered_floats = 0;  // root: the combined image (W*H*3, rows bottom-up)
    int gathered_w = 0, gathered_h = 0;          // the frame the last ptk_gather_accum combined (ptk_read_gathered refuses any other)
    bool gather_pending = false;
    // every wait of the exchange step is bounded (ptk_set_option "comm_timeout_s"): a rank that never arrives must end the run with
    // an error that names it, not hang the node (the first real 8-GPU run is the driver's, not ours)
    double opt_comm_timeout_s = 120.0;
    unsigned long long gather_step = 0;          // exchanges queued so far (named in the timeout message)
    size_t gather_bytes = 0;                     // bytes the last exchange moves on this rank (root: what it receives)
    int gather_root = 0;

    // log of every trace launch's duration (ptk_kernel_log): event pairs on the launch's own stream
    std::vector<hipEvent_t> klog_ev;             // 2 x capacity
    int klog_n = 0;
    static constexpr int kMaxTimedPasses = 64;
    hipEvent_t ev[kMaxTimedPasses][3] = {};      // per pass: before trace, after trace, after accumulate
    int last_passes = 0;
    int last_launches = 0;
    bool timed = false;
};

namespace {

int fail(ptk_ctx* c, int code, const std::string& msg)
{
    if (c) { std::lock_guard<std::mutex> g(c->err_mu); c->error = msg; }
    return code;
}
#define HIPCHK(c, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return fail(c, PTK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));          \
    } while (0)

template <class T>
void dfree(T*& p) { if (p) { (void)hipFree(p); p = nullptr; } }

float* accum_ptr(ptk_ctx* c) { return c->d_accum_bound ? c->d_accum_bound : c->d_accum; }

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
void frame_setup(ptk_ctx* c, PrimaryParams& pp)
{
    const float* pos = c->cam_pos; const float* dir = c->cam_dir; const float* up = c->cam_up;
    float center[3] = { pos[0] + dir[0] * c->focal, pos[1] + dir[1] * c->focal, pos[2] + dir[2] * c->focal };
    float img_h = (float)((double)(2.0f * c->focal) * std::tan((double)(c->fovy / 2.0f) * 3.14159265358979323846 / (double)180.0f));
    float aspect = (float)c->width / (float)c->height;
    float img_w = img_h * aspect;
    pp.delta_x = img_w / (float)c->width;
    pp.delta_y = img_h / (float)c->height;
    // camRight = normalize(cross(up, dir))
    float cr[3] = { up[1] * dir[2] - dir[1] * up[2], up[2] * dir[0] - dir[2] * up[0], up[0] * dir[1] - dir[0] * up[1] };
    normalize3(cr, c->cam_right);
    float hw = img_w * 0.5f, hh = img_h * 0.5f;
    for (int a = 0; a < 3; a++)
    {
        float tl = center[a] - c->cam_right[a] * hw;
        tl = tl + up[a] * hh;
        pp.top_left[a] = tl;
        pp.cam_pos[a] = pos[a]; pp.cam_right[a] = c->cam_right[a]; pp.cam_up[a] = up[a];
    }
    pp.primary = c->d_primary; pp.width = c->width; pp.height = c->height;
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

int ensure_primary(ptk_ctx* c)
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

bool primary_cacheable(const ptk_ctx* c)
{
    return c->opt_primary_cache && c->aperture == 0.0f && !c->scene_has_opacity && c->have_scene && c->d_primary_hit;
}

void fill_params(ptk_ctx* c, RenderParams& p, uint32_t first, uint32_t spp, uint64_t seed)
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
    for (int k = 0; k < NUM_FEATURES; k++) dfree(c->d_feat[k]);
    c->feat_w = c->feat_h = 0; c->feat_mask = 0;
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
    dfree(c->d_tri_pos); dfree(c->d_level_nodes); dfree(c->d_refit_side); dfree(c->d_refit_partial);
    c->level_start.clear();
    c->geo_updates = 0; c->sah_built = c->sah_now = 0.0; c->sah_now_pending = false;
}

void free_adaptive(ptk_ctx* c)
{
    dfree(c->d_counts); dfree(c->d_moments); dfree(c->d_adapt_active); dfree(c->d_adapt_traced); dfree(c->d_adapt_list);
    dfree(c->d_adapt_stats);
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
    if (primary_cacheable(c))
    {
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
    }
    // decided per render from the staged state: a material edit, a new scene or an opened aperture since the last one is seen here
    p.plain = (c->opt_plain_kernel && c->scene_plain && p.flat_count > 0 && p.primary_hit != nullptr) ? 1 : 0;
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
            dfree(c->d_live_mask); dfree(c->d_live_list); c->live_capacity = 0;
            HIPCHK(c, hipMalloc(&c->d_live_mask, (size_t)subtiles * sizeof(unsigned long long)));
            HIPCHK(c, hipMalloc(&c->d_live_list, ((size_t)subtiles + 1) * sizeof(unsigned)));
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
    const bool overlap = c->opt_overlap != 0 && c->trace_stream[0] != nullptr && !handoff && !ad;
    // The pass size: what the sample-buffer budget allows - and what the device can actually give.  When an allocation of that
    // size fails (memory shared with the caller's framework, a huge scene, a 144-megapixel frame) the pass is halved and tried
    // again instead of failing the render: more passes, the same image (chunk boundaries never change a bit).
    size_t budget = c->opt_pass_bytes;
    {
        const size_t have = overlap ? std::min(c->samples_bytes2[0], c->samples_bytes2[1]) : c->samples_bytes;
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
    // grows *buf to `need` bytes; false (nothing allocated, *bytes = 0) when the device refuses
    auto grow = [&](float4*& buf, size_t& bytes, size_t need) -> bool {
        dfree(buf); bytes = 0;
        if (hipMalloc(&buf, need) != hipSuccess) { (void)hipGetLastError(); buf = nullptr; return false; }
        bytes = need;
        return true;
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
                if (need > c->samples_bytes2[0] || need > c->samples_bytes2[1])
                {
                    HIPCHK(c, hipStreamSynchronize(c->trace_stream[0]));
                    HIPCHK(c, hipStreamSynchronize(c->trace_stream[1]));
                    HIPCHK(c, hipStreamSynchronize(c->stream));
                    for (int k = 0; k < 2 && ok; k++)
                        if (need > c->samples_bytes2[k]) ok = grow(c->d_samples2[k], c->samples_bytes2[k], need);
                }
            }
            else if (need > c->samples_bytes)
            {
                HIPCHK(c, hipStreamSynchronize(c->stream));
                ok = grow(c->d_samples, c->samples_bytes, need);
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
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev[pi][0], tstream));
        const int kl = (!stats && (size_t)(2 * c->klog_n + 1) < c->klog_ev.size()) ? c->klog_n : -1;
        if (kl >= 0) HIPCHK(c, hipEventRecord(c->klog_ev[2 * kl], tstream));
        p.queues = overlap ? c->d_queues2[b] : c->d_queues;
        if (c->opt_contract == 1 && !stats) fma::launch_trace(p, tiles * 4, c->resident_waves, tstream, false);
        else if (c->opt_contract == 2 && !stats) fast::launch_trace(p, tiles * 4, c->resident_waves, tstream, false);
        else launch_trace(p, tiles * 4, c->resident_waves, tstream, stats);
        HIPCHK(c, hipGetLastError());
        c->last_trace_variant = p.flat_count <= 0 ? PTK_TRACE_BVH : ((p.plain && !stats) ? PTK_TRACE_FLAT_PLAIN : PTK_TRACE_FLAT);
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev[pi][1], tstream));
        if (kl >= 0) { HIPCHK(c, hipEventRecord(c->klog_ev[2 * kl + 1], tstream)); c->klog_n = kl + 1; }
        if (overlap)
        {
            HIPCHK(c, hipEventRecord(c->ev_trace_done[b], tstream));
            HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_trace_done[b], 0));
        }
        if (ad) launch_accumulate_adaptive(p, ad->a, tiles, c->stream);
        else launch_accumulate(p, tiles, c->stream);
        HIPCHK(c, hipGetLastError());
        if (timed && pi >= 0) HIPCHK(c, hipEventRecord(c->ev[pi][2], c->stream));
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
    if (hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking) != hipSuccess) { delete c; return PTK_ERR_HIP; }
    c->own_stream = true;
    {
        int cus = 0;
        if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, device_ordinal) == hipSuccess && cus > 0)
            c->resident_waves = cus * 16;        // 4 SIMDs x 4 waves of the BVH trace kernel per CU (launch_trace scales it to x 5 for the FLAT kernel)
        if (cus > 0) c->num_cus = cus;
    }
    if (hipMalloc(&c->d_exit, sizeof(uint32_t)) != hipSuccess || hipMemset(c->d_exit, 0, sizeof(uint32_t)) != hipSuccess ||
        hipHostMalloc((void**)&c->h_exit, sizeof(uint32_t), hipHostMallocDefault) != hipSuccess ||
        hipMalloc(&c->d_stats, 16 * sizeof(unsigned long long)) != hipSuccess ||
        hipMalloc(&c->d_queues, PTK_QUEUE_BLOCK_BYTES) != hipSuccess)
    {
        ptk_destroy(c);
        return PTK_ERR_HIP;
    }
    *c->h_exit = 0;
    for (int i = 0; i < ptk_ctx::kMaxTimedPasses; i++)
        for (int k = 0; k < 3; k++)
            if (hipEventCreate(&c->ev[i][k]) != hipSuccess) { ptk_destroy(c); return PTK_ERR_HIP; }
    for (int b = 0; b < 2; b++)
        if (hipStreamCreateWithFlags(&c->trace_stream[b], hipStreamNonBlocking) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_trace_done[b], hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_acc_done[b], hipEventDisableTiming) != hipSuccess ||
            hipMalloc(&c->d_queues2[b], PTK_QUEUE_BLOCK_BYTES) != hipSuccess)
        { ptk_destroy(c); return PTK_ERR_HIP; }
    if (hipEventCreateWithFlags(&c->ev_inputs, hipEventDisableTiming) != hipSuccess) { ptk_destroy(c); return PTK_ERR_HIP; }
    if (hipStreamCreateWithFlags(&c->geo_stream, hipStreamNonBlocking) != hipSuccess ||
        hipMalloc(&c->d_geo_red, GEO_RED_WORDS * sizeof(uint32_t) + sizeof(double)) != hipSuccess ||
        hipHostMalloc((void**)&c->h_geo_red, GEO_RED_WORDS * sizeof(uint32_t), hipHostMallocDefault) != hipSuccess)
    { ptk_destroy(c); return PTK_ERR_HIP; }
    for (hipEvent_t& e : c->ev_geo_t)
        if (hipEventCreate(&e) != hipSuccess) { ptk_destroy(c); return PTK_ERR_HIP; }
    {
        int lo = 0, hi = 0;                      // (numerically lowest = greatest priority)
        (void)hipDeviceGetStreamPriorityRange(&lo, &hi);
        if (hipStreamCreateWithPriority(&c->xstream, hipStreamNonBlocking, hi) != hipSuccess ||
            hipStreamCreateWithPriority(&c->exit_stream, hipStreamNonBlocking, hi) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_rendered, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_packed, hipEventDisableTiming) != hipSuccess ||
            hipEventCreateWithFlags(&c->ev_gathered, hipEventDisableTiming) != hipSuccess)
        { ptk_destroy(c); return PTK_ERR_HIP; }
    }
    *out = c;
    return PTK_OK;
}

void ptk_destroy(ptk_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    unbind_out_image(c);
    dfree(c->d_nodes); dfree(c->d_tris); dfree(c->d_shade); dfree(c->d_mats); dfree(c->d_lights);
    dfree(c->d_flat_tris);
    free_geometry_cache(c); dfree(c->d_verts_res); dfree(c->d_geo_stage); dfree(c->d_geo_red);
    if (c->h_geo_red) (void)hipHostFree(c->h_geo_red);
    if (c->geo_stream) { (void)hipStreamSynchronize(c->geo_stream); (void)hipStreamDestroy(c->geo_stream); }
    for (hipEvent_t e : c->ev_geo_t) if (e) (void)hipEventDestroy(e);
    dfree(c->d_texinfo); dfree(c->d_texels); dfree(c->d_primary); dfree(c->d_primary_hit); dfree(c->d_primary_rd); dfree(c->d_accum); dfree(c->d_rgb8);
    dfree(c->d_pixel_rng);
    for (int b = 0; b < 2; b++)
    {
        if (c->trace_stream[b]) { (void)hipStreamSynchronize(c->trace_stream[b]); (void)hipStreamDestroy(c->trace_stream[b]); }
        if (c->ev_trace_done[b]) (void)hipEventDestroy(c->ev_trace_done[b]);
        if (c->ev_acc_done[b]) (void)hipEventDestroy(c->ev_acc_done[b]);
        dfree(c->d_samples2[b]); dfree(c->d_queues2[b]);
    }
    if (c->ev_inputs) (void)hipEventDestroy(c->ev_inputs);
    if (c->xstream) { (void)hipStreamSynchronize(c->xstream); }
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    if (c->ev_rendered) (void)hipEventDestroy(c->ev_rendered);
    if (c->ev_packed) (void)hipEventDestroy(c->ev_packed);
    if (c->ev_gathered) (void)hipEventDestroy(c->ev_gathered);
    dfree(c->d_packed); dfree(c->d_gathered);
    if (c->exit_stream) { (void)hipStreamSynchronize(c->exit_stream); (void)hipStreamDestroy(c->exit_stream); }
    if (c->h_exit) (void)hipHostFree(c->h_exit);
    dfree(c->d_exit); dfree(c->d_stats); dfree(c->d_queues); dfree(c->d_samples);
    dfree(c->d_live_mask); dfree(c->d_live_list);
    free_adaptive(c);
    free_features(c);
    dfree(c->d_rays_samples); dfree(c->d_rays_block);
    dfree(c->d_bake_plane); dfree(c->d_bake_compact); dfree(c->d_bake_dilate);
    if (c->h_bake_total) (void)hipHostFree(c->h_bake_total);
    dfree(c->d_radapt); dfree(c->d_radapt_need);
    if (c->h_radapt_total) (void)hipHostFree(c->h_radapt_total);
    for (hipEvent_t e : c->ev_radapt) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_bake) if (e) (void)hipEventDestroy(e);
    dfree(c->d_probe_basis); dfree(c->d_probe_rays); dfree(c->d_probe_table);
    for (hipEvent_t e : c->ev_probes) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_probe_blocks) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_rays) (void)hipEventDestroy(e);
    for (hipEvent_t e : c->ev_hits) if (e) (void)hipEventDestroy(e);
    for (int b = 0; b < 2; b++)
        if (c->ev_adapt[b]) (void)hipEventDestroy(c->ev_adapt[b]);
    if (c->h_adapt_count) (void)hipHostFree(c->h_adapt_count);
    for (int i = 0; i < ptk_ctx::kMaxTimedPasses; i++)
        for (int k = 0; k < 3; k++)
            if (c->ev[i][k]) (void)hipEventDestroy(c->ev[i][k]);
    for (hipEvent_t e : c->klog_ev) (void)hipEventDestroy(e);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
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
    if (c->own_stream && c->stream) { (void)hipStreamSynchronize(c->stream); (void)hipStreamDestroy(c->stream); }
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
    HIPCHK(c, hipStreamSynchronize(c->stream));

    const auto t_begin = std::chrono::steady_clock::now();
    auto ms_since = [](std::chrono::steady_clock::time_point t0) { return std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count(); };
    // BVH: on the device for scenes large enough to matter (replaces BVHNode::Construct, mesh.cpp:169-211), else - or when
    // the device build cannot meet the traversal-stack bound - by the host builder, which always can
    BuiltBvh bvh;
    DeviceBvh dbvh;
    bool on_device = false;
    float* d_verts = nullptr;
    struct TmpFree { std::vector<void*> p; ~TmpFree() { for (void* q : p) if (q) (void)hipFree(q); } } tmp;
    if (c->opt_device_build && n >= 4096)
    {
        HIPCHK(c, hipMalloc(&d_verts, (size_t)n * 9 * sizeof(float)));
        tmp.p.push_back(d_verts);
        HIPCHK(c, hipMemcpyAsync(d_verts, s->verts, (size_t)n * 9 * sizeof(float), hipMemcpyHostToDevice, c->stream));
        std::string derr;
        int leaf_max = 4;
        if (g_bvh_tuning.leaf_max > 0) leaf_max = g_bvh_tuning.leaf_max;                              // ptk_set_option "bvh_leaf_max"
        on_device = build_bvh_device(d_verts, n, PTK_MAX_BVH_DEPTH, leaf_max, c->stream, dbvh, &derr);
        if (on_device && dbvh.stack_need > PTK_MAX_BVH_DEPTH) { (void)hipFree(dbvh.d_nodes); (void)hipFree(dbvh.d_order); on_device = false; }
    }
    if (!on_device)
    {
        if (!build_bvh(s->verts, n, PTK_MAX_BVH_DEPTH, 4, bvh))
            return fail(c, PTK_ERR_LIMIT, "BVH exceeds the kernel's depth / index limits");
        if (bvh.stack_need > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    }
    struct DevBvhGuard { DeviceBvh& d; bool armed; ~DevBvhGuard() { if (armed) { (void)hipFree(d.d_nodes); (void)hipFree(d.d_order); } } } dguard{ dbvh, on_device };
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
    dfree(c->d_nodes); dfree(c->d_tris); dfree(c->d_shade); dfree(c->d_mats); dfree(c->d_lights);
    dfree(c->d_texinfo); dfree(c->d_texels);
    dfree(c->d_verts_res); free_geometry_cache(c);
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
        dfree(c->d_flat_tris);
        // the records are packed on the device from the boundary's flat arrays (one pass each; no host-side copies)
        float *d_normals = nullptr, *d_uvs = nullptr, *d_tbn = nullptr; uint8_t* d_smooth = nullptr; int32_t *d_material = nullptr, *d_optex = nullptr;
        std::vector<int32_t> optex(std::max<int32_t>(s->num_materials, 1), -1);
        for (int32_t i = 0; i < s->num_materials; i++) { const int32_t ot = s->materials[i].tex[5]; optex[i] = ot >= 0 ? texmap[ot] : -1; }
        auto tup = [&](void** dst, const void* src, size_t bytes) -> hipError_t {
            hipError_t e = hipMalloc(dst, bytes ? bytes : 16);
            if (e != hipSuccess) return e;
            tmp.p.push_back(*dst);
            return bytes ? hipMemcpyAsync(*dst, src, bytes, hipMemcpyHostToDevice, c->stream) : hipSuccess;
        };
        HIPCHK(c, tup((void**)&d_normals, s->normals, (size_t)n * 9 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_uvs, s->uvs, (size_t)n * 6 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_tbn, s->tbn, (size_t)n * 9 * sizeof(float)));
        HIPCHK(c, tup((void**)&d_smooth, s->smoothing, (size_t)n));
        HIPCHK(c, tup((void**)&d_material, s->material, (size_t)n * sizeof(int32_t)));
        HIPCHK(c, tup((void**)&d_optex, optex.data(), optex.size() * sizeof(int32_t)));
        HIPCHK(c, hipMalloc(&c->d_tris, (size_t)n * TRI_F4 * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_shade, (size_t)n * SHADE_F4 * sizeof(float4)));
        launch_pack_tris(d_verts, dbvh.d_order, d_material, d_optex, c->d_tris, n, c->stream);
        launch_pack_shade(d_normals, d_uvs, d_tbn, d_smooth, d_material, c->d_shade, n, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->d_nodes = dbvh.d_nodes; dguard.armed = false;
        c->d_verts_res = d_verts; tmp.p[0] = nullptr;              // the builder's input stays resident (ptk_update_geometry)
        (void)hipFree(dbvh.d_order); dbvh.d_order = nullptr;
        bvh.num_nodes = dbvh.num_nodes; bvh.depth = dbvh.depth; bvh.stack_need = dbvh.stack_need;
    }
    else
    {
        HIPCHK(c, up((void**)&c->d_nodes, bvh.nodes.data(), bvh.nodes.size() * 4));
        HIPCHK(c, up((void**)&c->d_tris, tris.data(), tris.size() * 4));
        dfree(c->d_flat_tris);
        if (n > 0 && n <= 16)
        {
            std::vector<float> flat((size_t)(FLAT_FRAMES_AT + n * FLAT_FRAME_F4) * 4);     // records, room up to FLAT_MAX_TRIS, frame table
            for (int32_t k = 0; k < n; k++)             // record of leaf position k holds triangle bvh.order[k]
                std::memcpy(flat.data() + (size_t)bvh.order[k] * TRI_F4 * 4, tris.data() + (size_t)k * TRI_F4 * 4, TRI_F4 * 16);
            HIPCHK(c, up((void**)&c->d_flat_tris, flat.data(), flat.size() * 4));
        }
        HIPCHK(c, up((void**)&c->d_shade, shade.data(), shade.size() * 4));
        if (c->d_flat_tris)                             // the frame table behind the flat records, from the normals just written
        {
            launch_flat_frames(c->d_shade, c->d_flat_tris, 0, n, c->stream);
            HIPCHK(c, hipGetLastError());
        }
        HIPCHK(c, up((void**)&c->d_verts_res, s->verts, (size_t)n * 9 * sizeof(float)));
    }
    c->built_on_device = on_device;
    HIPCHK(c, up((void**)&c->d_mats, mats.data(), mats.size() * 4));
    HIPCHK(c, up((void**)&c->d_lights, lights.data(), lights.size() * 4));
    HIPCHK(c, up((void**)&c->d_texinfo, texinfo.data(), texinfo.size() * sizeof(int4)));
    HIPCHK(c, up((void**)&c->d_texels, texels.data(), texels.size() * 4));
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
    c->inputs_dirty = true;
    return PTK_OK;
}

// ---- geometry updates after ptk_upload_scene (ptk.h) ----------------------------------------------------------
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
    int32_t* d_list = nullptr; int32_t* d_pos = nullptr; float4* d_side = nullptr; double* d_partial = nullptr;
    hipError_t e = hipMalloc(&d_list, (size_t)nn * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&d_partial, ((size_t)nn + 255) / 256 * sizeof(double));
    if (e == hipSuccess) e = hipMalloc(&d_pos, (size_t)nt * sizeof(int32_t));
    if (e == hipSuccess) e = hipMalloc(&d_side, (size_t)nn * 2 * sizeof(float4));
    if (e == hipSuccess) e = hipMemcpy(d_list, list.data(), (size_t)nn * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemsetAsync(d_pos, 0, (size_t)nt * sizeof(int32_t), c->stream);
    if (e != hipSuccess)
    {
        (void)hipFree(d_list); (void)hipFree(d_pos); (void)hipFree(d_side); (void)hipFree(d_partial);
        return fail(c, PTK_ERR_HIP, std::string("refit tables: ") + hipGetErrorString(e));
    }
    c->d_level_nodes = d_list; c->d_tri_pos = d_pos; c->d_refit_side = d_side; c->d_refit_partial = d_partial;
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
    if (floats > c->geo_stage_floats)
    {
        if (c->geo_done_recorded) HIPCHK(c, hipEventSynchronize(c->ev_geo_t[4]));       // (the previous update's repack reads the old buffer)
        dfree(c->d_geo_stage); c->geo_stage_floats = 0;
        HIPCHK(c, hipMalloc(&c->d_geo_stage, floats * sizeof(float)));
        c->geo_stage_floats = floats;
    }
    float* sv = c->d_geo_stage; float* sn = normals ? sv + per : nullptr; float* st = normals ? sv + 2 * per : nullptr;
    const hipMemcpyKind kind = on_device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
    if (c->geo_done_recorded) HIPCHK(c, hipStreamWaitEvent(c->geo_stream, c->ev_geo_t[4], 0));
    HIPCHK(c, hipEventRecord(c->ev_geo_t[0], c->geo_stream));
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
    HIPCHK(c, hipEventRecord(c->ev_geo_t[1], c->geo_stream));
    // the one host wait of an update: for the staging stream, which stands behind the PREVIOUS update only - renders queued
    // since then are not waited for; the caller's arrays are free again from here on
    HIPCHK(c, hipStreamSynchronize(c->geo_stream));
    const uint32_t* red = c->h_geo_red;
    if (red[7]) return fail(c, PTK_ERR_LIMIT, limit_msg);
    float vmax; std::memcpy(&vmax, &red[6], 4);

    // 2. rewrite on the context's stream: behind every render already queued - their accumulate kernels are on this stream,
    // each behind its trace kernel on the internal streams, so no trace still reads the old records - and ahead of every
    // later one (inputs_dirty re-anchors the trace streams behind these kernels)
    HIPCHK(c, hipEventRecord(c->ev_geo_t[2], c->stream));
    launch_repack_geometry(sv, sn, st, first, count, c->d_verts_res, c->d_tri_pos, c->d_tris, c->d_flat_tris, c->d_shade, c->stream);
    launch_repack_lights(c->d_verts_res, first, count, c->d_lights, c->num_lights, c->stream);
    if (c->d_flat_tris && sn) launch_flat_frames(c->d_shade, c->d_flat_tris, first, count, c->stream);     // (vertices only: the normals stay)
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_geo_t[3], c->stream));
    c->bvh_pad = 1e-5f * std::max(vmax, 1.0f);
    queue_refit(c, c->bvh_pad, 1, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_geo_t[4], c->stream));
    c->geo_done_recorded = true;

    c->scene_bound = 3.1f * (1.01f * vmax + 1e-3f);
    for (int a = 0; a < 3; a++) { c->scene_lo[a] = geo_dec(~red[a]); c->scene_hi[a] = geo_dec(red[3 + a]); }
    if (c->num_lights > 0) c->lights_stale = true;
    c->geo_updates++;
    c->sah_now_pending = true;
    c->view_generation++;
    c->primary_hit_dirty = true;
    c->out_full_next = true;
    c->inputs_dirty = true;
    return PTK_OK;
}

}  // namespace

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
    if (!c->geo_done_recorded) return fail(c, PTK_ERR_BAD_ARG, "no geometry update yet");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(c->ev_geo_t[4]));
    HIPCHK(c, hipEventElapsedTime(&ms3[0], c->ev_geo_t[0], c->ev_geo_t[1]));
    HIPCHK(c, hipEventElapsedTime(&ms3[1], c->ev_geo_t[2], c->ev_geo_t[3]));
    HIPCHK(c, hipEventElapsedTime(&ms3[2], c->ev_geo_t[3], c->ev_geo_t[4]));
    return PTK_OK;
}

int ptk_scene_is_plain(const ptk_scene_desc* s)
{
    if (!s) return 0;
    return plain_tables(s->num_triangles, s->smoothing, s->material, s->num_materials, s->materials) ? 1 : 0;
}

int ptk_trace_variant(ptk_ctx* c, int* variant)
{
    if (!c || !variant) return PTK_ERR_BAD_ARG;
    *variant = c->last_trace_variant;
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
        dfree(c->d_primary); dfree(c->d_primary_hit); dfree(c->d_primary_rd); dfree(c->d_accum); dfree(c->d_rgb8); dfree(c->d_pixel_rng);
        c->pixel_rng_valid = false;
        size_t px = (size_t)width * height;
        HIPCHK(c, hipMalloc(&c->d_primary, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_primary_hit, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_primary_rd, px * sizeof(float4)));
        HIPCHK(c, hipMalloc(&c->d_pixel_rng, px * sizeof(uint2)));
        HIPCHK(c, hipMalloc(&c->d_accum, px * 3 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_rgb8, px * 3));
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
    c->timed = false;
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
    c->timed = true;
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
    c->timed = false;
    const size_t px = (size_t)c->width * c->height;
    const int tiles_x = (c->width + PTK_TILE - 1) / PTK_TILE;
    const int capacity = tiles_x * ((c->height + PTK_TILE - 1) / PTK_TILE) * 4;
    if (c->adapt_capacity != capacity || !c->d_counts)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        free_adaptive(c);
        HIPCHK(c, hipMalloc(&c->d_counts, px * sizeof(uint32_t)));
        HIPCHK(c, hipMalloc(&c->d_moments, px * 3 * sizeof(float)));
        HIPCHK(c, hipMalloc(&c->d_adapt_active, (size_t)capacity * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(&c->d_adapt_traced, (size_t)capacity * sizeof(unsigned long long)));
        HIPCHK(c, hipMalloc(&c->d_adapt_list, ((size_t)capacity + 1) * sizeof(unsigned)));
        HIPCHK(c, hipMalloc(&c->d_adapt_stats, 4 * sizeof(unsigned long long)));
        c->adapt_capacity = capacity;
    }
    if (!c->h_adapt_count)
    {
        HIPCHK(c, hipHostMalloc((void**)&c->h_adapt_count, 2 * sizeof(unsigned), hipHostMallocDefault));
        for (int b = 0; b < 2; b++) HIPCHK(c, hipEventCreateWithFlags(&c->ev_adapt[b], hipEventDisableTiming));
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
        if (__atomic_load_n(c->h_exit, __ATOMIC_RELAXED) >= gen) break;                        // Exit(): the rest stands down anyway
    }
    HIPCHK(c, hipStreamSynchronize(c->stream));
    unsigned long long st[3] = { 0, 0, 0 };
    HIPCHK(c, hipMemcpyAsync(st, c->d_adapt_stats, sizeof(st), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    uint64_t active = 0;
    const bool cut = __atomic_load_n(c->h_exit, __ATOMIC_RELAXED) >= gen;
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
    if (primary_cacheable(c))
    {
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
    }
    const size_t px = (size_t)c->width * c->height;
    c->feat_mask = 0;
    for (int k = 0; k < NUM_FEATURES; k++)
        if (((mask >> k) & 1u) && !c->d_feat[k]) HIPCHK(c, hipMalloc(&c->d_feat[k], px * kFeatChannels[k] * 4));
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
    // one ray: [0] the triangle, [1] its material index, [2] the bits of t
    int32_t* d_out = nullptr;
    HIPCHK(c, hipMalloc(&d_out, 3 * sizeof(int32_t)));
    RenderParams p;
    fill_params(c, p, 0, 1, seed);
    FeatureParams f = {};
    f.sample = 0; f.seed_lo = (uint32_t)seed; f.seed_hi = (uint32_t)(seed >> 32);
    launch_pick(p, f, y_top_down * c->width + x, d_out, c->stream);
    int32_t out[3] = { -1, -1, 0 };
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, sizeof(out), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    float th; std::memcpy(&th, &out[2], 4);
    if (tri) *tri = out[0];
    if (material) *material = out[1];
    if (t) *t = th;
    return PTK_OK;
}

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
    c->rays_passes = 0;
    if (!c->d_rays_block) HIPCHK(c, hipMalloc(&c->d_rays_block, sizeof(RaysBlock)));
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
        if (want > c->rays_samples_bytes)        // (only a call that has to allocate asks the driver)
        {
            if (hipMemGetInfo(&free_b, &total_b) == hipSuccess) budget = std::min(budget, std::max(std::max(free_b / 2, c->rays_samples_bytes), group_bytes));
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
        if (need <= c->rays_samples_bytes) break;
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->d_rays_samples); c->rays_samples_bytes = 0;
        if (hipMalloc(&c->d_rays_samples, need) == hipSuccess) { c->rays_samples_bytes = need; break; }
        (void)hipGetLastError(); c->d_rays_samples = nullptr;
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
            const int pi = c->rays_passes < ptk_ctx::kMaxTimedPasses ? c->rays_passes : -1;
            if (pi >= 0)
                while (c->ev_rays.size() < (size_t)(pi + 1) * 3)
                {
                    hipEvent_t e = nullptr;
                    HIPCHK(c, hipEventCreate(&e));
                    c->ev_rays.push_back(e);
                }
            if (pi >= 0) HIPCHK(c, hipEventRecord(c->ev_rays[pi * 3], c->stream));
            launch_rays(p, r, c->d_rays_block, c->resident_waves, c->stream);
            HIPCHK(c, hipGetLastError());
            if (pi >= 0) HIPCHK(c, hipEventRecord(c->ev_rays[pi * 3 + 1], c->stream));
            fold(ray0, (int)nr, p.chunk, p.num_chunks, n, done);
            HIPCHK(c, hipGetLastError());
            if (pi >= 0) { HIPCHK(c, hipEventRecord(c->ev_rays[pi * 3 + 2], c->stream)); c->rays_passes = pi + 1; }
            done += n;
        }
    }
    return PTK_OK;
}

static int trace_rays_on_stream(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, uint32_t first_sample,
                                uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, const uint32_t* d_keys = nullptr)
{
    c->rays_passes = 0;
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
    int rc = check_rays_args(c, num_rays, origins, dirs, flags, out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // origins | dirs | out, staged for the length of the call
    const size_t n3 = (size_t)num_rays * 3, bytes = n3 * sizeof(float);
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, 3 * bytes));
    hipError_t e = hipMemcpyAsync(d, origins, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n3, dirs, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && (flags & PTK_RAYS_ACCUMULATE)) e = hipMemcpyAsync(d + 2 * n3, out, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = trace_rays_on_stream(c, num_rays, d, d + n3, max_depth, first_sample, spp, seed, key_base, flags, d + 2 * n3);
        if (rc == PTK_OK) e = hipMemcpyAsync(out, d + 2 * n3, bytes, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_last_rays_ms(ptk_ctx* c, float* trace_ms, float* fold_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float t = 0.0f, f = 0.0f;
    for (int i = 0; i < c->rays_passes; i++)
    {
        float a = 0.0f, b = 0.0f;
        HIPCHK(c, hipEventSynchronize(c->ev_rays[i * 3 + 2]));
        HIPCHK(c, hipEventElapsedTime(&a, c->ev_rays[i * 3], c->ev_rays[i * 3 + 1]));
        HIPCHK(c, hipEventElapsedTime(&b, c->ev_rays[i * 3 + 1], c->ev_rays[i * 3 + 2]));
        t += a; f += b;
    }
    if (trace_ms) *trace_ms = t;
    if (fold_ms) *fold_ms = f;
    return PTK_OK;
}

// ---- closest-hit and occlusion queries for caller-supplied rays (ptk.h) --------------------------------------------------------
// The argument checks the entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_hits_args(ptk_ctx* c, const char* who, int32_t num_rays, const float* origins, const float* dirs, bool have_out, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (num_rays < 0) return fail(c, PTK_ERR_BAD_ARG, (std::string(who) + ": negative ray count").c_str());
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!have_out) return fail(c, PTK_ERR_BAD_ARG, (std::string(who) + ": no output array").c_str());
    if (num_rays > 0 && (!origins || !dirs)) return fail(c, PTK_ERR_BAD_ARG, (std::string(who) + ": null array").c_str());
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    *nothing = num_rays == 0;
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory: h holds the rays and the outputs, the scene
// half is filled in here.  One kernel between the two events; a scene without triangles has no tree to walk and gets its misses
// from fills.
static int hits_on_stream(ptk_ctx* c, HitsParams& h, uint32_t sample, uint64_t seed, uint32_t key_base, bool occlusion)
{
    c->hits_timed = false;
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
    for (hipEvent_t& e : c->ev_hits)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    HIPCHK(c, hipEventRecord(c->ev_hits[0], c->stream));
    if (occlusion) launch_occluded(h, c->stream); else launch_hits(h, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_hits[1], c->stream));
    c->hits_timed = true;
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

// The host entries: origins | dirs | tmax | the requested outputs in one staging buffer (every part a multiple of 4 B but the
// occlusion bytes, which come last)
static int hits_staged(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample, uint64_t seed,
                       uint32_t key_base, int32_t* tri, float* t, float* bary, int32_t* material, uint8_t* occluded)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)num_rays, w = sizeof(float);
    const size_t words = 6 * n + (tmax ? n : 0) + (tri ? n : 0) + (t ? n : 0) + (bary ? 2 * n : 0) + (material ? n : 0);
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, words * w + (occluded ? n : 0)));
    float* q = d;
    auto take = [&](size_t k) { float* r = q; q += k; return r; };
    HitsParams h = {};
    float* const d_o = take(3 * n), * const d_d = take(3 * n);
    h.origins = d_o; h.dirs = d_d; h.num_rays = num_rays;
    float* const d_tmax = tmax ? take(n) : nullptr;
    h.tmax = d_tmax;
    if (tri) h.tri = (int32_t*)take(n);
    if (t) h.t = take(n);
    if (bary) h.bary = take(2 * n);
    if (material) h.material = (int32_t*)take(n);
    if (occluded) h.occluded = (uint8_t*)q;
    int rc = PTK_OK;
    hipError_t e = hipMemcpyAsync(d_o, origins, 3 * n * w, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_d, dirs, 3 * n * w, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && tmax) e = hipMemcpyAsync(d_tmax, tmax, n * w, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = hits_on_stream(c, h, sample, seed, key_base, occluded != nullptr);
        if (rc == PTK_OK && tri) e = hipMemcpyAsync(tri, h.tri, n * w, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && t) e = hipMemcpyAsync(t, h.t, n * w, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && bary) e = hipMemcpyAsync(bary, h.bary, 2 * n * w, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && material) e = hipMemcpyAsync(material, h.material, n * w, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && occluded) e = hipMemcpyAsync(occluded, h.occluded, n, hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_intersect_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, uint32_t sample, uint64_t seed, uint32_t key_base,
                       int32_t* tri, float* t, float* bary, int32_t* material)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_intersect_rays", num_rays, origins, dirs, tri || t || bary || material, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    return hits_staged(c, num_rays, origins, dirs, nullptr, sample, seed, key_base, tri, t, bary, material, nullptr);
}

int ptk_occluded_rays(ptk_ctx* c, int32_t num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample, uint64_t seed,
                      uint32_t key_base, uint8_t* occluded)
{
    bool nothing;
    const int rc = check_hits_args(c, "ptk_occluded_rays", num_rays, origins, dirs, num_rays == 0 || occluded, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    return hits_staged(c, num_rays, origins, dirs, tmax, sample, seed, key_base, nullptr, nullptr, nullptr, nullptr, occluded);
}

int ptk_last_hits_ms(ptk_ctx* c, float* ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t = 0.0f;
    if (c->hits_timed)
    {
        HIPCHK(c, hipSetDevice(c->device));
        HIPCHK(c, hipEventSynchronize(c->ev_hits[1]));
        HIPCHK(c, hipEventElapsedTime(&t, c->ev_hits[0], c->ev_hits[1]));
    }
    if (ms) *ms = t;
    return PTK_OK;
}

// ---- lightmap baking (ptk.h) -------------------------------------------------------------------------------------------------
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
    c->bake_timed = false; c->bake_traced = false;
    for (hipEvent_t& e : c->ev_bake)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    if (texels > c->bake_plane_texels)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->d_bake_plane); c->d_bake_plane = nullptr; c->bake_plane_texels = 0;
        // the plane, then one count per block of 256 texels
        HIPCHK(c, hipMalloc(&c->d_bake_plane, (texels + blocks + 1) * sizeof(int)));
        c->bake_plane_texels = texels;
    }
    b = BakeParams{};
    b.uvs = d_uvs; b.shade = c->d_shade; b.verts = c->d_verts_res; b.num_tris = c->d_verts_res ? c->num_tris : 0;
    b.width = width; b.height = height; b.offset = offset; b.back = (flags & PTK_BAKE_BACK) ? 1 : 0; b.key_base = key_base;
    b.plane = c->d_bake_plane; b.block_counts = (uint32_t*)(c->d_bake_plane + c->bake_plane_texels);
    b.owner = d_owner; b.bary = d_bary; b.pos = d_pos;
    HIPCHK(c, hipEventRecord(c->ev_bake[0], c->stream));
    HIPCHK(c, hipMemsetD32Async((hipDeviceptr_t)b.plane, PTK_BAKE_UNOWNED, texels, c->stream));
    launch_bake_cover(b, c->stream);
    HIPCHK(c, hipGetLastError());
    covered = 0;
    if (want_rays)
    {
        // the covered count sizes the compacted arrays and the trace: the one host wait of a bake
        if (!c->h_bake_total) HIPCHK(c, hipHostMalloc((void**)&c->h_bake_total, sizeof(uint32_t), hipHostMallocDefault));
        uint32_t* d_total = b.block_counts + blocks;
        launch_bake_count(b, d_total, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipEventRecord(c->ev_bake[1], c->stream));
        HIPCHK(c, hipMemcpyAsync(c->h_bake_total, d_total, sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        covered = *c->h_bake_total;
        if (covered > texels) return fail(c, PTK_ERR_HIP, "ptk_bake_lightmap: covered count exceeds the map");
        if (covered > c->bake_compact_rays)
        {
            dfree(c->d_bake_compact); c->d_bake_compact = nullptr; c->bake_compact_rays = 0;
            HIPCHK(c, hipMalloc(&c->d_bake_compact, (size_t)covered * 11 * sizeof(float)));
            c->bake_compact_rays = covered;
        }
        if (covered)
        {
            const size_t cap = c->bake_compact_rays;
            b.origins = c->d_bake_compact; b.dirs = b.origins + cap * 3; b.sums = b.dirs + cap * 3;
            b.keys = (uint32_t*)(b.sums + cap * 3); b.texel = b.keys + cap;
            b.out = acc_out;
        }
    }
    else HIPCHK(c, hipEventRecord(c->ev_bake[1], c->stream));
    HIPCHK(c, hipEventRecord(c->ev_bake[2], c->stream));
    launch_bake_rays(b, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_bake[3], c->stream));
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
        HIPCHK(c, hipEventRecord(c->ev_bake[4], c->stream));
        if (!(flags & PTK_BAKE_ACCUMULATE)) HIPCHK(c, hipMemsetAsync(d_out, 0, texels * 3 * sizeof(float), c->stream));     // uncovered texels
        launch_bake_scatter(b.sums, b.texel, covered, d_out, c->stream);
        HIPCHK(c, hipGetLastError());
        c->bake_traced = true;
    }
    else HIPCHK(c, hipEventRecord(c->ev_bake[4], c->stream));
    HIPCHK(c, hipEventRecord(c->ev_bake[5], c->stream));
    c->bake_timed = true;
    return PTK_OK;
}

// Host entries: uvs | out | owner | bary | pos staged in one device buffer for the length of the call.
static int bake_staged(ptk_ctx* c, int width, int height, const float* uvs, float offset, int max_depth, uint32_t first_sample, uint32_t spp,
                       uint64_t seed, uint32_t key_base, uint32_t flags, float* out, int32_t* owner, float* bary, float* pos)
{
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height, n_uv = uvs ? (size_t)c->num_tris * 6 : 0;
    const size_t words = n_uv + (out ? texels * 3 : 0) + (owner ? texels : 0) + (bary ? texels * 2 : 0) + (pos ? texels * 3 : 0);
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, std::max<size_t>(words, 1) * sizeof(float)));
    float* q = d;
    const float* d_uvs = n_uv ? q : nullptr; q += n_uv;
    float* d_out = out ? q : nullptr; q += out ? texels * 3 : 0;
    int32_t* d_owner = owner ? (int32_t*)q : nullptr; q += owner ? texels : 0;
    float* d_bary = bary ? q : nullptr; q += bary ? texels * 2 : 0;
    float* d_pos = pos ? q : nullptr;
    hipError_t e = hipSuccess;
    int rc = PTK_OK;
    if (n_uv) e = hipMemcpyAsync(d, uvs, n_uv * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && out && (flags & PTK_BAKE_ACCUMULATE)) e = hipMemcpyAsync(d_out, out, texels * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = bake_on_stream(c, width, height, d_uvs, offset, max_depth, first_sample, spp, seed, key_base, flags, d_out, d_owner, d_bary, d_pos);
        if (rc == PTK_OK && out) e = hipMemcpyAsync(out, d_out, texels * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && owner) e = hipMemcpyAsync(owner, d_owner, texels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && bary) e = hipMemcpyAsync(bary, d_bary, texels * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && pos) e = hipMemcpyAsync(pos, d_pos, texels * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
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

// ---- adaptive ray queries and lightmap bakes (ptk.h) -------------------------------------------------------------------------
static int check_adaptive_args(ptk_ctx* c, const char* who, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp)
{
    if (step < 2 || min_spp == 0 || min_spp % step != 0 || max_spp % step != 0 || min_spp > max_spp)
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": need step >= 2 dividing min_spp and max_spp, 0 < min_spp <= max_spp");
    if (!std::isfinite(threshold) || threshold < 0.0f) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": threshold must be finite and >= 0");
    return PTK_OK;
}

// the context's adaptive buffer, cut up for its capacity
struct RaysAdaptiveBuffers {
    float *origins, *dirs, *s2;
    uint32_t *keys, *src, *list, *keep, *counts, *block_counts, *total;
};
static RaysAdaptiveBuffers radapt_buffers(ptk_ctx* c)
{
    const size_t cap = c->radapt_rays;
    RaysAdaptiveBuffers a;
    a.origins = c->d_radapt; a.dirs = a.origins + cap * 3; a.s2 = a.dirs + cap * 3;
    a.keys = (uint32_t*)(a.s2 + cap * 3); a.src = a.keys + cap; a.list = a.src + cap; a.keep = a.list + cap; a.counts = a.keep + cap;
    a.block_counts = a.counts + cap; a.total = a.block_counts + (cap + 255) / 256;
    return a;
}

// The round loop on the context's stream, every pointer into this GPU's memory; n > 0.  s2 / counts null: the context's own.
// texel not null: a lightmap's covered texels (keys = their RNG pixels; the 3x3 rule over the width x height map).  Synchronous:
// every round ends with the host reading the next round's ray count.
static int rays_adaptive_on_stream(ptk_ctx* c, uint32_t n, const float* d_origins, const float* d_dirs, const uint32_t* d_keys, uint32_t key_base,
                                   int max_depth, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t rays_flags,
                                   float* s1, float* s2, uint32_t* counts, const uint32_t* texel, int width, int height, ptk_rays_adaptive_result* res)
{
    const auto t0 = std::chrono::steady_clock::now();
    c->radapt_ms[0] = c->radapt_ms[1] = c->radapt_ms[2] = 0.0f;
    if (n > c->radapt_rays)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->d_radapt); c->d_radapt = nullptr; c->radapt_rays = 0;
        HIPCHK(c, hipMalloc(&c->d_radapt, ((size_t)n * 14 + ((size_t)n + 255) / 256 + 1) * sizeof(float)));
        c->radapt_rays = n;
    }
    if (!c->h_radapt_total)
    {
        HIPCHK(c, hipHostMalloc((void**)&c->h_radapt_total, sizeof(uint32_t), hipHostMallocDefault));
        for (hipEvent_t& e : c->ev_radapt) HIPCHK(c, hipEventCreate(&e));
    }
    const RaysAdaptiveBuffers a = radapt_buffers(c);
    if (!s2) s2 = a.s2;
    if (!counts) counts = a.counts;
    uint8_t* need = nullptr;
    if (texel)
    {
        const size_t texels = (size_t)width * height;
        if (texels > c->radapt_need_texels)
        {
            HIPCHK(c, hipStreamSynchronize(c->stream));
            dfree(c->d_radapt_need); c->d_radapt_need = nullptr; c->radapt_need_texels = 0;
            HIPCHK(c, hipMalloc(&c->d_radapt_need, texels));
            c->radapt_need_texels = texels;
        }
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
            HIPCHK(c, hipEventRecord(c->ev_radapt[0], c->stream));
            launch_rays_gather(list, active, d_origins, d_dirs, d_keys, key_base, a.origins, a.dirs, a.keys, a.src, c->stream);
            HIPCHK(c, hipGetLastError());
            const int rc = trace_rays_passes(c, (int32_t)active, a.origins, a.dirs, max_depth, done, take, seed, 0u, rays_flags, a.keys,
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
            HIPCHK(c, hipEventRecord(c->ev_radapt[1], c->stream));
            HIPCHK(c, hipStreamSynchronize(c->stream));
            if (*c->h_radapt_total > active) return fail(c, PTK_ERR_HIP, "adaptive rays: the active list grew");
            float all = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&all, c->ev_radapt[0], c->ev_radapt[1]));
            float trace = 0.0f;
            for (int i = 0; i < c->rays_passes; i++)
            {
                float t = 0.0f;
                HIPCHK(c, hipEventElapsedTime(&t, c->ev_rays[i * 3], c->ev_rays[i * 3 + 1]));
                trace += t;
            }
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
    int rc = check_rays_adaptive_args(c, num_rays, origins, dirs, threshold, min_spp, step, max_spp, flags, sum, counts, &nothing);
    if (rc != PTK_OK) return rc;
    if (res) std::memset(res, 0, sizeof(*res));
    if (nothing) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    // origins | dirs | sum | sumsq | counts, staged for the length of the call
    const size_t n3 = (size_t)num_rays * 3, bytes = n3 * sizeof(float);
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, 4 * bytes + (size_t)num_rays * sizeof(uint32_t)));
    float *d_sum = d + 2 * n3, *d_sumsq = d + 3 * n3;
    uint32_t* d_counts = (uint32_t*)(d + 4 * n3);
    hipError_t e = hipMemcpyAsync(d, origins, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d + n3, dirs, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = rays_adaptive_on_stream(c, (uint32_t)num_rays, d, d + n3, nullptr, key_base, max_depth, threshold, min_spp, step, max_spp, seed, flags, d_sum,
                                     d_sumsq, d_counts, nullptr, 0, 0, res);
        if (rc == PTK_OK) e = hipMemcpyAsync(sum, d_sum, bytes, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && sumsq) e = hipMemcpyAsync(sumsq, d_sumsq, bytes, hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, (size_t)num_rays * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
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
    int rc = check_lightmap_adaptive_args(c, width, height, offset, threshold, min_spp, step, max_spp, flags, out, counts);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // uvs | out | counts | owner, staged for the length of the call
    const size_t texels = (size_t)width * height, n_uv = uvs ? (size_t)c->num_tris * 6 : 0;
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, (n_uv + texels * 5) * sizeof(float)));
    float* d_out = d + n_uv;
    uint32_t* d_counts = (uint32_t*)(d_out + texels * 3);
    int32_t* d_owner = owner ? (int32_t*)(d_counts + texels) : nullptr;
    hipError_t e = hipSuccess;
    if (n_uv) e = hipMemcpyAsync(d, uvs, n_uv * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = ptk_bake_lightmap_adaptive_device(c, width, height, n_uv ? d : nullptr, offset, max_depth, threshold, min_spp, step, max_spp, seed, key_base,
                                               flags, d_out, d_counts, d_owner, res);
        if (rc == PTK_OK) e = hipMemcpyAsync(out, d_out, texels * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess) e = hipMemcpyAsync(counts, d_counts, texels * sizeof(uint32_t), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && owner) e = hipMemcpyAsync(owner, d_owner, texels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_last_rays_adaptive_ms(ptk_ctx* c, float* total_ms, float* trace_ms, float* other_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (total_ms) *total_ms = c->radapt_ms[0];
    if (trace_ms) *trace_ms = c->radapt_ms[1];
    if (other_ms) *other_ms = c->radapt_ms[2];
    return PTK_OK;
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
    if (texels > c->bake_dilate_texels)
    {
        HIPCHK(c, hipStreamSynchronize(c->stream));
        dfree(c->d_bake_dilate); c->d_bake_dilate = nullptr; c->bake_dilate_texels = 0;
        HIPCHK(c, hipMalloc(&c->d_bake_dilate, texels * 4 * sizeof(float)));
        c->bake_dilate_texels = texels;
    }
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
    int rc = check_dilate_args(c, width, height, passes, image, owner);
    if (rc != PTK_OK || passes == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t texels = (size_t)width * height;
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, texels * 4 * sizeof(float)));
    int32_t* d_owner = (int32_t*)(d + texels * 3);
    hipError_t e = hipMemcpyAsync(d, image, texels * 3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_owner, owner, texels * sizeof(int32_t), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = ptk_lightmap_dilate_device(c, width, height, passes, d, d_owner);
        if (rc == PTK_OK) e = hipMemcpyAsync(image, d, texels * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess) e = hipMemcpyAsync(owner, d_owner, texels * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_last_bake_ms(ptk_ctx* c, float* coverage_ms, float* raygen_ms, float* trace_ms, float* scatter_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float t[4] = { 0.0f, 0.0f, 0.0f, 0.0f };
    if (c->bake_timed)
    {
        HIPCHK(c, hipEventSynchronize(c->ev_bake[5]));
        HIPCHK(c, hipEventElapsedTime(&t[0], c->ev_bake[0], c->ev_bake[1]));
        HIPCHK(c, hipEventElapsedTime(&t[1], c->ev_bake[2], c->ev_bake[3]));
        HIPCHK(c, hipEventElapsedTime(&t[2], c->ev_bake[3], c->ev_bake[4]));
        HIPCHK(c, hipEventElapsedTime(&t[3], c->ev_bake[4], c->ev_bake[5]));
    }
    if (coverage_ms) *coverage_ms = t[0];
    if (raygen_ms) *raygen_ms = t[1];
    if (trace_ms) *trace_ms = t[2];
    if (scatter_ms) *scatter_ms = t[3];
    return PTK_OK;
}

// ---- irradiance probe baking (ptk.h) -----------------------------------------------------------------------------------------
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

// brings a context-owned buffer of `floats_per` floats per element to at least `want` elements
static int grow_probe_buffer(ptk_ctx* c, float*& buf, size_t& have, size_t want, size_t floats_per)
{
    if (want <= have) return PTK_OK;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    dfree(buf); have = 0;
    HIPCHK(c, hipMalloc(&buf, want * floats_per * sizeof(float)));
    have = want;
    return PTK_OK;
}

// The bake proper, on the context's stream, every pointer into this GPU's memory: the basis table, then block by block of whole
// probes the rays and their trace into the block's slice of the radiance table, then the projection of the whole table.
static int probes_on_stream(ptk_ctx* c, int32_t num_probes, const float* d_positions, int32_t num_dirs, const float* d_dirs, int max_depth,
                            uint32_t first_sample, uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float weight, float* d_radiance,
                            float* d_coefs)
{
    c->probes_timed = false; c->probe_blocks_timed = 0;
    for (hipEvent_t& e : c->ev_probes)
        if (!e) HIPCHK(c, hipEventCreate(&e));
    const size_t D = (size_t)num_dirs, rays = (size_t)num_probes * D;
    // a block holds at most max(D, pass_bytes / 256) rays, in whole probes: the rays are never all materialised
    const size_t block_probes = std::min<size_t>((size_t)num_probes, std::max<size_t>(1, c->opt_pass_bytes / 256 / D));
    int rc = grow_probe_buffer(c, c->d_probe_basis, c->probe_basis_dirs, D, PTK_PROBE_COEFS);
    if (rc == PTK_OK) rc = grow_probe_buffer(c, c->d_probe_rays, c->probe_rays_cap, block_probes * D, 6);
    if (rc == PTK_OK && !d_radiance) rc = grow_probe_buffer(c, c->d_probe_table, c->probe_table_rays, rays, 3);
    if (rc != PTK_OK) return rc;
    float* const table = d_radiance ? d_radiance : c->d_probe_table;
    float* const origins = c->d_probe_rays, * const ray_dirs = origins + c->probe_rays_cap * 3;
    HIPCHK(c, hipEventRecord(c->ev_probes[0], c->stream));
    launch_probe_basis(d_dirs, num_dirs, c->d_probe_basis, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_probes[1], c->stream));
    for (size_t p0 = 0; p0 < (size_t)num_probes; p0 += block_probes)
    {
        const size_t np = std::min(block_probes, (size_t)num_probes - p0), ray0 = p0 * D;
        const int bi = c->probe_blocks_timed < ptk_ctx::kMaxTimedPasses ? c->probe_blocks_timed : -1;
        if (bi >= 0)
            while (c->ev_probe_blocks.size() < (size_t)(bi + 1) * 3)
            {
                hipEvent_t e = nullptr;
                HIPCHK(c, hipEventCreate(&e));
                c->ev_probe_blocks.push_back(e);
            }
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_blocks[bi * 3], c->stream));
        launch_probe_rays(d_positions + p0 * 3, d_dirs, (int)np, num_dirs, origins, ray_dirs, c->stream);
        HIPCHK(c, hipGetLastError());
        if (bi >= 0) HIPCHK(c, hipEventRecord(c->ev_probe_blocks[bi * 3 + 1], c->stream));
        // (contiguous keys: plain rays_kernel)
        rc = trace_rays_on_stream(c, (int32_t)(np * D), origins, ray_dirs, max_depth, first_sample, spp, seed, key_base + (uint32_t)ray0,
                                  (flags & PTK_PROBES_ACCUMULATE) ? PTK_RAYS_ACCUMULATE : 0u, table + ray0 * 3);
        if (rc != PTK_OK) return rc;
        if (bi >= 0) { HIPCHK(c, hipEventRecord(c->ev_probe_blocks[bi * 3 + 2], c->stream)); c->probe_blocks_timed = bi + 1; }
    }
    HIPCHK(c, hipEventRecord(c->ev_probes[2], c->stream));
    launch_probe_project(table, c->d_probe_basis, num_probes, num_dirs, weight, d_coefs, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_probes[3], c->stream));
    c->probes_timed = true;
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
    int rc = check_probes_args(c, num_probes, positions, num_dirs, dirs, flags, weight, radiance, coefs, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // positions | dirs | coefs | radiance (where the caller wants it), staged for the length of the call
    const size_t n_pos = (size_t)num_probes * 3, n_dir = (size_t)num_dirs * 3, n_coef = (size_t)num_probes * PTK_PROBE_COEFS * 3;
    const size_t n_rad = radiance ? (size_t)num_probes * (size_t)num_dirs * 3 : 0;
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, (n_pos + n_dir + n_coef + n_rad) * sizeof(float)));
    float* d_dirs = d + n_pos, * d_coefs = d_dirs + n_dir, * d_rad = radiance ? d_coefs + n_coef : nullptr;
    hipError_t e = hipMemcpyAsync(d, positions, n_pos * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_dirs, dirs, n_dir * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess && (flags & PTK_PROBES_ACCUMULATE)) e = hipMemcpyAsync(d_rad, radiance, n_rad * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        rc = probes_on_stream(c, num_probes, d, num_dirs, d_dirs, max_depth, first_sample, spp, seed, key_base, flags, weight, d_rad, d_coefs);
        if (rc == PTK_OK) e = hipMemcpyAsync(coefs, d_coefs, n_coef * sizeof(float), hipMemcpyDeviceToHost, c->stream);
        if (rc == PTK_OK && e == hipSuccess && radiance) e = hipMemcpyAsync(radiance, d_rad, n_rad * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    }
    const hipError_t es = hipStreamSynchronize(c->stream);      // (also on the way out of a failure: the staging buffer may be in use)
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (rc != PTK_OK) return rc;
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
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
    int rc = check_irradiance_args(c, dims, origin, spacing, coefs, num_points, points, normals, out, &g, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    // coefs | points | normals | out, staged for the length of the call
    const size_t n_coef = (size_t)dims[0] * dims[1] * dims[2] * PTK_PROBE_COEFS * 3, n3 = (size_t)num_points * 3;
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, (n_coef + 3 * n3) * sizeof(float)));
    float* d_points = d + n_coef, * d_normals = d_points + n3, * d_out = d_normals + n3;
    hipError_t e = hipMemcpyAsync(d, coefs, n_coef * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_points, points, n3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_normals, normals, n3 * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        launch_probe_irradiance(g, d, num_points, d_points, d_normals, d_out, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, n3 * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    const hipError_t es = hipStreamSynchronize(c->stream);
    if (e == hipSuccess) e = es;
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_last_probes_ms(ptk_ctx* c, float* raygen_ms, float* trace_ms, float* project_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    float gen = 0.0f, trace = 0.0f, project = 0.0f;
    if (c->probes_timed)
    {
        HIPCHK(c, hipEventSynchronize(c->ev_probes[3]));
        HIPCHK(c, hipEventElapsedTime(&gen, c->ev_probes[0], c->ev_probes[1]));         // (the basis table counts as ray generation)
        HIPCHK(c, hipEventElapsedTime(&project, c->ev_probes[2], c->ev_probes[3]));
        for (int i = 0; i < c->probe_blocks_timed; i++)
        {
            float a = 0.0f, b = 0.0f;
            HIPCHK(c, hipEventElapsedTime(&a, c->ev_probe_blocks[i * 3], c->ev_probe_blocks[i * 3 + 1]));
            HIPCHK(c, hipEventElapsedTime(&b, c->ev_probe_blocks[i * 3 + 1], c->ev_probe_blocks[i * 3 + 2]));
            gen += a; trace += b;
        }
    }
    if (raygen_ms) *raygen_ms = gen;
    if (trace_ms) *trace_ms = trace;
    if (project_ms) *project_ms = project;
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
    float* scratch = nullptr; uint8_t* scratch8 = nullptr;
    HIPCHK(c, hipMalloc(&scratch, px * 3 * sizeof(float)));
    if (hipMalloc(&scratch8, px * 3) != hipSuccess) { (void)hipFree(scratch); return fail(c, PTK_ERR_HIP, "hipMalloc"); }
    (void)hipMemsetAsync(scratch, 0, px * 3 * sizeof(float), c->stream);
    (void)hipMemsetAsync(c->d_stats, 0, 16 * sizeof(unsigned long long), c->stream);
    c->inputs_dirty = true;                      // ... and the zeroed counters
    rc = run_passes(c, first_sample, spp_count, seed, true, scratch, scratch8, nullptr, false);
    c->timed = false;
    unsigned long long h[16] = { 0 };
    hipError_t e = hipMemcpyAsync(h, c->d_stats, sizeof(h), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(scratch); (void)hipFree(scratch8);
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
    if (gen > __atomic_load_n(c->h_exit, __ATOMIC_RELAXED)) __atomic_store_n(c->h_exit, gen, __ATOMIC_RELAXED);
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

// ---- multi-GPU exchange step -------------------------------------------------------------------------------------
static int64_t packed_floats_of(int width, int height, int rank, int world)
{
    const int64_t tiles = (int64_t)((width + PTK_TILE - 1) / PTK_TILE) * ((height + PTK_TILE - 1) / PTK_TILE);
    const int64_t owned = tiles <= rank ? 0 : (tiles - rank + world - 1) / world;
    return owned * PTK_TILE * PTK_TILE * 3;
}

int64_t ptk_packed_floats(int width, int height, int rank, int world)
{
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world) return -1;
    return packed_floats_of(width, height, rank, world);
}

int ptk_packed_layout(int width, int height, int rank, int world, int64_t* src_index)
{
    if (width <= 0 || height <= 0 || world < 1 || rank < 0 || rank >= world || !src_index) return PTK_ERR_BAD_ARG;
    const int tiles_x = (width + PTK_TILE - 1) / PTK_TILE, num_tiles = tiles_x * ((height + PTK_TILE - 1) / PTK_TILE);
    int64_t k = 0;
    for (int tile = rank; tile < num_tiles; tile += world)
    {
        int tx, ty; tile_origin(tile, tiles_x, tx, ty);
        for (int p = 0; p < PTK_TILE * PTK_TILE; p++)
        {
            const int px = tx * PTK_TILE + (p & 15), py = ty * PTK_TILE + (p >> 4);
            const bool on = px < width && py < height;
            const int64_t a = ((int64_t)(height - 1 - py) * width + px) * 3;
            for (int ch = 0; ch < 3; ch++) src_index[k++] = on ? a + ch : -1;
        }
    }
    return PTK_OK;
}

int ptk_comm_unique_id(void* id_out)
{
    if (!id_out) return PTK_ERR_BAD_ARG;
    static_assert(sizeof(ncclUniqueId) == 128, "ptk.h promises 128 bytes");
    ncclUniqueId id;
    if (ncclGetUniqueId(&id) != ncclSuccess) return PTK_ERR_RCCL;
    std::memcpy(id_out, &id, sizeof(id));
    return PTK_OK;
}

int ptk_comm_init(ptk_ctx* c, const void* id_in, int rank, int world)
{
    if (!c || !id_in || world < 1 || world > PTK_MAX_RANKS || rank < 0 || rank >= world) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    // ncclCommInitRank blocks until EVERY rank of the group has called it: a rank that died on the way (or was never started)
    // would hang the others for good.  It runs on a helper thread and is waited for with a bound; on a timeout the caller gets an
    // error that names the rank and is expected to end the process (the helper thread is abandoned with its own state).
    struct InitJob { ncclComm_t comm = nullptr; ncclResult_t r = ncclSuccess; std::atomic<int> done{ 0 }; };
    auto job = std::make_shared<InitJob>();
    ncclUniqueId id;
    std::memcpy(&id, id_in, sizeof(id));
    const int device = c->device;
    std::thread([job, id, rank, world, device] {
        (void)hipSetDevice(device);
        job->r = ncclCommInitRank(&job->comm, world, id, rank);
        job->done.store(1);
    }).detach();
    const auto t0 = std::chrono::steady_clock::now();
    while (!job->done.load())
    {
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (waited > c->opt_comm_timeout_s)
        {
            char msg[256];
            std::snprintf(msg, sizeof(msg), "ncclCommInitRank: rank %d of %d (HIP device %d) waited %.0f s for the other ranks to join the communicator - "
                          "is every rank running, on a device of its own?", rank, world, device, waited);
            return fail(c, PTK_ERR_RCCL, msg);
        }
        std::this_thread::sleep_for(std::chrono::milliseconds(2));
    }
    if (job->r != ncclSuccess || !job->comm)
    {
        char msg[256];
        std::snprintf(msg, sizeof(msg), "ncclCommInitRank: rank %d of %d (HIP device %d): %s", rank, world, device, ncclGetErrorString(job->r));
        return fail(c, PTK_ERR_RCCL, msg);
    }
    c->comm = job->comm;
    c->comm_rank = rank; c->comm_world = world;
    c->rank = rank; c->world = world;            // the frame is split over the group (ptk_set_tile)
    return PTK_OK;
}

int ptk_comm_info(ptk_ctx* c, int* rank, int* world, int* comm_device, int* ctx_device)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (ctx_device) *ctx_device = c->device;
    if (!c->comm) return fail(c, PTK_ERR_BAD_ARG, "no communicator: call ptk_comm_init");
    int r = -1, w = 0, d = -1;
    if (ncclCommCount(c->comm, &w) != ncclSuccess || ncclCommUserRank(c->comm, &r) != ncclSuccess || ncclCommCuDevice(c->comm, &d) != ncclSuccess)
        return fail(c, PTK_ERR_RCCL, "ncclCommCount / ncclCommUserRank / ncclCommCuDevice failed");
    if (rank) *rank = r;
    if (world) *world = w;
    if (comm_device) *comm_device = d;
    return PTK_OK;
}

int ptk_comm_destroy(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    (void)hipSetDevice(c->device);
    if (c->xstream) (void)hipStreamSynchronize(c->xstream);
    if (c->comm) { (void)ncclCommDestroy(c->comm); c->comm = nullptr; }
    return PTK_OK;
}

// Packed gather.  Everything is queued on the context's exchange stream behind what the render stream holds now:
//   pack kernel (snapshot of the owned tiles; the render stream waits only for this) -> grouped ncclSend / ncclRecv
//   (each rank's 1/world of the image goes straight to the root over its own xGMI link) -> root: unpack kernel.
// The next ptk_render may be issued at once: its trace kernel does not touch the accumulator and overlaps the exchange.
int ptk_gather_accum(ptk_ctx* c, void* rccl_comm, int root)
{
    if (!c) return PTK_ERR_BAD_ARG;
    ncclComm_t comm = rccl_comm ? (ncclComm_t)rccl_comm : c->comm;
    if (!comm) return fail(c, PTK_ERR_BAD_ARG, "no communicator: pass one or call ptk_comm_init");
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int world = 0, rank = 0;
    if (ncclCommCount(comm, &world) != ncclSuccess || ncclCommUserRank(comm, &rank) != ncclSuccess)
        return fail(c, PTK_ERR_RCCL, "ncclCommCount / ncclCommUserRank failed");
    if (world != c->world || rank != c->rank) return fail(c, PTK_ERR_BAD_ARG, "communicator rank / size differ from ptk_set_tile");
    if (root < 0 || root >= world || world > PTK_MAX_RANKS) return fail(c, PTK_ERR_BAD_ARG, "bad root");
    const int W = c->width, H = c->height;
    long long bases[PTK_MAX_RANKS] = { 0 };
    size_t total = 0;
    for (int r = 0; r < world; r++) { bases[r] = (long long)total; total += (size_t)packed_floats_of(W, H, r, world); }
    const size_t mine = (size_t)packed_floats_of(W, H, rank, world);
    const size_t need = rank == root ? total : mine;
    if (need > c->packed_floats)
    {
        HIPCHK(c, hipStreamSynchronize(c->xstream));
        dfree(c->d_packed); c->packed_floats = 0;
        HIPCHK(c, hipMalloc(&c->d_packed, std::max<size_t>(need, 4) * sizeof(float)));
        c->packed_floats = need;
    }
    const size_t img = (size_t)W * H * 3;
    if (rank == root && img > c->gathered_floats)
    {
        HIPCHK(c, hipStreamSynchronize(c->xstream));
        dfree(c->d_gathered); c->gathered_floats = 0;
        HIPCHK(c, hipMalloc(&c->d_gathered, img * sizeof(float)));
        c->gathered_floats = img;
    }
    HIPCHK(c, hipEventRecord(c->ev_rendered, c->stream));
    HIPCHK(c, hipStreamWaitEvent(c->xstream, c->ev_rendered, 0));
    float* my_slot = c->d_packed + (rank == root ? bases[rank] : 0);
    launch_pack_owned(accum_ptr(c), my_slot, W, H, rank, world, c->xstream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipEventRecord(c->ev_packed, c->xstream));
    HIPCHK(c, hipStreamWaitEvent(c->stream, c->ev_packed, 0));      // the next accumulate_kernel may overwrite the accumulator from here on
    if (world > 1)
    {
        ncclResult_t r = ncclGroupStart();
        if (r == ncclSuccess)
        {
            if (rank == root)
            {
                for (int src = 0; src < world && r == ncclSuccess; src++)
                {
                    const size_t n = (size_t)packed_floats_of(W, H, src, world);
                    if (src != root && n) r = ncclRecv(c->d_packed + bases[src], n, ncclFloat, src, comm, c->xstream);
                }
            }
            else if (mine) r = ncclSend(my_slot, mine, ncclFloat, root, comm, c->xstream);
            ncclResult_t e = ncclGroupEnd();
            if (r == ncclSuccess) r = e;
        }
        if (r != ncclSuccess) return fail(c, PTK_ERR_RCCL, std::string("packed gather (ncclSend/ncclRecv): ") + ncclGetErrorString(r));
    }
    if (rank == root)
    {
        launch_unpack_all(c->d_packed, bases, c->d_gathered, W, H, world, c->xstream);
        HIPCHK(c, hipGetLastError());
        c->gathered_w = W; c->gathered_h = H;
    }
    HIPCHK(c, hipEventRecord(c->ev_gathered, c->xstream));
    c->gather_pending = true;
    c->gather_step++; c->gather_root = root;
    c->gather_bytes = (rank == root ? total - mine : mine) * sizeof(float);
    return PTK_OK;
}

// Bounded: polls the exchange's last event; when it has not fired within comm_timeout_s (a rank never entered its
// ptk_gather_accum, or died in it) the communicator is aborted - which releases the transfer kernel stuck on the exchange
// stream - and the caller gets PTK_ERR_RCCL with rank, step and the bytes that were expected.  An asynchronous RCCL error
// (a peer's process gone) ends the wait at once.  A failed exchange leaves no gathered image: d_gathered may hold part of this
// step's or the last step's image, so ptk_read_gathered and ptk_gathered_device_ptr refuse until a ptk_gather_accum succeeds.
int ptk_gather_wait(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->gather_pending) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const auto t0 = std::chrono::steady_clock::now();
    unsigned spins = 0;
    for (;;)
    {
        const hipError_t q = hipEventQuery(c->ev_gathered);
        if (q == hipSuccess) break;
        if (q != hipErrorNotReady)
        {
            c->gather_pending = false; c->gathered_w = c->gathered_h = 0;
            return fail(c, PTK_ERR_HIP, std::string("hipEventQuery (exchange): ") + hipGetErrorString(q));
        }
        (void)hipGetLastError();
        const double waited = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        ncclResult_t async = ncclSuccess;
        const bool poll_comm = c->comm && (++spins & 1023u) == 0;
        if (poll_comm && ncclCommGetAsyncError(c->comm, &async) != ncclSuccess) async = ncclSystemError;
        if (waited > c->opt_comm_timeout_s || (async != ncclSuccess && async != ncclInProgress))
        {
            char msg[384];
            std::snprintf(msg, sizeof(msg), "exchange step %llu on rank %d of %d (root %d) %s after %.1f s: %s %zu bytes%s",
                          c->gather_step, c->rank, c->world, c->gather_root,
                          async != ncclSuccess && async != ncclInProgress ? "failed" : "timed out", waited,
                          c->rank == c->gather_root ? "still expecting" : "still sending", c->gather_bytes,
                          async != ncclSuccess && async != ncclInProgress ? (std::string(" - RCCL: ") + ncclGetErrorString(async)).c_str() : " - a rank never joined this step");
            if (c->comm)
            {
                // the abort releases RCCL's own kernels, but it also waits for whatever else sits on the stream: it runs on a helper
                // thread and this call gives it one more timeout's worth (at most 5 s) before it returns regardless
                ncclComm_t doomed = c->comm;
                c->comm = nullptr;
                auto done = std::make_shared<std::atomic<bool>>(false);
                std::thread([doomed, done] { (void)ncclCommAbort(doomed); done->store(true); }).detach();
                const auto a0 = std::chrono::steady_clock::now();
                const double grace = std::min(c->opt_comm_timeout_s, 5.0);
                while (!done->load() && std::chrono::duration<double>(std::chrono::steady_clock::now() - a0).count() < grace)
                    std::this_thread::sleep_for(std::chrono::milliseconds(1));
            }
            c->gather_pending = false; c->gathered_w = c->gathered_h = 0;
            return fail(c, PTK_ERR_RCCL, msg);
        }
        if (waited > 0.002) std::this_thread::sleep_for(std::chrono::microseconds(200));
    }
    c->gather_pending = false;
    return PTK_OK;
}

// Test hook of the bounded waits: one lane that keeps the exchange stream busy for a fixed time (wall clock, 100 MHz), so that
// a single GPU can show what ptk_gather_wait does when an exchange step does not complete in time.  It always ends by itself.
__global__ void stall_kernel(unsigned long long ticks)
{
    const unsigned long long t0 = wall_clock64();
    while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(64);
}

int ptk_debug_stall_exchange(ptk_ctx* c, int milliseconds)
{
    if (!c || milliseconds < 0 || milliseconds > 10000) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    stall_kernel<<<1, 1, 0, c->xstream>>>((unsigned long long)milliseconds * 100000ull);
    HIPCHK(c, hipGetLastError());
    return PTK_OK;
}

int ptk_gathered_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    *dev_ptr = nullptr;
    if (bytes) *bytes = 0;
    if (!c->d_gathered || c->gathered_w == 0) return fail(c, PTK_ERR_BAD_ARG, "no gathered image on this rank (not the root, or ptk_gather_accum not called)");
    if (c->gathered_w != c->width || c->gathered_h != c->height)
        return fail(c, PTK_ERR_BAD_ARG, "the gathered image was combined for another resolution: call ptk_gather_accum again after ptk_set_frame");
    *dev_ptr = c->d_gathered;
    if (bytes) *bytes = (size_t)c->gathered_w * c->gathered_h * 3 * sizeof(float);
    return PTK_OK;
}

int ptk_read_gathered(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_gathered || c->gathered_w == 0) return fail(c, PTK_ERR_BAD_ARG, "no gathered image on this rank (not the root, or ptk_gather_accum not called)");
    if (c->gathered_w != c->width || c->gathered_h != c->height)
        return fail(c, PTK_ERR_BAD_ARG, "the gathered image was combined for another resolution: call ptk_gather_accum again after ptk_set_frame");
    int rc = ptk_gather_wait(c);
    if (rc != PTK_OK) return rc;
    HIPCHK(c, hipMemcpy(host_out, c->d_gathered, (size_t)c->width * c->height * 3 * sizeof(float), hipMemcpyDeviceToHost));
    return PTK_OK;
}

// parity probes of the two exchange kernels (one GPU can play every rank of a split)
int ptk_probe_pack(ptk_ctx* c, int rank, int world, float* host_out)
{
    if (!c || !host_out || world < 1 || world > PTK_MAX_RANKS || rank < 0 || rank >= world) return PTK_ERR_BAD_ARG;
    if (!accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)packed_floats_of(c->width, c->height, rank, world);
    if (n == 0) return PTK_OK;
    float* d = nullptr;
    HIPCHK(c, hipMalloc(&d, n * sizeof(float)));
    launch_pack_owned(accum_ptr(c), d, c->width, c->height, rank, world, c->stream);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(host_out, d, n * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_probe_unpack(ptk_ctx* c, int world, const float* host_packed, float* host_image)
{
    if (!c || !host_packed || !host_image || world < 1 || world > PTK_MAX_RANKS) return PTK_ERR_BAD_ARG;
    if (c->width <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    long long bases[PTK_MAX_RANKS] = { 0 };
    size_t total = 0;
    for (int r = 0; r < world; r++) { bases[r] = (long long)total; total += (size_t)packed_floats_of(c->width, c->height, r, world); }
    const size_t img = (size_t)c->width * c->height * 3;
    float *d = nullptr, *di = nullptr;
    HIPCHK(c, hipMalloc(&d, std::max<size_t>(total, 4) * sizeof(float)));
    if (hipMalloc(&di, img * sizeof(float)) != hipSuccess) { (void)hipFree(d); return fail(c, PTK_ERR_HIP, "hipMalloc"); }
    hipError_t e = hipMemcpyAsync(d, host_packed, total * sizeof(float), hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemsetAsync(di, 0xff, img * sizeof(float), c->stream);       // NaNs: every pixel must be written
    if (e == hipSuccess) { launch_unpack_all(d, bases, di, c->width, c->height, world, c->stream); e = hipGetLastError(); }
    if (e == hipSuccess) e = hipMemcpyAsync(host_image, di, img * sizeof(float), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d); (void)hipFree(di);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
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
    for (hipEvent_t e : c->klog_ev) (void)hipEventDestroy(e);
    c->klog_ev.clear(); c->klog_n = 0;
    for (int i = 0; i < 2 * capacity; i++)
    {
        hipEvent_t e = nullptr;
        HIPCHK(c, hipEventCreate(&e));
        c->klog_ev.push_back(e);
    }
    return PTK_OK;
}

int ptk_kernel_log_read(ptk_ctx* c, float* trace_ms, int max_entries, int* num_entries)
{
    if (!c || !num_entries || (max_entries > 0 && !trace_ms)) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    for (int k = 0; k < 2; k++) if (c->trace_stream[k]) HIPCHK(c, hipStreamSynchronize(c->trace_stream[k]));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    const int n = std::min(c->klog_n, max_entries);
    for (int i = 0; i < n; i++) HIPCHK(c, hipEventElapsedTime(&trace_ms[i], c->klog_ev[2 * i], c->klog_ev[2 * i + 1]));
    *num_entries = n;
    c->klog_n = 0;
    return PTK_OK;
}

int ptk_last_kernel_ms(ptk_ctx* c, float* trace_ms, float* accumulate_ms)
{
    if (!c || !trace_ms || !accumulate_ms) return PTK_ERR_BAD_ARG;
    *trace_ms = 0.0f; *accumulate_ms = 0.0f;
    if (!c->timed) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    int n = std::min(c->last_passes, (int)ptk_ctx::kMaxTimedPasses);
    for (int i = 0; i < n; i++)
    {
        float a = 0.0f, b = 0.0f;
        HIPCHK(c, hipEventSynchronize(c->ev[i][2]));
        HIPCHK(c, hipEventElapsedTime(&a, c->ev[i][0], c->ev[i][1]));
        HIPCHK(c, hipEventElapsedTime(&b, c->ev[i][1], c->ev[i][2]));
        *trace_ms += a; *accumulate_ms += b;
    }
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

int ptk_probe_hits(ptk_ctx* c, int n, const float* ro, const float* rd, int32_t* tri, float* tuv)
{
    if (!c || n < 0 || (n > 0 && (!ro || !rd || !tri || !tuv))) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float *d_ro = nullptr, *d_rd = nullptr, *d_tuv = nullptr; int32_t* d_tri = nullptr;
    size_t b3 = (size_t)n * 3 * sizeof(float);
    hipError_t e = hipMalloc(&d_ro, b3);
    if (e == hipSuccess) e = hipMalloc(&d_rd, b3);
    if (e == hipSuccess) e = hipMalloc(&d_tuv, b3);
    if (e == hipSuccess) e = hipMalloc(&d_tri, (size_t)n * sizeof(int32_t));
    if (e == hipSuccess) e = hipMemcpyAsync(d_ro, ro, b3, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(d_rd, rd, b3, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        ProbeParams p = {};
        p.nodes = c->d_nodes; p.tris = c->d_tris; p.shade = c->d_shade; p.mats = c->d_mats;
        p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.ro = d_ro; p.rd = d_rd; p.tri = d_tri; p.tuv = d_tuv;
        p.n = n; p.num_nodes = c->num_nodes; p.scene_bound = c->scene_bound;
        launch_probe(p, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(tri, d_tri, (size_t)n * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(tuv, d_tuv, b3, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_ro); (void)hipFree(d_rd); (void)hipFree(d_tuv); (void)hipFree(d_tri);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_probe_direct(ptk_ctx* c, int n, const float* pts, const float* normals, const float* diffuse, const float* tape3, float* out3)
{
    if (!c || n < 0 || (n > 0 && (!pts || !normals || !diffuse || !tape3 || !out3))) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t b3 = (size_t)n * 3 * sizeof(float);
    float* d[5] = { nullptr, nullptr, nullptr, nullptr, nullptr };
    const float* src[4] = { pts, normals, diffuse, tape3 };
    hipError_t e = hipSuccess;
    for (int k = 0; k < 5 && e == hipSuccess; k++) e = hipMalloc(&d[k], b3);
    for (int k = 0; k < 4 && e == hipSuccess; k++) e = hipMemcpyAsync(d[k], src[k], b3, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        ProbeParams p = {};
        p.nodes = c->d_nodes; p.tris = c->d_tris; p.shade = c->d_shade; p.mats = c->d_mats;
        p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.lights = c->d_lights; p.num_lights = c->num_lights;
        p.n = n; p.num_nodes = c->num_nodes; p.scene_bound = c->scene_bound;
        launch_probe_direct(p, d[0], d[1], d[2], d[3], d[4], c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out3, d[4], b3, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    for (int k = 0; k < 5; k++) (void)hipFree(d[k]);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_probe_math(ptk_ctx* c, int op, int n, const float* in, float* out)
{
    if (!c || op < 0 || op > 5 || n < 0 || (n > 0 && (!in || !out))) return PTK_ERR_BAD_ARG;
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    float *d_in = nullptr, *d_out = nullptr;
    const size_t bytes = (size_t)n * sizeof(float);
    hipError_t e = hipMalloc(&d_in, bytes);
    if (e == hipSuccess) e = hipMalloc(&d_out, bytes);
    if (e == hipSuccess) e = hipMemcpyAsync(d_in, in, bytes, hipMemcpyHostToDevice, c->stream);
    if (e == hipSuccess)
    {
        // the build the "contract" option selects for the trace kernels
        if (c->opt_contract == 1) fma::launch_probe_math(op, d_in, d_out, n, c->stream);
        else if (c->opt_contract == 2) fast::launch_probe_math(op, d_in, d_out, n, c->stream);
        else launch_probe_math(op, d_in, d_out, n, c->stream);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(out, d_out, bytes, hipMemcpyDeviceToHost, c->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
    (void)hipFree(d_in); (void)hipFree(d_out);
    if (e != hipSuccess) return fail(c, PTK_ERR_HIP, hipGetErrorString(e));
    return PTK_OK;
}

int ptk_probe_primary_dirs(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!c->d_primary) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    int rc = ensure_primary(c);
    if (rc != PTK_OK) return rc;
    size_t px = (size_t)c->width * c->height;
    std::vector<float4> tmp(px);
    HIPCHK(c, hipMemcpyAsync(tmp.data(), c->d_primary, px * sizeof(float4), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    for (size_t i = 0; i < px; i++) { host_out[i * 3] = tmp[i].x; host_out[i * 3 + 1] = tmp[i].y; host_out[i * 3 + 2] = tmp[i].z; }
    return PTK_OK;
}

}  // extern "C"
