// The context of the ptk C-ABI (include/ptk.h) and what the host API files ptk_api*.hip share.  Internal: not installed.
#pragma once
#include <hip/hip_runtime.h>

#include <atomic>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "ptk_features.h"
#include "ptk_own.h"

typedef struct ncclComm* ncclComm_t;             // rccl.h's own declaration, repeated so that only ptk_api_exchange.hip includes that header (which checks it)
namespace ptk { struct RaysBlock; }

struct ptk_ctx {
    // The streams come first: members go in reverse order of declaration, so every buffer and event below goes before the stream
    // that works on it (each stream is drained as it goes).  own_stream: `stream` is stream_own, not a caller's (ptk_set_stream)
    ptk::Stream stream_own, trace_stream[2], geo_stream, xstream, exit_stream;
    int device = 0;
    hipStream_t stream = nullptr;
    bool own_stream = false;
    std::string error;
    std::mutex err_mu;

    // scene (device)
    ptk::Buf<float4> d_flat_tris;       // <= 16 triangles: records in ascending triangle index for the FLAT kernel
    ptk::Buf<float4> d_nodes, d_tris, d_shade, d_mats, d_lights;
    ptk::Buf<int4> d_texinfo;
    ptk::Buf<uint32_t> d_texels;
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
    ptk::Buf<float> d_verts_res;                 // [num_tris][9]
    ptk::Buf<int32_t> d_tri_pos;                 // triangle -> position of its record in the leaf order
    ptk::Buf<int32_t> d_level_nodes;             // node indices sorted by level, the root's level first
    std::vector<int> level_start;                // [levels + 1] offsets into d_level_nodes
    ptk::Buf<double> d_refit_partial;            // one partial SAH sum per 256 nodes
    ptk::Buf<float4> d_refit_side;               // per node: union box + summed child half-area (ptk_refit.h)
    ptk::Buf<float> d_geo_stage;                 // staged verts | normals | tbn of the update in progress
    ptk::Buf<uint32_t> d_geo_red;                // GEO_RED_WORDS of the bounds reduction, then one double: the SAH cost
    ptk::Pinned<uint32_t> h_geo_red;             // page-locked target of its read-back
    // geo_stream: staging copies and the bounds reduction: the one host wait of an update is for this stream alone
    // events of the newest update: [0] [1] around staging + bounds on geo_stream; [2] before the repack, [3] behind it, [4] behind
    // the refit on the context's stream ([4] also orders the next update's staging behind this one's kernels)
    // (all five made by ptk_create; timed: an update has recorded them)
    ptk::Timer<5> ev_geo_t;
    bool lights_stale = false;                   // h_lights lacks the vertices an update moved
    uint32_t geo_updates = 0;
    double sah_built = 0.0, sah_now = 0.0; bool sah_now_pending = false;
    float bvh_pad = 0.0f;                        // the builders' box padding for the current scene extent
    bool scene_plain = false;           // plain_tables() of the staged scene: kept current by ptk_upload_scene and ptk_update_materials
    int opt_plain_kernel = 1;           // 0: plain scenes launch the generic FLAT kernel too (tests, A/B runs)
    bool scene_lambert = false;         // lambert_tables() of the staged scene (plain and no reflectiveness > 0): kept current with scene_plain
    int opt_lambert_kernel = 1;         // 0: Lambert scenes launch the PLAIN kernel's generic level (tests, A/B runs)
    int opt_flat_rect_pairs = 1;        // 1: exact PLAIN scenes run the pair-pass unit's kernels, which test the list's prefix of fan-split rectangles pair by pair
    int opt_flat_cycle = 1;             // 1 (with opt_flat_rect_pairs): ... from the cycle unit, the same pass and shade block in a fixed cycle with a scalar unit deal
    int opt_flat_zero_classes = 1;      // 0: the exact PLAIN pass treats every flat record as class 0 (the class table's first word is kept zero)
    int last_trace_variant = PTK_TRACE_NONE;     // of the newest trace launch (ptk_trace_variant)
    int last_trace_unit = PTK_UNIT_NONE;         // ... which unit's kernel it was, for the exact PLAIN kernels (ptk_trace_unit)
    bool last_trace_lambert = false;    // ... and whether it ran the LAMBERT level of the PLAIN kernel (ptk_trace_is_lambert)

    // camera (host copies, already normalised / clamped like the reference setters)
    float cam_pos[3] = { 0, 0, 0 }, cam_dir[3] = { 0, 0, 1 }, cam_up[3] = { 0, 1, 0 };
    float focal = 0.1f, fovy = 90.0f, focal_dist = 5.0f, aperture = 0.0f;   // pathtracer.cpp:17-22
    float cam_right[3] = { 1, 0, 0 };
    bool primary_dirty = true;

    // frame
    int width = 0, height = 0, max_depth = 3;                                 // pathtracer.cpp:15
    ptk::Buf<float4> d_primary;
    ptk::Buf<float4> d_primary_hit;   // primary-visibility cache (pinhole, no opacity textures)
    ptk::Buf<float4> d_primary_rd;    // ... and the camera ray's direction per pixel
    ptk::Buf<uint2> d_pixel_rng;      // per pixel: (pixel key, PCG increment) for pixel_rng_seed
    uint64_t pixel_rng_seed = 0; bool pixel_rng_valid = false;
    bool primary_hit_dirty = true, scene_has_opacity = false;
    int opt_primary_cache = 1;
    int opt_flat_shade_w = 8, opt_flat_gen_w = 64;
    int opt_flat = 1;                    // scenes of <= PTK_FLAT_MAX triangles: no BVH walk (trace_kernel<.., FLAT>)
    ptk::Buf<float> d_accum;         // owned accumulator
    float* d_accum_bound = nullptr;  // caller-owned accumulator (ptk_bind_accum) or null
    ptk::Buf<uint8_t> d_rgb8;
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
    ptk::Buf<uint32_t> d_exit;
    ptk::Pinned<uint32_t> h_exit;                // page-locked source of the copy that writes d_exit (ptk_request_exit)
    // exit_stream: high priority, nothing else on it: the copy of the Exit() word never waits behind a render
    std::mutex exit_mu;                          // (Exit() may come from several threads: the source word never goes back)
    ptk::Buf<unsigned long long> d_stats;
    ptk::Buf<unsigned> d_queues;                 // item queues of trace_kernel's persistent waves
    // live-quadrant list (which 8x8 quadrants of the owned tiles have pixels to trace) and what it was built for
    ptk::Buf<unsigned long long> d_live_mask;
    ptk::Buf<unsigned> d_live_list;              // [capacity] entries + 1 word: the count
    int live_capacity = 0;
    unsigned long long hit_generation = 0;       // bumped whenever the primary-hit cache is recomputed
    struct LiveKey { int width, height, rank, world, cached; unsigned long long generation; } live_key = { 0, 0, -1, 0, -1, 0 };
    int resident_waves = 4096;                   // one-wave workgroups the device holds at once (CUs x 16)

    // adaptive render (ptk_render_adaptive): allocated by the first one, freed by ptk_set_frame with another resolution
    ptk::Buf<uint32_t> d_counts;                 // [H][W] samples per pixel, rows bottom-up
    ptk::Buf<float> d_moments;                   // [H][W][3] sums of squared samples (S2)
    ptk::Buf<unsigned long long> d_adapt_active, d_adapt_traced;                  // per quadrant of the frame: active set, active & live
    ptk::Buf<unsigned> d_adapt_list;             // [adapt_capacity] entries + 1 word: the count (the traced mask's quadrants)
    ptk::Buf<unsigned long long> d_adapt_stats;  // [0] pixel samples, [1] largest count, [2] low word: active pixels after the last test
    int adapt_capacity = 0;                      // quadrants the buffers hold (every quadrant of the frame: any tile split fits)
    ptk::Pinned<unsigned> h_adapt_count;         // page-locked [2]: the active count of rounds r and r + 1, read one round behind
    ptk::Event ev_adapt[2];
    bool adaptive_accum = false;                 // the accumulator holds an adaptive render: per-pixel counts, no single sample count

    // first-hit feature planes (ptk_render_features): allocated on first use, each for the frame feat_w x feat_h
    ptk::Buf<void> d_feat[ptk::NUM_FEATURES];
    int feat_w = 0, feat_h = 0;                  // the frame the planes were allocated for and last rendered at
    uint32_t feat_mask = 0;                      // planes the last ptk_render_features wrote

    // radiance along caller-supplied rays (ptk_trace_rays): its own sample buffer between rays_kernel and rays_fold_kernel - renders
    // may still be in flight on the internal streams with theirs -, grown to the largest pass so far; the item counter and
    // parameter block of a launch; three events per pass of the last call: before rays_kernel, behind it, behind the fold
    ptk::Buf<float4> d_rays_samples;             // (capacity in bytes)
    ptk::Buf<ptk::RaysBlock> d_rays_block;
    ptk::PassTimer ev_rays;                      // (at most kMaxTimedPasses passes of the last call)

    // lightmap baking (ptk_bake_lightmap), each grown to the largest bake so far: the owner plane (4 B per texel) with the covered
    // count per block of 256 texels behind it; the compacted rays of the covered texels (origins | dirs | sums | keys | texel
    // index, 44 B each); the second image + owner plane of ptk_lightmap_dilate (16 B per texel); the covered count's page-locked
    // read-back word; six events of the last bake: start, behind coverage + count, before and behind the ray generator, behind the
    // trace, behind the scatter
    ptk::Buf<int> d_bake_plane;
    ptk::Buf<float> d_bake_compact, d_bake_dilate;
    ptk::Pinned<uint32_t> h_bake_total;
    ptk::Timer<6> ev_bake;

    // adaptive ray queries and lightmap bakes (ptk_trace_rays_adaptive, ptk_bake_lightmap_adaptive), each grown to the largest call
    // so far: per ray 56 B - the round's compacted origins | dirs (24 B), keys, source indices, the next active list and the keep
    // flags (4 B each), S2 and the counts where the caller's arrays do not hold them (12 + 4 B) - with a count per 256 rays and the
    // total behind them; a lightmap's need plane (1 B per texel); the total's page-locked read-back word; two events around the
    // GPU work of a round; the last call's times (ptk_last_rays_adaptive_ms)
    ptk::Buf<float> d_radapt;
    ptk::Buf<uint8_t> d_radapt_need;
    ptk::Pinned<uint32_t> h_radapt_total;
    ptk::Timer<2> ev_radapt;
    float radapt_ms[3] = { 0.0f, 0.0f, 0.0f };   // host wall time of the round loop; rays_keyed_kernel; the other kernels of the rounds

    // irradiance probe baking (ptk_bake_probes), each grown to the largest call so far: the basis table (36 B per direction), one
    // block of rays (origins | dirs, 24 B each) and, while the caller passes no table, the radiance table (12 B per ray); four
    // events of the last bake - around the basis table, around the projection - and three per block of probes (the first
    // kMaxTimedPasses of them): before the ray generator, behind it, behind the trace
    ptk::Buf<float> d_probe_basis, d_probe_rays, d_probe_table;
    ptk::Timer<4> ev_probes;
    ptk::PassTimer ev_probe_blocks;

    // probe visibility (ptk_bake_probe_visibility): the depth table while the caller passes none (4 B per ray, grown to the largest
    // call so far; the rays of a block are d_probe_rays); two events of the last call around the moments kernel and three per block
    // of probes as above: before the ray generator, behind it, behind hits_kernel
    ptk::Buf<float> d_probe_depth;
    ptk::Timer<2> ev_probe_vis;
    ptk::PassTimer ev_probe_vis_blocks;

    // closest-hit and occlusion queries (ptk_intersect_rays, ptk_occluded_rays): two events around the last call's kernel, made
    // by the first call
    ptk::Timer<2> ev_hits;

    // closest-point queries (ptk_closest_points): two events around the last call's kernel, made by the first call; the two
    // counters of ptk_closest_stats, made by its first call
    ptk::Timer<2> ev_closest;
    ptk::Buf<unsigned long long> d_closest_stats;

    // crossing counts, containment and signed distance (ptk_crossings_rays, ptk_contains_points, ptk_signed_distance): two events
    // around the last call's kernels, made by the first call
    ptk::Timer<2> ev_crossings;

    // ordered multi-hit queries (ptk_multihit_rays): two events around the last call's kernel, made by the first call
    ptk::Timer<2> ev_multihit;

    // K-nearest triangle queries (ptk_nearest_triangles): two events around the last call's kernel, made by the first call; the two
    // counters of ptk_nearest_stats, made by its first call
    ptk::Timer<2> ev_nearest;
    ptk::Buf<unsigned long long> d_nearest_stats;

    // overlap queries (ptk_overlap_boxes, ptk_overlap_spheres): two events around the last call's kernel, made by the first call;
    // the four counters of ptk_overlap_stats, made by its first call
    ptk::Timer<2> ev_overlap;
    ptk::Buf<unsigned long long> d_overlap_stats;

    // surface sampling (ptk_sample_surface, ptk_surface_weights).  The table, 8 B per triangle - the inclusive sums of the quantised
    // weights - with the 8 KiB coarse table behind it; the caller's weights (4 B per triangle) while some are set; the workgroup
    // sums of the scan; the reduction block of the build.  All made by the first use for a scene and freed with it.  surf_valid: the
    // table holds the resident vertices and the weights as they are (ptk_update_geometry and ptk_surface_weights clear it).  What
    // ptk_surface_info reports: exponent and max from the build, total and drawable read back once asked for.  Two timers: around
    // the last build (timed: the last call built the table), around the last call's kernel
    ptk::Buf<uint64_t> d_surf_table, d_surf_sums;
    ptk::Buf<float> d_surf_weights;
    ptk::Buf<uint32_t> d_surf_red;
    bool surf_valid = false, surf_info_pending = false;
    uint64_t surf_total = 0;
    int surf_exponent = 0, surf_drawable = 0;
    float surf_max = 0.0f;
    ptk::Timer<2> ev_surf_table, ev_surface;
    int opt_surface_variant = 1;                 // surface_sample_kernel's variant (ptk_surface.h; 1: the coarse table in LDS): speed only

    // surface attribute queries (ptk_surface_attributes): two events around the last call's kernel, made by the first call
    ptk::Timer<2> ev_attributes;

    // a-trous denoiser (ptk_denoise_planes, ptk_denoise_frame): the four packed float4 images of a call (64 B per pixel, grown to the
    // largest call so far); the denoised frame [H][W][3], made by the first ptk_denoise_frame, freed with the feature planes, and
    // the resolution it was last written at; four events of the last call: before the pack, behind it, behind the filter, behind
    // the unpack
    ptk::Buf<float4> d_denoise;
    ptk::Buf<float> d_denoised;
    int den_w = 0, den_h = 0;
    ptk::Timer<4> ev_denoise;

    // temporal reprojection (ptk_reproject_planes, ptk_temporal_frame).  The frame entry's buffer, 112 B per pixel, made by the first
    // ptk_temporal_frame at a resolution and freed with the feature planes: two histories of three float4 images each, then the
    // unpacked result, colour [H][W][3] and count [H][W].  temporal_set names the history the last call wrote, temporal_view the view
    // stored with it; temporal_w x temporal_h is the resolution of that call (0: none yet).  The planes entries pack the caller's
    // history into d_temporal_pack (48 B per pixel, grown to the largest call so far).  Three events of the last call: before the
    // pack, behind it, behind the kernel
    ptk::Buf<float4> d_temporal;
    int temporal_w = 0, temporal_h = 0, temporal_set = 0;
    ptk_view temporal_view = {};
    ptk::Buf<float4> d_temporal_pack;
    ptk::Timer<3> ev_temporal;

    // moving geometry under temporal reprojection (ptk_geometry_snapshot, ptk_render_motion, ptk_temporal_frame_moving).  The snapshot
    // of d_verts_res, 36 B per triangle, made by the first ptk_geometry_snapshot of a scene and freed with it; have_snapshot: it
    // holds one.  The three planes of ptk_render_motion in one buffer, 32 B per pixel - previous position [H][W][3] | previous
    // normal [H][W][3] | motion [H][W][2] -, made by the first call at a resolution and freed with the feature planes; motion_w x
    // motion_h is the resolution of the last call (0: none yet).  Two events of the last call around motion_kernel; timed 1:
    // they are set, 2: and ev_temporal holds the reprojection kernel that followed
    ptk::Buf<float> d_verts_prev;
    bool have_snapshot = false;
    ptk::Buf<float> d_motion;
    int motion_w = 0, motion_h = 0;
    ptk::Timer<2> ev_motion;

    // temporal moments and variance (ptk_temporal_frame_moments, ptk_temporal_variance, ptk_denoise_temporal).  The frame entry's
    // buffer, 52 B per pixel, made by the first moments call at a resolution and freed with the feature planes: the fourth packed
    // image of the two history sets (m1, m2, count, the frame's own count), then the unpacked moments [H][W][2], the raw and the
    // final variance [H][W] each and ptk_denoise_temporal's mask [H][W].  temporal_moments: the last frame call at temporal_w x
    // temporal_h was a moments call, so set temporal_set holds moments; temporal_variance: ptk_temporal_variance has run since.
    // The planes entries pack into d_variance_pack (52 B per pixel with the raw plane, grown to the largest call so far);
    // ptk_reproject_moments packs the history's moments into d_temporal_pack_mm (16 B per pixel, likewise).  Three events of the
    // last variance call: before variance_kernel, behind it, behind the prefilter
    ptk::Buf<float4> d_temporal_mm;
    bool temporal_moments = false, temporal_variance = false;
    ptk::Buf<float4> d_variance_pack, d_temporal_pack_mm;
    ptk::Timer<3> ev_variance;                   // timed 2: the last call ran the prefilter too

    // display transform (ptk_display_planes, ptk_display_frame).  The luminance histogram, 2048 uint32 (8 KB), with the 32 B exposure
    // state behind it: made and zeroed by the first call, the histogram cleared by each call's exposure step behind itself.  The
    // frame entry's 8-bit image [H][W][3], made by the first ptk_display_frame at a resolution, freed with the feature planes, and
    // the resolution it was last written at.  Four events of the last call: before the meter, behind it, behind the exposure step,
    // behind the apply kernel
    ptk::Buf<uint32_t> d_display_hist;
    ptk::Buf<uint8_t> d_display;
    int disp_w = 0, disp_h = 0;
    ptk::Timer<4> ev_display;

    // guided upsampling (ptk_render_guides, ptk_upsample_planes, ptk_upsample_frame).  The guide planes at a resolution of their
    // own with their primary-direction table (16 B per guide pixel), each grown to the largest call so far and freed with the
    // feature planes; guide_w x guide_h, guide_mask and guide_view describe the last ptk_render_guides (0: none yet).  The packed
    // low image of a call, three or four float4 images (48 or 64 B per low pixel), grown likewise.  The frame entry's result, colour
    // [H][W][3] then class [H][W] (16 B per high pixel), grown likewise and freed with the guide planes; ups_w x ups_h is the size
    // it was last written at.  Three events of the last upsample call: before the pack, behind it, behind upsample_kernel
    ptk::Buf<void> d_guide[ptk::NUM_FEATURES];   // (capacity in pixels)
    ptk::Buf<float4> d_guide_primary;
    int guide_w = 0, guide_h = 0;
    uint32_t guide_mask = 0;
    ptk_view guide_view = {};
    ptk::Buf<float4> d_upsample_pack;
    ptk::Buf<float> d_upsampled;
    int ups_w = 0, ups_h = 0;
    ptk::Timer<3> ev_upsample;

    // sample buffer between trace_kernel and accumulate_kernel (grown on demand, never shrunk)
    // Two sample buffers / queue blocks / trace streams: the trace kernel of pass k+1 runs on the other stream and
    // overlaps the tail of pass k's (a launch ends with the few waves that hold its longest paths - Russian roulette
    // lets one path in tens of millions live for 60+ bounces, ~0.4 ms with the rest of the chip idle) and pass k's
    // accumulate kernel.  The accumulate kernels stay on the context's stream, in order, each behind its trace kernel,
    // so everything the caller orders after ptk_render on that stream still sees the finished batch.
    ptk::Buf<float4> d_samples;                  // (non-overlapped path; capacities in bytes)
    ptk::Buf<float4> d_samples2[2];
    ptk::Buf<unsigned> d_queues2[2];
    ptk::Event ev_trace_done[2], ev_acc_done[2], ev_inputs;      // ordering events: no timing
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
    // xstream: high priority: its kernels and the collective take wave slots ahead of queued trace waves
    ptk::Event ev_rendered, ev_packed, ev_gathered;            // ordering events: no timing
    ptk::Buf<float> d_packed;                    // non-root: this rank's packed tiles; root: every rank's, back to back
    ptk::Buf<float> d_gathered;                  // root: the combined image (W*H*3, rows bottom-up)
    int gathered_w = 0, gathered_h = 0;          // the frame the last ptk_gather_accum combined (ptk_read_gathered refuses any other)
    bool gather_pending = false;
    // every wait of the exchange step is bounded (ptk_set_option "comm_timeout_s"): a rank that never arrives must end the run with
    // an error that names it, not hang the node (the first real 8-GPU run is the driver's, not ours)
    double opt_comm_timeout_s = 120.0;
    unsigned long long gather_step = 0;          // exchanges queued so far (named in the timeout message)
    size_t gather_bytes = 0;                     // bytes the last exchange moves on this rank (root: what it receives)
    int gather_root = 0;

    // log of every trace launch's duration (ptk_kernel_log): event pairs on the launch's own stream
    std::vector<ptk::Event> klog_ev;             // 2 x capacity
    int klog_n = 0;
    static constexpr int kMaxTimedPasses = 64;
    ptk::PassTimer ev;                           // per pass: before trace, after trace, after accumulate; all made by ptk_create
    int last_passes = 0;
    int last_launches = 0;
};

namespace ptk {
inline int fail(ptk_ctx* c, int code, const std::string& msg)
{
    if (c) { std::lock_guard<std::mutex> g(c->err_mu); c->error = msg; }
    return code;
}
#define HIPCHK(c, expr)                                                                              \
    do {                                                                                             \
        hipError_t e_ = (expr);                                                                      \
        if (e_ != hipSuccess)                                                                        \
            return ptk::fail(c, PTK_ERR_HIP, std::string(#expr) + ": " + hipGetErrorString(e_));     \
    } while (0)

inline float* accum_ptr(ptk_ctx* c) { return c->d_accum_bound ? c->d_accum_bound : c->d_accum; }

// ---- the owners' members that need the context (ptk_own.h)
template <class T>
int Buf<T>::alloc_bytes(ptk_ctx* c, size_t bytes, size_t n)
{
    HIPCHK(c, try_alloc(bytes, n));
    return PTK_OK;
}
template <class T>
int Buf<T>::grow(ptk_ctx* c, size_t want, size_t bytes_per, size_t extra, hipStream_t user)
{
    if (want <= cap) return PTK_OK;
    HIPCHK(c, hipStreamSynchronize(user ? user : c->stream));
    return alloc_bytes(c, want * bytes_per + extra, want);
}
inline int event_ms(ptk_ctx* c, hipEvent_t a, hipEvent_t b, float* ms)
{
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipEventSynchronize(b));
    HIPCHK(c, hipEventElapsedTime(ms, a, b));
    return PTK_OK;
}
template <int N>
int Timer<N>::mark(ptk_ctx* c, int k, hipStream_t s)
{
    HIPCHK(c, ev[k].create());
    HIPCHK(c, hipEventRecord(ev[k], s));
    return PTK_OK;
}
inline int PassTimer::reserve(ptk_ctx* c, int n)
{
    while (ev.size() < (size_t)n * 3) { Event e; HIPCHK(c, e.create()); ev.push_back(std::move(e)); }
    return PTK_OK;
}
inline int PassTimer::add(ptk_ctx* c, int i, float* first, float* second)
{
    float a = 0.0f, b = 0.0f;
    if (second) { if (const int rc = event_ms(c, at(i, 1), at(i, 2), &b); rc != PTK_OK) return rc; *second += b; }
    if (first) { if (const int rc = event_ms(c, at(i, 0), at(i, 1), &a); rc != PTK_OK) return rc; *first += a; }
    return PTK_OK;
}

// the frame entries' temporal buffer cut up (ptk_api_temporal.hip writes it, ptk_api_variance.hip reads it):
// history set 0 | history set 1 | colour | count ...
inline bool have_temporal(const ptk_ctx* c) { return c->d_temporal && c->temporal_w == c->width && c->temporal_h == c->height && c->temporal_w > 0; }
inline float* temporal_color(const ptk_ctx* c, size_t px) { return (float*)(c->d_temporal + 6 * px); }
inline float* temporal_count(const ptk_ctx* c, size_t px) { return temporal_color(c, px) + 3 * px; }
// ... and the moments buffer: mm of set 0 | mm of set 1 | moments | raw variance | variance | mask
inline bool have_temporal_moments(const ptk_ctx* c) { return have_temporal(c) && c->d_temporal_mm && c->temporal_moments; }
inline float4* temporal_mm(const ptk_ctx* c, size_t px, int set) { return c->d_temporal_mm + (size_t)set * px; }
inline float* temporal_moments_plane(const ptk_ctx* c, size_t px) { return (float*)(c->d_temporal_mm + 2 * px); }
inline float* temporal_raw_variance(const ptk_ctx* c, size_t px) { return temporal_moments_plane(c, px) + 2 * px; }
inline float* temporal_variance_plane(const ptk_ctx* c, size_t px) { return temporal_moments_plane(c, px) + 3 * px; }
inline int32_t* temporal_mask_plane(const ptk_ctx* c, size_t px) { return (int32_t*)(temporal_moments_plane(c, px) + 4 * px); }
constexpr size_t kTemporalMomentsBytes = 2 * sizeof(float4) + 5 * sizeof(float);      // per pixel

// ---- internals that cross the files: ptk_api.hip ...
void fill_params(ptk_ctx* c, RenderParams& p, uint32_t first, uint32_t spp, uint64_t seed);
int ensure_primary(ptk_ctx* c);
void frame_view(ptk_ctx* c, PrimaryParams& pp);       // frame_setup's arithmetic for the current camera and frame: host only
void frame_view_at(const ptk_ctx* c, int width, int height, PrimaryParams& pp);      // ... at another size; pp.primary is left null
// ... ptk_api_rays.hip: a ray query on the context's stream; the checks and the round loop the adaptive lightmap bake shares with
// the adaptive ray query, and the context's adaptive buffer cut up for its capacity ...
int trace_rays_on_stream(ptk_ctx* c, int32_t num_rays, const float* d_origins, const float* d_dirs, int max_depth, uint32_t first_sample,
                         uint32_t spp, uint64_t seed, uint32_t key_base, uint32_t flags, float* d_out, const uint32_t* d_keys = nullptr);
int check_adaptive_args(ptk_ctx* c, const char* who, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp);
// ... the argument checks of the ray, point and surface query entries (see there)
int check_query_args(ptk_ctx* c, const char* who, const char* count_word, int32_t num, const void* a, const void* b, bool have_out, bool* nothing,
                     const char* also = nullptr);
// ... and what the one-kernel query entries share beyond them.  The body of a ptk_last_*_ms over two events around the kernel:
inline int last_ms(ptk_ctx* c, Timer<2> ptk_ctx::*ev, float* ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t = 0.0f;
    const int rc = (c->*ev).elapsed(c, 0, 1, &t);
    if (ms) *ms = t;
    return rc;
}
// The scene half of a point or region query's parameter block (ClosestParams, NearestParams, OverlapParams)
template <class P>
void query_scene(const ptk_ctx* c, P& h)
{
    h.nodes = c->d_nodes; h.tris = c->d_tris; h.num_nodes = c->num_nodes; h.scene_bound = c->scene_bound;
}
// Such a query proper, on the context's stream, every pointer into this GPU's memory: h holds the queries and the outputs, the scene
// half is filled in here.  One kernel between the two events; a scene without triangles has no tree to walk and gets its misses
// from fills() instead, untimed.
template <class P, class FILLS>
int query_on_stream(ptk_ctx* c, Timer<2>& ev, P& h, void (*launch)(const P&, hipStream_t), FILLS fills)
{
    ev.begin();
    if (c->num_nodes == 0) return fills();
    query_scene(c, h);
    if (const int rc = ev.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch(h, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rc = ev.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    ev.done();
    return PTK_OK;
}
// ... and its counting call (ptk_*_stats): the N counters, made by the first call, cleared, added to by the kernel's STATS variant
// and read back - one host wait.  got stays as it is when there are no queries (nothing) or no tree.
template <class P, int N>
int query_stats(ptk_ctx* c, bool nothing, Buf<unsigned long long>& d_stats, P& h, void (*launch)(const P&, hipStream_t), unsigned long long (&got)[N])
{
    if (nothing || c->num_nodes == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (!d_stats) HIPCHK(c, hipMalloc(&d_stats.p, sizeof(got)));
    HIPCHK(c, hipMemsetAsync(d_stats, 0, sizeof(got), c->stream));
    h.stats = d_stats;
    query_scene(c, h);
    launch(h, c->stream);
    HIPCHK(c, hipGetLastError());
    HIPCHK(c, hipMemcpyAsync(got, d_stats, sizeof(got), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}
struct RaysAdaptiveBuffers {
    float *origins, *dirs, *s2;
    uint32_t *keys, *src, *list, *keep, *counts, *block_counts, *total;
};
RaysAdaptiveBuffers radapt_buffers(ptk_ctx* c);
int rays_adaptive_on_stream(ptk_ctx* c, uint32_t n, const float* d_origins, const float* d_dirs, const uint32_t* d_keys, uint32_t key_base,
                            int max_depth, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, uint64_t seed, uint32_t rays_flags,
                            float* s1, float* s2, uint32_t* counts, const uint32_t* texel, int width, int height, ptk_rays_adaptive_result* res);
// ... ptk_api_denoise.hip: the parameter check and the planes call proper of ptk_denoise_planes_device, for ptk_denoise_temporal ...
int check_denoise_params(ptk_ctx* c, const char* who, const ptk_denoise_params* p);
int denoise_planes_on_stream(ptk_ctx* c, int width, int height, const float* d_color, const int32_t* d_mask, const float* d_normal,
                             const float* d_position, const float* d_albedo, const float* d_variance, const ptk_denoise_params& p,
                             float* d_out_color, float* d_out_variance);
// ... ptk_api_surface.hip: frees the sampling table and the weights of the scene that goes; builds the table where it is missing or
// stale, on the context's stream (one host wait, for the eight bytes of the build's reduction)
void surface_release(ptk_ctx* c);
int ensure_surface_table(ptk_ctx* c);
// ... ptk_api_exchange.hip: destroys the context's own communicator, if there is one
void comm_release(ptk_ctx* c);

}  // namespace ptk
