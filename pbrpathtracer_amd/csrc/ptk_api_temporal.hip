// Host side of the ptk C-ABI: temporal reprojection for image planes and for the context's frame (ptk.h ptk_get_view,
// ptk_reproject_planes, ptk_temporal_frame), and its moving-geometry mode with the motion planes (ptk.h
// ptk_geometry_snapshot, ptk_render_motion, ptk_reproject_planes_moving, ptk_temporal_frame_moving), and the
// moments of demodulated luminance carried through either (ptk.h ptk_reproject_moments, ptk_temporal_frame_moments).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ptk_ctx.h"
#include "ptk_motion.h"
#include "ptk_stage.h"
#include "ptk_temporal.h"

using namespace ptk;

static int check_temporal_params(ptk_ctx* c, const char* who, const ptk_temporal_params* p)
{
    if (!p) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null params");
    if (!std::isfinite(p->max_plane_dist) || !(p->max_plane_dist > 0.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": max_plane_dist is not a finite positive number");
    if (!std::isfinite(p->min_normal_dot) || !(p->min_normal_dot >= -1.0f && p->min_normal_dot <= 1.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": min_normal_dot outside -1..1");
    if (!std::isfinite(p->max_history) || !(p->max_history >= 1.0f)) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": max_history is not a finite number >= 1");
    return PTK_OK;
}

// The argument checks the planes entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
template <size_t N>
static int check_planes_args(ptk_ctx* c, int width, int height, const ptk_view* view, const void* const (&planes)[N], const ptk_temporal_params* p,
                             bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (width < 0 || height < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_planes: negative size");
    if (const int rc = check_temporal_params(c, "ptk_reproject_planes", p); rc != PTK_OK) return rc;
    if (!view) return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_planes: null view");
    if (width == 0 || height == 0) { *nothing = true; return PTK_OK; }
    for (const void* a : planes)
        if (!a) return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_planes: null plane");
    if ((int64_t)width * height > (1ll << 28) || height > 4 * 65535) return fail(c, PTK_ERR_LIMIT, "ptk_reproject_planes: more than 2^28 pixels or 262140 rows");
    return PTK_OK;
}

// The rule's once-per-call values, in float32 and in the header's order (this file is compiled with -ffp-contract=off too).
static void fill_view(TemporalParams& k, const ptk_view& v, const ptk_temporal_params& p)
{
    const float* r = v.right; const float* u = v.up;
    k.nrm[0] = (r[1] * u[2]) - (r[2] * u[1]); k.nrm[1] = (r[2] * u[0]) - (r[0] * u[2]); k.nrm[2] = (r[0] * u[1]) - (r[1] * u[0]);
    for (int a = 0; a < 3; a++) { k.pos[a] = v.pos[a]; k.right[a] = r[a]; k.up[a] = u[a]; k.e[a] = v.top_left[a] - v.pos[a]; }
    k.num = ((k.e[0] * k.nrm[0]) + (k.e[1] * k.nrm[1])) + (k.e[2] * k.nrm[2]);
    k.delta_x = v.delta_x; k.delta_y = v.delta_y;
    k.zz = p.max_plane_dist * p.max_plane_dist;
    k.min_normal_dot = p.min_normal_dot; k.max_history = p.max_history; k.match_id = p.match_id != 0;
}

// The planes call proper, on the context's stream, every pointer into this GPU's memory: events [0] before the pack, [1] behind
// it, [2] behind the reprojection.
static int planes_on_stream(ptk_ctx* c, int width, int height, const ptk_view& view, const float* d_color, const float* d_count, const int32_t* d_id,
                            const float* d_position, const float* d_normal, const float* d_hist_color, const float* d_hist_count,
                            const int32_t* d_hist_id, const float* d_hist_position, const float* d_hist_normal, const ptk_temporal_params& p,
                            float* d_out_color, float* d_out_count, const float* d_prev_position = nullptr, const float* d_prev_normal = nullptr,
                            const float* d_albedo = nullptr, const float* d_hist_moments = nullptr, float* d_out_moments = nullptr)
{
    c->ev_temporal.begin();
    if (c->ev_motion.timed == 2) c->ev_motion.done(1);      // (ev_temporal stops being the kernel behind the last motion_kernel)
    const size_t px = (size_t)width * height;
    if (const int rc = c->d_temporal_pack.grow(c, px, 3 * sizeof(float4)); rc != PTK_OK) return rc;
    if (d_out_moments)
        if (const int rc = c->d_temporal_pack_mm.grow(c, px, sizeof(float4)); rc != PTK_OK) return rc;
    TemporalImages im = { c->d_temporal_pack, c->d_temporal_pack + px, c->d_temporal_pack + 2 * px };
    if (const int rm = c->ev_temporal.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    TemporalPackParams pk = {};
    pk.color = d_hist_color; pk.count = d_hist_count; pk.id = d_hist_id; pk.position = d_hist_position; pk.normal = d_hist_normal;
    pk.width = width; pk.height = height;
    launch_temporal_pack(pk, im, c->stream);
    if (d_out_moments) launch_temporal_pack_moments(d_hist_moments, c->d_temporal_pack_mm, width, height, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_temporal.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    TemporalParams k = {};
    k.color = d_color; k.count = d_count; k.id = d_id; k.position = d_position; k.normal = d_normal;
    k.hist = im; k.out_color = d_out_color; k.out_count = d_out_count; k.width = width; k.height = height;
    k.prev_position = d_prev_position; k.prev_normal = d_prev_normal;
    k.albedo = d_albedo; k.hist_mm = d_out_moments ? c->d_temporal_pack_mm : nullptr; k.out_moments = d_out_moments;
    fill_view(k, view, p);
    launch_temporal(k, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_temporal.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    c->ev_temporal.done();
    return PTK_OK;
}

// a history set of the frame entries' buffer (ptk_ctx.h cuts up the rest)
static TemporalImages temporal_set(const ptk_ctx* c, size_t px, int set)
{
    float4* b = c->d_temporal + (size_t)set * 3 * px;
    return { b, b + px, b + 2 * px };
}

static bool have_motion(const ptk_ctx* c) { return c->d_motion && c->motion_w == c->width && c->motion_h == c->height && c->motion_w > 0; }
// the motion buffer cut up: previous position | previous normal | motion
static float* motion_prev_position(const ptk_ctx* c, size_t) { return c->d_motion; }
static float* motion_prev_normal(const ptk_ctx* c, size_t px) { return c->d_motion + 3 * px; }
static float* motion_vectors(const ptk_ctx* c, size_t px) { return c->d_motion + 6 * px; }

// What ptk_render_motion and ptk_temporal_frame_moving need of the context beyond their own arguments
static int check_motion_state(ptk_ctx* c, const char* who, uint32_t need, const char* names)
{
    if (!c->have_scene || !c->d_verts_res) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (!c->d_primary || c->width <= 0 || c->height <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": no feature planes for the current resolution: ptk_render_features first");
    if ((c->feat_mask & need) != need) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": the last ptk_render_features lacks " + names);
    return PTK_OK;
}

// motion_kernel over the context's feature planes on the context's stream, between the two events of ev_motion; view null: no
// motion vectors
static int motion_on_stream(ptk_ctx* c, const ptk_view* view)
{
    c->ev_motion.begin();
    const size_t px = (size_t)c->width * c->height;
    if (!c->d_motion) HIPCHK(c, hipMalloc(&c->d_motion.p, px * 8 * sizeof(float)));
    MotionParams m = {};
    m.tri = (const int32_t*)c->d_feat[PTK_FEAT_TRIANGLE].p; m.bary = (const float*)c->d_feat[PTK_FEAT_BARY].p;
    m.position = (const float*)c->d_feat[PTK_FEAT_POSITION].p; m.normal = (const float*)c->d_feat[PTK_FEAT_NORMAL].p;
    m.verts = c->d_verts_res; m.prev = c->have_snapshot ? c->d_verts_prev : nullptr; m.num_tris = c->num_tris;
    m.prev_position = motion_prev_position(c, px); m.prev_normal = motion_prev_normal(c, px); m.motion = motion_vectors(c, px);
    m.width = c->width; m.height = c->height;
    if (view)
    {
        TemporalParams k = {};
        fill_view(k, *view, ptk_temporal_params{ 1.0f, 0.0f, 1.0f, 0 });
        m.have_view = 1;
        for (int a = 0; a < 3; a++) { m.pos[a] = k.pos[a]; m.right[a] = k.right[a]; m.up[a] = k.up[a]; m.e[a] = k.e[a]; m.nrm[a] = k.nrm[a]; }
        m.num = k.num; m.delta_x = k.delta_x; m.delta_y = k.delta_y;
    }
    if (const int rm = c->ev_motion.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    launch_motion(m, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_motion.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    c->ev_motion.done();
    c->motion_w = c->width; c->motion_h = c->height;
    return PTK_OK;
}

// ptk_temporal_frame, ptk_temporal_frame_moving and - moments - ptk_temporal_frame_moments
static int temporal_frame(ptk_ctx* c, const char* who, const ptk_temporal_params* params, uint32_t flags, bool moving, bool moments = false)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_temporal_params(c, who, params); rc != PTK_OK) return rc;
    if (flags & ~PTK_TEMPORAL_RESET) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": unknown flag bit");
    if (!c->d_primary || !accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    uint32_t need = (1u << PTK_FEAT_MATERIAL) | (1u << PTK_FEAT_POSITION) | (1u << PTK_FEAT_NORMAL);
    if (moments) need |= 1u << PTK_FEAT_ALBEDO;
    if (moving)
    {
        need |= (1u << PTK_FEAT_TRIANGLE) | (1u << PTK_FEAT_BARY);
        if (const int rc = check_motion_state(c, who, need, moments ? "MATERIAL, TRIANGLE, BARY, POSITION, NORMAL or ALBEDO" : "MATERIAL, TRIANGLE, BARY, POSITION or NORMAL"); rc != PTK_OK)
            return rc;
    }
    else if (moments)
    {
        if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
            return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": no feature planes for the current resolution: ptk_render_features first");
        if ((c->feat_mask & need) != need) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": the last ptk_render_features lacks MATERIAL, POSITION, NORMAL or ALBEDO");
    }
    else
    {
        if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
            return fail(c, PTK_ERR_BAD_ARG, "ptk_temporal_frame: no feature planes for the current resolution: ptk_render_features first");
        if ((c->feat_mask & need) != need) return fail(c, PTK_ERR_BAD_ARG, "ptk_temporal_frame: the last ptk_render_features lacks MATERIAL, POSITION or NORMAL");
    }
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->width * c->height;
    // (ptk_set_frame with another resolution has freed the buffer with the feature planes: there is no history then)
    const bool fresh = !have_temporal(c);
    if (!c->d_temporal) HIPCHK(c, hipMalloc(&c->d_temporal.p, px * 7 * sizeof(float4)));
    if (moments && !c->d_temporal_mm) HIPCHK(c, hipMalloc(&c->d_temporal_mm.p, px * kTemporalMomentsBytes));
    ptk_view now;
    if (const int rc = ptk_get_view(c, &now); rc != PTK_OK) return rc;
    c->ev_temporal.begin();
    if (c->ev_motion.timed == 2) c->ev_motion.done(1);
    // (a moments call behind a plain one starts over, colour included: a fresh moment pair behind a long colour count would
    // report no variance at all)
    const bool with_history = !fresh && !(flags & PTK_TEMPORAL_RESET) && (!moments || c->temporal_moments);
    if (moving)
        if (const int rc = motion_on_stream(c, with_history ? &c->temporal_view : nullptr); rc != PTK_OK) return rc;
    const bool adaptive = c->adaptive_accum && c->d_counts && c->d_moments;
    const int next = fresh ? 0 : c->temporal_set ^ 1;
    TemporalParams k = {};
    k.accum = accum_ptr(c); k.counts = adaptive ? c->d_counts : nullptr; k.samples = c->samples.load(); k.rank = c->rank; k.world = c->world;
    k.id = (const int32_t*)c->d_feat[PTK_FEAT_MATERIAL].p; k.position = (const float*)c->d_feat[PTK_FEAT_POSITION].p;
    k.normal = (const float*)c->d_feat[PTK_FEAT_NORMAL].p;
    if (with_history) k.hist = temporal_set(c, px, c->temporal_set);
    k.next = temporal_set(c, px, next);
    k.out_color = temporal_color(c, px); k.out_count = temporal_count(c, px); k.width = c->width; k.height = c->height;
    if (moving) { k.prev_position = motion_prev_position(c, px); k.prev_normal = motion_prev_normal(c, px); }
    if (moments)
    {
        k.albedo = (const float*)c->d_feat[PTK_FEAT_ALBEDO].p; k.out_moments = temporal_moments_plane(c, px);
        if (with_history) k.hist_mm = temporal_mm(c, px, c->temporal_set);
        k.next_mm = temporal_mm(c, px, next);
    }
    fill_view(k, c->temporal_view, *params);
    if (const int rm = c->ev_temporal.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    if (const int rm = c->ev_temporal.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    launch_temporal(k, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_temporal.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    c->ev_temporal.done();
    if (moving) c->ev_motion.done(2);
    c->temporal_set = next; c->temporal_view = now; c->temporal_w = c->width; c->temporal_h = c->height;
    c->temporal_moments = moments; c->temporal_variance = false;
    return PTK_OK;
}

extern "C" {

int ptk_get_view(ptk_ctx* c, ptk_view* out)
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    if (!c->d_primary || c->width <= 0 || c->height <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    PrimaryParams pp;
    frame_view(c, pp);
    for (int a = 0; a < 3; a++) { out->pos[a] = pp.cam_pos[a]; out->right[a] = pp.cam_right[a]; out->up[a] = pp.cam_up[a]; out->top_left[a] = pp.top_left[a]; }
    out->delta_x = pp.delta_x; out->delta_y = pp.delta_y;
    return PTK_OK;
}

int ptk_reproject_planes_device(ptk_ctx* c, int width, int height, const ptk_view* view, const float* d_color, const float* d_count,
                                const int32_t* d_id, const float* d_position, const float* d_normal, const float* d_hist_color,
                                const float* d_hist_count, const int32_t* d_hist_id, const float* d_hist_position,
                                const float* d_hist_normal, const ptk_temporal_params* params, float* d_out_color, float* d_out_count)
{
    bool nothing;
    const void* const planes[12] = { d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count, d_hist_id, d_hist_position,
                                     d_hist_normal, d_out_color, d_out_count };
    const int rc = check_planes_args(c, width, height, view, planes, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return planes_on_stream(c, width, height, *view, d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count, d_hist_id,
                            d_hist_position, d_hist_normal, *params, d_out_color, d_out_count);
}

// The host entry: the planes and the outputs staged for the length of the call
int ptk_reproject_planes(ptk_ctx* c, int width, int height, const ptk_view* view, const float* color, const float* count, const int32_t* id,
                         const float* position, const float* normal, const float* hist_color, const float* hist_count, const int32_t* hist_id,
                         const float* hist_position, const float* hist_normal, const ptk_temporal_params* params, float* out_color,
                         float* out_count)
{
    bool nothing;
    const void* const planes[12] = { color, count, id, position, normal, hist_color, hist_count, hist_id, hist_position, hist_normal, out_color, out_count };
    const int rc = check_planes_args(c, width, height, view, planes, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    Stage s(c);
    const auto d_color = s.in(color, 3 * px), d_position = s.in(position, 3 * px), d_normal = s.in(normal, 3 * px), d_count = s.in(count, px);
    const auto d_id = s.in(id, px);
    const auto d_hist_color = s.in(hist_color, 3 * px), d_hist_position = s.in(hist_position, 3 * px), d_hist_normal = s.in(hist_normal, 3 * px);
    const auto d_hist_count = s.in(hist_count, px);
    const auto d_hist_id = s.in(hist_id, px);
    const auto d_out_color = s.out(out_color, 3 * px), d_out_count = s.out(out_count, px);
    return s.run([&] {
        return planes_on_stream(c, width, height, *view, d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count, d_hist_id,
                                d_hist_position, d_hist_normal, *params, d_out_color, d_out_count);
    });
}

int ptk_temporal_frame(ptk_ctx* c, const ptk_temporal_params* params, uint32_t flags)
{
    return temporal_frame(c, "ptk_temporal_frame", params, flags, false);
}

int ptk_read_temporal(ptk_ctx* c, float* color, float* count)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_temporal(c)) return fail(c, PTK_ERR_BAD_ARG, "no reprojected frame at the current resolution: ptk_temporal_frame first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->temporal_w * c->temporal_h;
    if (color) HIPCHK(c, hipMemcpyAsync(color, temporal_color(c, px), px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (count) HIPCHK(c, hipMemcpyAsync(count, temporal_count(c, px), px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_temporal_device_ptr(ptk_ctx* c, void** color, void** count, size_t* pixels)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_temporal(c)) return fail(c, PTK_ERR_BAD_ARG, "no reprojected frame at the current resolution: ptk_temporal_frame first");
    const size_t px = (size_t)c->temporal_w * c->temporal_h;
    if (color) *color = temporal_color(c, px);
    if (count) *count = temporal_count(c, px);
    if (pixels) *pixels = px;
    return PTK_OK;
}

int ptk_last_temporal_ms(ptk_ctx* c, float* pack_ms, float* kernel_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[2] = { 0.0f, 0.0f };
    const int rc = c->ev_temporal.spans(c, 0, 2, t);
    if (pack_ms) *pack_ms = t[0];
    if (kernel_ms) *kernel_ms = t[1];
    return rc;
}

// ---- moving geometry ------------------------------------------------------------------------------------------------------------
int ptk_geometry_snapshot(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (c->num_tris <= 0 || !c->d_verts_res) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t bytes = (size_t)c->num_tris * 9 * sizeof(float);
    if (!c->d_verts_prev) HIPCHK(c, hipMalloc(&c->d_verts_prev.p, bytes));
    // on the stream ptk_update_geometry rewrites d_verts_res on: behind every update so far, ahead of every later one
    HIPCHK(c, hipMemcpyAsync(c->d_verts_prev, c->d_verts_res, bytes, hipMemcpyDeviceToDevice, c->stream));
    c->have_snapshot = true;
    return PTK_OK;
}

int ptk_render_motion(ptk_ctx* c, const ptk_view* view)
{
    if (!c) return PTK_ERR_BAD_ARG;
    const uint32_t need = (1u << PTK_FEAT_TRIANGLE) | (1u << PTK_FEAT_BARY) | (1u << PTK_FEAT_POSITION) | (1u << PTK_FEAT_NORMAL);
    if (const int rc = check_motion_state(c, "ptk_render_motion", need, "TRIANGLE, BARY, POSITION or NORMAL"); rc != PTK_OK) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return motion_on_stream(c, view);
}

int ptk_read_motion(ptk_ctx* c, float* prev_position, float* prev_normal, float* motion)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_motion(c)) return fail(c, PTK_ERR_BAD_ARG, "no motion planes at the current resolution: ptk_render_motion or ptk_temporal_frame_moving first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->motion_w * c->motion_h;
    if (prev_position) HIPCHK(c, hipMemcpyAsync(prev_position, motion_prev_position(c, px), px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (prev_normal) HIPCHK(c, hipMemcpyAsync(prev_normal, motion_prev_normal(c, px), px * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (motion) HIPCHK(c, hipMemcpyAsync(motion, motion_vectors(c, px), px * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_motion_device_ptr(ptk_ctx* c, void** prev_position, void** prev_normal, void** motion, size_t* pixels)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_motion(c)) return fail(c, PTK_ERR_BAD_ARG, "no motion planes at the current resolution: ptk_render_motion or ptk_temporal_frame_moving first");
    const size_t px = (size_t)c->motion_w * c->motion_h;
    if (prev_position) *prev_position = motion_prev_position(c, px);
    if (prev_normal) *prev_normal = motion_prev_normal(c, px);
    if (motion) *motion = motion_vectors(c, px);
    if (pixels) *pixels = px;
    return PTK_OK;
}

int ptk_reproject_planes_moving_device(ptk_ctx* c, int width, int height, const ptk_view* view, const float* d_color, const float* d_count,
                                       const int32_t* d_id, const float* d_position, const float* d_normal, const float* d_prev_position,
                                       const float* d_prev_normal, const float* d_hist_color, const float* d_hist_count, const int32_t* d_hist_id,
                                       const float* d_hist_position, const float* d_hist_normal, const ptk_temporal_params* params,
                                       float* d_out_color, float* d_out_count)
{
    bool nothing;
    const void* const planes[14] = { d_color, d_count, d_id, d_position, d_normal, d_prev_position, d_prev_normal, d_hist_color, d_hist_count,
                                     d_hist_id, d_hist_position, d_hist_normal, d_out_color, d_out_count };
    const int rc = check_planes_args(c, width, height, view, planes, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return planes_on_stream(c, width, height, *view, d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count, d_hist_id,
                            d_hist_position, d_hist_normal, *params, d_out_color, d_out_count, d_prev_position, d_prev_normal);
}

int ptk_reproject_planes_moving(ptk_ctx* c, int width, int height, const ptk_view* view, const float* color, const float* count, const int32_t* id,
                                const float* position, const float* normal, const float* prev_position, const float* prev_normal,
                                const float* hist_color, const float* hist_count, const int32_t* hist_id, const float* hist_position,
                                const float* hist_normal, const ptk_temporal_params* params, float* out_color, float* out_count)
{
    bool nothing;
    const void* const planes[14] = { color, count, id, position, normal, prev_position, prev_normal, hist_color, hist_count, hist_id, hist_position,
                                     hist_normal, out_color, out_count };
    const int rc = check_planes_args(c, width, height, view, planes, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    Stage s(c);
    const auto d_color = s.in(color, 3 * px), d_position = s.in(position, 3 * px), d_normal = s.in(normal, 3 * px), d_count = s.in(count, px);
    const auto d_id = s.in(id, px);
    const auto d_prev_position = s.in(prev_position, 3 * px), d_prev_normal = s.in(prev_normal, 3 * px);
    const auto d_hist_color = s.in(hist_color, 3 * px), d_hist_position = s.in(hist_position, 3 * px), d_hist_normal = s.in(hist_normal, 3 * px);
    const auto d_hist_count = s.in(hist_count, px);
    const auto d_hist_id = s.in(hist_id, px);
    const auto d_out_color = s.out(out_color, 3 * px), d_out_count = s.out(out_count, px);
    return s.run([&] {
        return planes_on_stream(c, width, height, *view, d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count, d_hist_id,
                                d_hist_position, d_hist_normal, *params, d_out_color, d_out_count, d_prev_position, d_prev_normal);
    });
}

int ptk_temporal_frame_moving(ptk_ctx* c, const ptk_temporal_params* params, uint32_t flags)
{
    return temporal_frame(c, "ptk_temporal_frame_moving", params, flags, true);
}

// ---- moments of demodulated luminance through the reprojection --------------------------------------------------------------------
// The checks of the two planes entries
static int check_moments_desc(ptk_ctx* c, const ptk_reproject_desc* d, const ptk_temporal_params* p, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (!d) return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_moments: null descriptor");
    if ((d->prev_position != nullptr) != (d->prev_normal != nullptr))
        return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_moments: prev_position and prev_normal go together");
    const void* const planes[13] = { d->color, d->count, d->id, d->position, d->normal, d->hist_color, d->hist_count, d->hist_id, d->hist_position,
                                     d->hist_normal, d->hist_moments, d->out_color, d->out_count };
    if (const int rc = check_planes_args(c, d->width, d->height, d->hist_view, planes, p, nothing); rc != PTK_OK || *nothing) return rc;
    if (!d->out_moments) return fail(c, PTK_ERR_BAD_ARG, "ptk_reproject_moments: null plane");
    return PTK_OK;
}

int ptk_reproject_moments_device(ptk_ctx* c, const ptk_reproject_desc* d, const ptk_temporal_params* params)
{
    bool nothing;
    const int rc = check_moments_desc(c, d, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return planes_on_stream(c, d->width, d->height, *d->hist_view, d->color, d->count, d->id, d->position, d->normal, d->hist_color, d->hist_count,
                            d->hist_id, d->hist_position, d->hist_normal, *params, d->out_color, d->out_count, d->prev_position, d->prev_normal,
                            d->albedo, d->hist_moments, d->out_moments);
}

int ptk_reproject_moments(ptk_ctx* c, const ptk_reproject_desc* d, const ptk_temporal_params* params)
{
    bool nothing;
    const int rc = check_moments_desc(c, d, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)d->width * d->height;
    Stage s(c);
    const auto d_color = s.in(d->color, 3 * px), d_position = s.in(d->position, 3 * px), d_normal = s.in(d->normal, 3 * px), d_count = s.in(d->count, px);
    const auto d_id = s.in(d->id, px);
    const auto d_prev_position = s.in(d->prev_position, 3 * px), d_prev_normal = s.in(d->prev_normal, 3 * px), d_albedo = s.in(d->albedo, 3 * px);
    const auto d_hist_color = s.in(d->hist_color, 3 * px), d_hist_position = s.in(d->hist_position, 3 * px), d_hist_normal = s.in(d->hist_normal, 3 * px);
    const auto d_hist_count = s.in(d->hist_count, px), d_hist_moments = s.in(d->hist_moments, 2 * px);
    const auto d_hist_id = s.in(d->hist_id, px);
    const auto d_out_color = s.out(d->out_color, 3 * px), d_out_count = s.out(d->out_count, px), d_out_moments = s.out(d->out_moments, 2 * px);
    return s.run([&] {
        return planes_on_stream(c, d->width, d->height, *d->hist_view, d_color, d_count, d_id, d_position, d_normal, d_hist_color, d_hist_count,
                                d_hist_id, d_hist_position, d_hist_normal, *params, d_out_color, d_out_count, d_prev_position, d_prev_normal,
                                d_albedo, d_hist_moments, d_out_moments);
    });
}

int ptk_temporal_frame_moments(ptk_ctx* c, const ptk_temporal_params* params, uint32_t flags)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (flags & ~(PTK_TEMPORAL_RESET | PTK_TEMPORAL_MOVING)) return fail(c, PTK_ERR_BAD_ARG, "ptk_temporal_frame_moments: unknown flag bit");
    return temporal_frame(c, "ptk_temporal_frame_moments", params, flags & PTK_TEMPORAL_RESET, (flags & PTK_TEMPORAL_MOVING) != 0, true);
}

int ptk_last_motion_ms(ptk_ctx* c, float* motion_ms, float* temporal_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[2] = { 0.0f, 0.0f };
    // (the reprojection kernel's events are the frame entry's own, so that it is timed exactly as ptk_last_temporal_ms times it)
    int rc = c->ev_motion.elapsed(c, 0, 1, &t[0]);
    if (rc == PTK_OK && c->ev_motion.timed == 2) rc = c->ev_temporal.elapsed(c, 1, 2, &t[1]);
    if (motion_ms) *motion_ms = t[0];
    if (temporal_ms) *temporal_ms = t[1];
    return rc;
}

}  // extern "C"
