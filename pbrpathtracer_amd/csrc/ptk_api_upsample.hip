// Host side of the ptk C-ABI: guide planes at a resolution of their own and guided upsampling for image planes and for the
// context's frame (ptk.h ptk_render_guides, ptk_upsample_planes, ptk_upsample_frame).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_upsample.h"

using namespace ptk;

static int check_upsample_params(ptk_ctx* c, const char* who, const ptk_upsample_params* p)
{
    if (!p) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null params");
    if (!std::isfinite(p->max_plane_dist) || !(p->max_plane_dist > 0.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": max_plane_dist is not a finite positive number");
    if (!std::isfinite(p->min_normal_dot) || !(p->min_normal_dot >= -1.0f && p->min_normal_dot <= 1.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": min_normal_dot outside -1..1");
    if (p->wide != 0 && p->wide != 1) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": wide is neither 0 nor 1");
    return PTK_OK;
}

static bool over_limit(int width, int height) { return (int64_t)width * height > (1ll << 28) || height > 4 * 65535; }

// The argument checks the planes entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_planes_args(ptk_ctx* c, int w, int h, int W, int H, const void* const (&planes)[9], const void* albedo, const void* hi_albedo,
                             const ptk_upsample_params* p, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (w < 0 || h < 0 || W < 0 || H < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_planes: negative size");
    if (const int rc = check_upsample_params(c, "ptk_upsample_planes", p); rc != PTK_OK) return rc;
    if ((albedo != nullptr) != (hi_albedo != nullptr)) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_planes: the two albedo planes go together");
    if (w == 0 || h == 0 || W == 0 || H == 0) { *nothing = true; return PTK_OK; }
    for (const void* a : planes)
        if (!a) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_planes: null plane");
    if (over_limit(w, h) || over_limit(W, H)) return fail(c, PTK_ERR_LIMIT, "ptk_upsample_planes: more than 2^28 pixels or 262140 rows");
    return PTK_OK;
}

// The low planes as the pack kernel takes them
struct LowPlanes {
    const float* color; const uint32_t* counts; int samples, kind;
    const int32_t* id; const float* position; const float* normal; const float* albedo;
};

// The call proper, on the context's stream, every pointer into this GPU's memory: events [0] before the pack, [1] behind it, [2]
// behind upsample_kernel.  The rule's once-per-call values are computed here, in float32 (this file is compiled with
// -ffp-contract=off too).
static int upsample_on_stream(ptk_ctx* c, int w, int h, const LowPlanes& lo, int W, int H, const int32_t* d_hi_id, const float* d_hi_position,
                              const float* d_hi_normal, const float* d_hi_albedo, const ptk_upsample_params& p, float* d_out_color,
                              int32_t* d_out_class)
{
    c->ev_upsample.begin();
    const size_t px = (size_t)w * h;
    const size_t images = lo.albedo ? 4 : 3;
    if (const int rc = c->d_upsample_pack.grow(c, images * px, sizeof(float4)); rc != PTK_OK) return rc;
    UpsampleImages im = { c->d_upsample_pack, c->d_upsample_pack + px, c->d_upsample_pack + 2 * px, lo.albedo ? c->d_upsample_pack + 3 * px : nullptr };
    if (const int rm = c->ev_upsample.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    UpsamplePackParams pk = {};
    pk.color = lo.color; pk.counts = lo.counts; pk.samples = lo.samples; pk.kind = lo.kind;
    pk.id = lo.id; pk.position = lo.position; pk.normal = lo.normal; pk.albedo = lo.albedo; pk.width = w; pk.height = h;
    launch_upsample_pack(pk, im, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_upsample.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    UpsampleParams k = {};
    k.lo = im; k.w = w; k.h = h;
    k.hi_id = d_hi_id; k.hi_position = d_hi_position; k.hi_normal = d_hi_normal; k.hi_albedo = d_hi_albedo;
    k.out_color = d_out_color; k.out_class = d_out_class; k.W = W; k.H = H;
    k.sx = (float)w / (float)W; k.sy = (float)h / (float)H;
    k.zz = p.max_plane_dist * p.max_plane_dist; k.min_normal_dot = p.min_normal_dot; k.wide = p.wide;
    launch_upsample(k, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_upsample.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    c->ev_upsample.done();
    return PTK_OK;
}

static LowPlanes plane_source(const float* color, const int32_t* id, const float* position, const float* normal, const float* albedo)
{
    return { color, nullptr, 0, UPSAMPLE_SRC_PLANE, id, position, normal, albedo };
}

static int guide_channels(int feature) { int ch = 0; (void)ptk_feature_info(feature, &ch, nullptr); return ch; }

// the plane `feature` of the last ptk_render_guides, or null with the reason in the context's error text
static void* guide_plane(ptk_ctx* c, int feature, size_t* bytes)
{
    if (feature < 0 || feature >= NUM_FEATURES) { fail(c, PTK_ERR_BAD_ARG, "unknown feature id"); return nullptr; }
    if (c->guide_w <= 0 || c->guide_h <= 0) { fail(c, PTK_ERR_BAD_ARG, "no guide planes: ptk_render_guides first"); return nullptr; }
    if (!((c->guide_mask >> feature) & 1u) || !c->d_guide[feature])
    { fail(c, PTK_ERR_BAD_ARG, "this feature was not in the mask of the last ptk_render_guides"); return nullptr; }
    *bytes = (size_t)c->guide_w * c->guide_h * guide_channels(feature) * 4;
    return c->d_guide[feature];
}

// The parameter blocks of a guide render, built HERE and nowhere else: every size in them is the guides' (a frame-sized field among
// them would index the guide planes with the frame's pitch).  The scene, camera and walk fields are fill_params'; the frame's
// tables, buffers and tile split are taken out.
static void guide_params(ptk_ctx* c, int width, int height, uint32_t sample, uint64_t seed, PrimaryParams& pp, RenderParams& p)
{
    frame_view_at(c, width, height, pp);
    pp.primary = c->d_guide_primary;
    fill_params(c, p, sample, 1, seed);
    p.primary = c->d_guide_primary;
    p.primary_hit = nullptr; p.primary_rd = nullptr;           // always the walk
    p.samples = nullptr; p.accum = nullptr; p.rgb8 = nullptr; p.rgb8_host = nullptr; p.queues = nullptr;
    p.width = width; p.height = height;
    p.tiles_x = (width + PTK_TILE - 1) / PTK_TILE;
    p.num_tiles = p.tiles_x * ((height + PTK_TILE - 1) / PTK_TILE);
    p.rank = 0; p.world = 1;
    for (int a = 0; a < 3; a++) p.cam_right[a] = pp.cam_right[a];          // (of the camera as it is now, a pending ptk_set_camera included)
}

static bool have_upsampled(const ptk_ctx* c) { return c->d_upsampled && c->ups_w > 0 && c->ups_h > 0; }
static int32_t* upsampled_class(const ptk_ctx* c) { return (int32_t*)(c->d_upsampled + 3 * (size_t)c->ups_w * c->ups_h); }

extern "C" {

int ptk_render_guides(ptk_ctx* c, int width, int height, uint32_t sample, uint64_t seed, uint32_t mask)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (width < 0 || height < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_render_guides: negative size");
    if (mask >> NUM_FEATURES) return fail(c, PTK_ERR_BAD_ARG, "unknown feature bit in the mask");
    if (c->world > 1) return fail(c, PTK_ERR_BAD_ARG, "ptk_render_guides: not under a tile split");
    if (width == 0 || height == 0) return PTK_OK;
    if (over_limit(width, height)) return fail(c, PTK_ERR_LIMIT, "ptk_render_guides: more than 2^28 pixels or 262140 rows");
    if (c->bvh_stack > PTK_MAX_BVH_DEPTH) return fail(c, PTK_ERR_LIMIT, "BVH needs more entries than the LDS traversal stack holds");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    // (a failure below leaves no guides rather than half of them)
    c->guide_w = c->guide_h = 0; c->guide_mask = 0;
    if (const int rc = c->d_guide_primary.grow(c, px, sizeof(float4)); rc != PTK_OK) return rc;
    for (int k = 0; k < NUM_FEATURES; k++)
        if ((mask >> k) & 1u)
            if (const int rc = c->d_guide[k].grow(c, px, (size_t)guide_channels(k) * 4); rc != PTK_OK) return rc;
    PrimaryParams pp;
    RenderParams p;
    guide_params(c, width, height, sample, seed, pp, p);
    launch_primary(pp, c->stream);
    HIPCHK(c, hipGetLastError());
    FeatureParams f = {};
    void** slot[NUM_FEATURES] = { (void**)&f.depth, (void**)&f.triangle, (void**)&f.material, (void**)&f.bary, (void**)&f.position,
                                  (void**)&f.normal_geom, (void**)&f.normal, (void**)&f.albedo, (void**)&f.emission, (void**)&f.gloss };
    for (int k = 0; k < NUM_FEATURES; k++)
        if ((mask >> k) & 1u) *slot[k] = c->d_guide[k];
    f.sample = sample; f.seed_lo = (uint32_t)seed; f.seed_hi = (uint32_t)(seed >> 32);
    if (mask) launch_features(p, f, p.num_tiles, c->stream);
    HIPCHK(c, hipGetLastError());
    for (int a = 0; a < 3; a++)
    {
        c->guide_view.pos[a] = pp.cam_pos[a]; c->guide_view.right[a] = pp.cam_right[a]; c->guide_view.up[a] = pp.cam_up[a];
        c->guide_view.top_left[a] = pp.top_left[a];
    }
    c->guide_view.delta_x = pp.delta_x; c->guide_view.delta_y = pp.delta_y;
    c->guide_w = width; c->guide_h = height; c->guide_mask = mask;
    return PTK_OK;
}

int ptk_read_guide(ptk_ctx* c, int feature, void* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    size_t bytes = 0;
    void* d = guide_plane(c, feature, &bytes);
    if (!d) return PTK_ERR_BAD_ARG;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, d, bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_guide_device_ptr(ptk_ctx* c, int feature, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    size_t b = 0;
    void* d = guide_plane(c, feature, &b);
    if (!d) return PTK_ERR_BAD_ARG;
    *dev_ptr = d;
    if (bytes) *bytes = b;
    return PTK_OK;
}

int ptk_guide_view(ptk_ctx* c, ptk_view* out)
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    if (c->guide_w <= 0 || c->guide_h <= 0) return fail(c, PTK_ERR_BAD_ARG, "no guide planes: ptk_render_guides first");
    *out = c->guide_view;
    return PTK_OK;
}

int ptk_upsample_planes_device(ptk_ctx* c, int w, int h, const float* d_color, const int32_t* d_id, const float* d_position, const float* d_normal,
                               const float* d_albedo, int W, int H, const int32_t* d_hi_id, const float* d_hi_position, const float* d_hi_normal,
                               const float* d_hi_albedo, const ptk_upsample_params* params, float* d_out_color, int32_t* d_out_class)
{
    bool nothing;
    const void* const planes[9] = { d_color, d_id, d_position, d_normal, d_hi_id, d_hi_position, d_hi_normal, d_out_color, d_out_class };
    const int rc = check_planes_args(c, w, h, W, H, planes, d_albedo, d_hi_albedo, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return upsample_on_stream(c, w, h, plane_source(d_color, d_id, d_position, d_normal, d_albedo), W, H, d_hi_id, d_hi_position, d_hi_normal,
                              d_hi_albedo, *params, d_out_color, d_out_class);
}

// The host entry: the planes and the outputs staged for the length of the call
int ptk_upsample_planes(ptk_ctx* c, int w, int h, const float* color, const int32_t* id, const float* position, const float* normal,
                        const float* albedo, int W, int H, const int32_t* hi_id, const float* hi_position, const float* hi_normal,
                        const float* hi_albedo, const ptk_upsample_params* params, float* out_color, int32_t* out_class)
{
    bool nothing;
    const void* const planes[9] = { color, id, position, normal, hi_id, hi_position, hi_normal, out_color, out_class };
    const int rc = check_planes_args(c, w, h, W, H, planes, albedo, hi_albedo, params, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)w * h, PX = (size_t)W * H;
    Stage s(c);
    const auto d_color = s.in(color, 3 * px), d_position = s.in(position, 3 * px), d_normal = s.in(normal, 3 * px), d_albedo = s.in(albedo, 3 * px);
    const auto d_id = s.in(id, px);
    const auto d_hi_position = s.in(hi_position, 3 * PX), d_hi_normal = s.in(hi_normal, 3 * PX), d_hi_albedo = s.in(hi_albedo, 3 * PX);
    const auto d_hi_id = s.in(hi_id, PX);
    const auto d_out_color = s.out(out_color, 3 * PX);
    const auto d_out_class = s.out(out_class, PX);
    return s.run([&] {
        return upsample_on_stream(c, w, h, plane_source(d_color, d_id, d_position, d_normal, d_albedo), W, H, d_hi_id, d_hi_position, d_hi_normal,
                                  d_hi_albedo, *params, d_out_color, d_out_class);
    });
}

int ptk_upsample_frame(ptk_ctx* c, int source, const ptk_upsample_params* params)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_upsample_params(c, "ptk_upsample_frame", params); rc != PTK_OK) return rc;
    if (source != PTK_UPSAMPLE_ACCUM && source != PTK_UPSAMPLE_DENOISED && source != PTK_UPSAMPLE_TEMPORAL)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: unknown source");
    if (!c->d_primary || !accum_ptr(c) || c->width <= 0 || c->height <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (c->world > 1) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: not under a tile split");
    const uint32_t need = (1u << PTK_FEAT_MATERIAL) | (1u << PTK_FEAT_POSITION) | (1u << PTK_FEAT_NORMAL) | (1u << PTK_FEAT_ALBEDO);
    if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: no feature planes for the current resolution: ptk_render_features first");
    if ((c->feat_mask & need) != need) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: the last ptk_render_features lacks MATERIAL, POSITION, NORMAL or ALBEDO");
    if (c->guide_w <= 0 || c->guide_h <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: no guide planes: ptk_render_guides first");
    if ((c->guide_mask & need) != need) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: the last ptk_render_guides lacks MATERIAL, POSITION, NORMAL or ALBEDO");
    const int w = c->width, h = c->height, W = c->guide_w, H = c->guide_h;
    if ((int64_t)W * h != (int64_t)H * w) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: the frame and the guide planes differ in aspect ratio");
    const size_t px = (size_t)w * h, PX = (size_t)W * H;
    LowPlanes lo = plane_source(nullptr, (const int32_t*)c->d_feat[PTK_FEAT_MATERIAL].p, (const float*)c->d_feat[PTK_FEAT_POSITION].p,
                                (const float*)c->d_feat[PTK_FEAT_NORMAL].p, (const float*)c->d_feat[PTK_FEAT_ALBEDO].p);
    if (source == PTK_UPSAMPLE_DENOISED)
    {
        if (!c->d_denoised || c->den_w != w || c->den_h != h || c->den_w == 0)
            return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: no denoised frame at the current resolution");
        lo.color = c->d_denoised;
    }
    else if (source == PTK_UPSAMPLE_TEMPORAL)
    {
        if (!have_temporal(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_upsample_frame: no temporal frame at the current resolution");
        lo.color = temporal_color(c, px);
    }
    else
    {
        const bool adaptive = c->adaptive_accum && c->d_counts && c->d_moments;
        lo.color = accum_ptr(c);
        lo.counts = adaptive ? c->d_counts : nullptr;
        lo.samples = c->samples.load();
        lo.kind = adaptive ? UPSAMPLE_SRC_ACCUM_COUNTS : UPSAMPLE_SRC_ACCUM_SAMPLES;
    }
    HIPCHK(c, hipSetDevice(c->device));
    // (a result of another size is gone once its buffer is handed to this call)
    const int was_w = c->ups_w, was_h = c->ups_h;
    c->ups_w = c->ups_h = 0;
    if (const int rc = c->d_upsampled.grow(c, PX, 4 * sizeof(float)); rc != PTK_OK) return rc;
    c->ups_w = W; c->ups_h = H;
    const int rc = upsample_on_stream(c, w, h, lo, W, H, (const int32_t*)c->d_guide[PTK_FEAT_MATERIAL].p, (const float*)c->d_guide[PTK_FEAT_POSITION].p,
                                      (const float*)c->d_guide[PTK_FEAT_NORMAL].p, (const float*)c->d_guide[PTK_FEAT_ALBEDO].p, *params, c->d_upsampled,
                                      upsampled_class(c));
    if (rc != PTK_OK && (was_w != W || was_h != H)) c->ups_w = c->ups_h = 0;
    return rc;
}

int ptk_read_upsampled(ptk_ctx* c, float* color, int32_t* cls)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_upsampled(c)) return fail(c, PTK_ERR_BAD_ARG, "no upsampled frame: ptk_upsample_frame first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t PX = (size_t)c->ups_w * c->ups_h;
    if (color) HIPCHK(c, hipMemcpyAsync(color, c->d_upsampled, PX * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (cls) HIPCHK(c, hipMemcpyAsync(cls, upsampled_class(c), PX * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_upsampled_device_ptr(ptk_ctx* c, void** color, void** cls, int* width, int* height)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_upsampled(c)) return fail(c, PTK_ERR_BAD_ARG, "no upsampled frame: ptk_upsample_frame first");
    if (color) *color = c->d_upsampled;
    if (cls) *cls = upsampled_class(c);
    if (width) *width = c->ups_w;
    if (height) *height = c->ups_h;
    return PTK_OK;
}

int ptk_last_upsample_ms(ptk_ctx* c, float* pack_ms, float* kernel_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[2] = { 0.0f, 0.0f };
    const int rc = c->ev_upsample.spans(c, 0, 2, t);
    if (pack_ms) *pack_ms = t[0];
    if (kernel_ms) *kernel_ms = t[1];
    return rc;
}

}  // extern "C"
