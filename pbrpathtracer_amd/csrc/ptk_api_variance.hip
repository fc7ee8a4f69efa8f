// Host side of the ptk C-ABI: the variance of the accumulated demodulated luminance from its temporal moments, for image planes and
// for the context's temporal result, and the denoiser run over that result on the device (ptk.h ptk_variance_planes,
// ptk_temporal_variance, ptk_denoise_temporal).  The moments themselves come out of the reprojection
// (ptk_api_temporal.hip).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_variance.h"

using namespace ptk;

static int check_variance_params(ptk_ctx* c, const char* who, const ptk_variance_params* p)
{
    if (!p) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null params");
    if (p->radius < 1 || p->radius > 3) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": radius outside 1..3");
    if (p->prefilter != 0 && p->prefilter != 1) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": prefilter is neither 0 nor 1");
    if (!std::isfinite(p->min_frames) || !(p->min_frames >= 2.0f)) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": min_frames is not a finite number >= 2");
    if (!std::isfinite(p->max_plane_dist) || !(p->max_plane_dist > 0.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": max_plane_dist is not a finite positive number");
    if (!std::isfinite(p->min_normal_dot) || !(p->min_normal_dot >= -1.0f && p->min_normal_dot <= 1.0f))
        return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": min_normal_dot outside -1..1");
    return PTK_OK;
}

// The argument checks the planes entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_planes_args(ptk_ctx* c, int width, int height, const float* moments, const float* count, const float* frame_count, const int32_t* id,
                             const float* position, const float* normal, const ptk_variance_params* p, const float* out, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (width < 0 || height < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_variance_planes: negative size");
    if (const int rc = check_variance_params(c, "ptk_variance_planes", p); rc != PTK_OK) return rc;
    if (width == 0 || height == 0) { *nothing = true; return PTK_OK; }
    if (!moments || !count || !frame_count || !id || !position || !normal || !out) return fail(c, PTK_ERR_BAD_ARG, "ptk_variance_planes: null plane");
    if ((int64_t)width * height > (1ll << 28) || height > 4 * 65535) return fail(c, PTK_ERR_LIMIT, "ptk_variance_planes: more than 2^28 pixels or 262140 rows");
    return PTK_OK;
}

// variance_kernel and the prefilter over packed images, on the context's stream: events [0] before variance_kernel, [1] behind it,
// [2] behind the prefilter.  d_raw is needed with the prefilter only; without it variance_kernel writes d_out itself.
static int variance_on_stream(ptk_ctx* c, int width, int height, const VarianceImages& im, const ptk_variance_params& p, float* d_raw, float* d_out)
{
    c->ev_variance.begin();
    VarianceParams k = {};
    k.mm = im.mm; k.pi = im.pi; k.nz = im.nz; k.raw = p.prefilter ? d_raw : d_out; k.width = width; k.height = height;
    k.radius = p.radius; k.mark = p.prefilter; k.min_frames = p.min_frames; k.zz = p.max_plane_dist * p.max_plane_dist;
    k.min_normal_dot = p.min_normal_dot;
    if (const int rm = c->ev_variance.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    launch_variance(k, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_variance.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    if (p.prefilter)
    {
        VariancePrefilterParams f = {};
        f.raw = d_raw; f.out = d_out; f.width = width; f.height = height;
        launch_variance_prefilter(f, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (const int rm = c->ev_variance.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    c->ev_variance.done(p.prefilter ? 2 : 1);
    return PTK_OK;
}

// The planes call proper, on the context's stream, every pointer into this GPU's memory: the pack, then the above.
static int planes_on_stream(ptk_ctx* c, int width, int height, const float* d_moments, const float* d_count, const float* d_frame_count,
                            const int32_t* d_id, const float* d_position, const float* d_normal, const ptk_variance_params& p, float* d_out)
{
    const size_t px = (size_t)width * height;
    // three float4 images, and the raw plane behind them
    if (const int rc = c->d_variance_pack.grow(c, px, 3 * sizeof(float4) + sizeof(float)); rc != PTK_OK) return rc;
    const VarianceImages im = { c->d_variance_pack, c->d_variance_pack + px, c->d_variance_pack + 2 * px };
    VariancePackParams k = {};
    k.moments = d_moments; k.count = d_count; k.frame_count = d_frame_count; k.id = d_id; k.position = d_position; k.normal = d_normal;
    k.width = width; k.height = height;
    launch_variance_pack(k, im, c->stream);
    HIPCHK(c, hipGetLastError());
    return variance_on_stream(c, width, height, im, p, (float*)(c->d_variance_pack + 3 * px), d_out);
}

extern "C" {

int ptk_variance_planes_device(ptk_ctx* c, int width, int height, const float* d_moments, const float* d_count, const float* d_frame_count,
                               const int32_t* d_id, const float* d_position, const float* d_normal, const ptk_variance_params* params,
                               float* d_out_variance)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, d_moments, d_count, d_frame_count, d_id, d_position, d_normal, params, d_out_variance, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return planes_on_stream(c, width, height, d_moments, d_count, d_frame_count, d_id, d_position, d_normal, *params, d_out_variance);
}

// The host entry: the planes and the output staged for the length of the call
int ptk_variance_planes(ptk_ctx* c, int width, int height, const float* moments, const float* count, const float* frame_count, const int32_t* id,
                        const float* position, const float* normal, const ptk_variance_params* params, float* out_variance)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, moments, count, frame_count, id, position, normal, params, out_variance, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    Stage s(c);
    const auto d_moments = s.in(moments, 2 * px), d_count = s.in(count, px), d_frame_count = s.in(frame_count, px);
    const auto d_id = s.in(id, px);
    const auto d_position = s.in(position, 3 * px), d_normal = s.in(normal, 3 * px);
    const auto d_out = s.out(out_variance, px);
    return s.run([&] { return planes_on_stream(c, width, height, d_moments, d_count, d_frame_count, d_id, d_position, d_normal, *params, d_out); });
}

int ptk_temporal_variance(ptk_ctx* c, const ptk_variance_params* params)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_variance_params(c, "ptk_temporal_variance", params); rc != PTK_OK) return rc;
    if (!have_temporal_moments(c))
        return fail(c, PTK_ERR_BAD_ARG, "ptk_temporal_variance: no moments at the current resolution: ptk_temporal_frame_moments first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->temporal_w * c->temporal_h;
    // the history set the moments call has just written: its pi and nz are that call's MATERIAL, POSITION and NORMAL
    float4* set = c->d_temporal + (size_t)c->temporal_set * 3 * px;
    const VarianceImages im = { temporal_mm(c, px, c->temporal_set), set + px, set + 2 * px };
    const int rc = variance_on_stream(c, c->temporal_w, c->temporal_h, im, *params, temporal_raw_variance(c, px), temporal_variance_plane(c, px));
    if (rc == PTK_OK) c->temporal_variance = true;
    return rc;
}

int ptk_read_temporal_variance(ptk_ctx* c, float* moments, float* variance)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_temporal_moments(c)) return fail(c, PTK_ERR_BAD_ARG, "no moments at the current resolution: ptk_temporal_frame_moments first");
    if (variance && !c->temporal_variance) return fail(c, PTK_ERR_BAD_ARG, "no variance of the last moments call: ptk_temporal_variance first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->temporal_w * c->temporal_h;
    if (moments) HIPCHK(c, hipMemcpyAsync(moments, temporal_moments_plane(c, px), px * 2 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    if (variance) HIPCHK(c, hipMemcpyAsync(variance, temporal_variance_plane(c, px), px * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_temporal_variance_device_ptr(ptk_ctx* c, void** moments, void** variance, size_t* pixels)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!have_temporal_moments(c)) return fail(c, PTK_ERR_BAD_ARG, "no moments at the current resolution: ptk_temporal_frame_moments first");
    if (variance && !c->temporal_variance) return fail(c, PTK_ERR_BAD_ARG, "no variance of the last moments call: ptk_temporal_variance first");
    const size_t px = (size_t)c->temporal_w * c->temporal_h;
    if (moments) *moments = temporal_moments_plane(c, px);
    if (variance) *variance = temporal_variance_plane(c, px);
    if (pixels) *pixels = px;
    return PTK_OK;
}

int ptk_denoise_temporal(ptk_ctx* c, const ptk_denoise_params* params, uint32_t flags)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_denoise_params(c, "ptk_denoise_temporal", params); rc != PTK_OK) return rc;
    if (flags & ~PTK_DENOISE_VARIANCE) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_temporal: unknown flag bit");
    if (!c->d_primary || c->width <= 0 || c->height <= 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (!have_temporal(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_temporal: no reprojected frame at the current resolution: ptk_temporal_frame first");
    const uint32_t need = (1u << PTK_FEAT_TRIANGLE) | (1u << PTK_FEAT_POSITION) | (1u << PTK_FEAT_NORMAL) | (1u << PTK_FEAT_ALBEDO) | (1u << PTK_FEAT_EMISSION);
    if (c->feat_w != c->width || c->feat_h != c->height || (c->feat_mask & need) != need)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_temporal: the last ptk_render_features lacks TRIANGLE, POSITION, NORMAL, ALBEDO or EMISSION");
    const bool variance = (flags & PTK_DENOISE_VARIANCE) != 0;
    if (variance && !(have_temporal_moments(c) && c->temporal_variance))
        return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_temporal: PTK_DENOISE_VARIANCE needs ptk_temporal_variance behind the last ptk_temporal_frame_moments");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->width * c->height;
    if (!c->d_temporal_mm) HIPCHK(c, hipMalloc(&c->d_temporal_mm.p, px * kTemporalMomentsBytes));      // (the mask lives there)
    if (!c->d_denoised) HIPCHK(c, hipMalloc(&c->d_denoised.p, px * 3 * sizeof(float)));
    int32_t* mask = temporal_mask_plane(c, px);
    launch_temporal_mask(temporal_count(c, px), (const int32_t*)c->d_feat[PTK_FEAT_TRIANGLE].p, (const float*)c->d_feat[PTK_FEAT_EMISSION].p, mask, c->width,
                         c->height, c->stream);
    HIPCHK(c, hipGetLastError());
    const int rc = denoise_planes_on_stream(c, c->width, c->height, temporal_color(c, px), mask, (const float*)c->d_feat[PTK_FEAT_NORMAL].p,
                                            (const float*)c->d_feat[PTK_FEAT_POSITION].p, (const float*)c->d_feat[PTK_FEAT_ALBEDO].p,
                                            variance ? temporal_variance_plane(c, px) : nullptr, *params, c->d_denoised, nullptr);
    if (rc == PTK_OK) { c->den_w = c->width; c->den_h = c->height; }
    return rc;
}

int ptk_last_variance_ms(ptk_ctx* c, float* variance_ms, float* prefilter_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[2] = { 0.0f, 0.0f };
    const int rc = c->ev_variance.spans(c, 0, c->ev_variance.timed == 2 ? 2 : 1, t);
    if (variance_ms) *variance_ms = t[0];
    if (prefilter_ms) *prefilter_ms = t[1];
    return rc;
}

}  // extern "C"
