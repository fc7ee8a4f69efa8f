// Host side of the ptk C-ABI: the a-trous denoiser for image planes and for the context's frame (ptk.h ptk_denoise_planes,
// ptk_denoise_frame).
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_denoise.h"

using namespace ptk;

int ptk::check_denoise_params(ptk_ctx* c, const char* who, const ptk_denoise_params* p)
{
    if (!p) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": null params");
    if (p->iterations < 1 || p->iterations > 8) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": iterations outside 1..8");
    if (p->normal_squarings < 0 || p->normal_squarings > 7) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": normal_squarings outside 0..7");
    if (!std::isfinite(p->sigma_z) || !(p->sigma_z > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": sigma_z is not a finite positive number");
    if (!std::isfinite(p->sigma_l) || !(p->sigma_l > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, std::string(who) + ": sigma_l is not a finite positive number");
    return PTK_OK;
}

// The argument checks the planes entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_planes_args(ptk_ctx* c, int width, int height, const float* color, const int32_t* mask, const float* normal, const float* position,
                             const float* variance, const ptk_denoise_params* p, const float* out_color, const float* out_variance, bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (width < 0 || height < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_planes: negative size");
    if (const int rc = check_denoise_params(c, "ptk_denoise_planes", p); rc != PTK_OK) return rc;
    if (out_variance && !variance) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_planes: out_variance without a variance plane");
    if (width == 0 || height == 0) { *nothing = true; return PTK_OK; }
    if (!color || !mask || !normal || !position || !out_color) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_planes: null plane");
    if ((int64_t)width * height > (1ll << 28) || height > 4 * 65535) return fail(c, PTK_ERR_LIMIT, "ptk_denoise_planes: more than 2^28 pixels or 262140 rows");
    return PTK_OK;
}

// the context's four packed images for `px` pixels (64 B per pixel, grown to the largest call so far)
static int denoise_images(ptk_ctx* c, size_t px, DenoiseImages& im)
{
    if (const int rc = c->d_denoise.grow(c, px, 4 * sizeof(float4)); rc != PTK_OK) return rc;
    im.g0 = c->d_denoise; im.g1 = im.g0 + px; im.c[0] = im.g1 + px; im.c[1] = im.c[0] + px;
    return PTK_OK;
}

// The iterations and the unpack behind a pack that has been launched: events [1] behind the pack, [2] behind the filter, [3]
// behind the unpack ([0] was recorded by the caller, before its pack).
static int filter_on_stream(ptk_ctx* c, int width, int height, const DenoiseImages& im, bool have_variance, const ptk_denoise_params& p,
                            const float* d_albedo, float* d_out_color, float* d_out_variance)
{
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_denoise.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    DenoiseFilterParams f = {};
    f.g0 = im.g0; f.g1 = im.g1; f.width = width; f.height = height;
    f.iterations = p.iterations; f.normal_squarings = p.normal_squarings; f.have_variance = have_variance ? 1 : 0;
    f.sigma_z = p.sigma_z; f.sigma_l = p.sigma_l;
    for (int k = 0; k < p.iterations; k++)
    {
        f.in = im.c[k & 1]; f.out = im.c[(k + 1) & 1]; f.s = 1 << k;
        launch_denoise_filter(f, c->stream);
    }
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_denoise.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    DenoiseUnpackParams u = {};
    u.g0 = im.g0; u.c = im.c[p.iterations & 1]; u.albedo = d_albedo; u.out_color = d_out_color; u.out_variance = d_out_variance;
    u.width = width; u.height = height;
    launch_denoise_unpack(u, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_denoise.mark(c, 3, c->stream); rm != PTK_OK) return rm;
    c->ev_denoise.done();
    return PTK_OK;
}

// The planes call proper, on the context's stream, every pointer into this GPU's memory.
static int planes_on_stream(ptk_ctx* c, int width, int height, const float* d_color, const int32_t* d_mask, const float* d_normal,
                            const float* d_position, const float* d_albedo, const float* d_variance, const ptk_denoise_params& p,
                            float* d_out_color, float* d_out_variance)
{
    c->ev_denoise.begin();
    DenoiseImages im;
    if (const int rc = denoise_images(c, (size_t)width * height, im); rc != PTK_OK) return rc;
    if (const int rm = c->ev_denoise.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    DenoisePackParams k = {};
    k.color = d_color; k.mask = d_mask; k.normal = d_normal; k.position = d_position; k.albedo = d_albedo; k.variance = d_variance;
    k.width = width; k.height = height;
    launch_denoise_pack(k, im, c->stream);
    return filter_on_stream(c, width, height, im, d_variance != nullptr, p, d_albedo, d_out_color, d_out_variance);
}

int ptk::denoise_planes_on_stream(ptk_ctx* c, int width, int height, const float* d_color, const int32_t* d_mask, const float* d_normal,
                                  const float* d_position, const float* d_albedo, const float* d_variance, const ptk_denoise_params& p,
                                  float* d_out_color, float* d_out_variance)
{
    return planes_on_stream(c, width, height, d_color, d_mask, d_normal, d_position, d_albedo, d_variance, p, d_out_color, d_out_variance);
}

static bool have_denoised(const ptk_ctx* c) { return c->d_denoised && c->den_w == c->width && c->den_h == c->height && c->den_w > 0; }

extern "C" {

int ptk_denoise_planes_device(ptk_ctx* c, int width, int height, const float* d_color, const int32_t* d_mask, const float* d_normal,
                              const float* d_position, const float* d_albedo, const float* d_variance, const ptk_denoise_params* params,
                              float* d_out_color, float* d_out_variance)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, d_color, d_mask, d_normal, d_position, d_variance, params, d_out_color, d_out_variance, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return planes_on_stream(c, width, height, d_color, d_mask, d_normal, d_position, d_albedo, d_variance, *params, d_out_color, d_out_variance);
}

// The host entry: the planes and the requested outputs staged for the length of the call
int ptk_denoise_planes(ptk_ctx* c, int width, int height, const float* color, const int32_t* mask, const float* normal, const float* position,
                       const float* albedo, const float* variance, const ptk_denoise_params* params, float* out_color, float* out_variance)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, color, mask, normal, position, variance, params, out_color, out_variance, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    Stage s(c);
    const auto d_color = s.in(color, 3 * px), d_normal = s.in(normal, 3 * px), d_position = s.in(position, 3 * px);
    const auto d_mask = s.in(mask, px);
    const auto d_albedo = s.in(albedo, 3 * px), d_variance = s.in(variance, px);
    const auto d_out_color = s.out(out_color, 3 * px), d_out_variance = s.out(out_variance, px);
    return s.run([&] {
        return planes_on_stream(c, width, height, d_color, d_mask, d_normal, d_position, d_albedo, d_variance, *params, d_out_color, d_out_variance);
    });
}

int ptk_denoise_frame(ptk_ctx* c, const ptk_denoise_params* params, uint32_t flags)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_denoise_params(c, "ptk_denoise_frame", params); rc != PTK_OK) return rc;
    if (flags & ~PTK_DENOISE_VARIANCE) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_frame: unknown flag bit");
    if (!c->d_primary || !accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    if (c->feat_w != c->width || c->feat_h != c->height || c->feat_w == 0)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_frame: no feature planes for the current resolution: ptk_render_features first");
    const uint32_t need = (1u << PTK_FEAT_TRIANGLE) | (1u << PTK_FEAT_POSITION) | (1u << PTK_FEAT_NORMAL) | (1u << PTK_FEAT_ALBEDO) | (1u << PTK_FEAT_EMISSION);
    if ((c->feat_mask & need) != need)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_frame: the last ptk_render_features lacks TRIANGLE, POSITION, NORMAL, ALBEDO or EMISSION");
    const bool adaptive = c->adaptive_accum && c->d_counts && c->d_moments;
    const bool variance = (flags & PTK_DENOISE_VARIANCE) != 0;
    if (variance && !adaptive) return fail(c, PTK_ERR_BAD_ARG, "ptk_denoise_frame: PTK_DENOISE_VARIANCE needs an adaptive render in the accumulator");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)c->width * c->height;
    if (!c->d_denoised) HIPCHK(c, hipMalloc(&c->d_denoised.p, px * 3 * sizeof(float)));
    c->ev_denoise.begin();
    DenoiseImages im;
    if (const int rc = denoise_images(c, px, im); rc != PTK_OK) return rc;
    if (const int rm = c->ev_denoise.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    DenoiseFramePackParams k = {};
    k.accum = accum_ptr(c); k.moments = variance ? c->d_moments : nullptr; k.counts = adaptive ? c->d_counts : nullptr;
    k.triangle = (const int32_t*)c->d_feat[PTK_FEAT_TRIANGLE].p; k.emission = (const float*)c->d_feat[PTK_FEAT_EMISSION].p;
    k.normal = (const float*)c->d_feat[PTK_FEAT_NORMAL].p; k.position = (const float*)c->d_feat[PTK_FEAT_POSITION].p;
    k.albedo = (const float*)c->d_feat[PTK_FEAT_ALBEDO].p;
    k.width = c->width; k.height = c->height; k.samples = c->samples.load(); k.rank = c->rank; k.world = c->world;
    launch_denoise_pack_frame(k, im, c->stream);
    const int rc = filter_on_stream(c, c->width, c->height, im, variance, *params, k.albedo, c->d_denoised, nullptr);
    if (rc == PTK_OK) { c->den_w = c->width; c->den_h = c->height; }
    return rc;
}

int ptk_read_denoised(ptk_ctx* c, float* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!have_denoised(c)) return fail(c, PTK_ERR_BAD_ARG, "no denoised frame at the current resolution: ptk_denoise_frame first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_denoised, (size_t)c->den_w * c->den_h * 3 * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_denoised_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    if (!have_denoised(c)) return fail(c, PTK_ERR_BAD_ARG, "no denoised frame at the current resolution: ptk_denoise_frame first");
    *dev_ptr = c->d_denoised;
    if (bytes) *bytes = (size_t)c->den_w * c->den_h * 3 * sizeof(float);
    return PTK_OK;
}

int ptk_resolve_denoised_rgb8(ptk_ctx* c, uint8_t* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!have_denoised(c)) return fail(c, PTK_ERR_BAD_ARG, "no denoised frame at the current resolution: ptk_denoise_frame first");
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)c->den_w * c->den_h * 3;
    Stage s(c);
    const auto d_out = s.out(host_out, n);
    return s.run([&] {
        launch_denoise_resolve8(c->d_denoised, d_out, n, c->stream);
        return s.launched();
    });
}

int ptk_last_denoise_ms(ptk_ctx* c, float* pack_ms, float* filter_ms, float* unpack_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[3] = { 0.0f, 0.0f, 0.0f };
    const int rc = c->ev_denoise.spans(c, 0, 3, t);
    if (pack_ms) *pack_ms = t[0];
    if (filter_ms) *filter_ms = t[1];
    if (unpack_ms) *unpack_ms = t[2];
    return rc;
}

}  // extern "C"
