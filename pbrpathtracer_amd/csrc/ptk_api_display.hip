// Host side of the ptk C-ABI: the display transform for image planes and for the context's frame (ptk.h ptk_display_planes,
// ptk_display_frame).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_display.h"

using namespace ptk;

static const float kSrgbTable[256] = { PTK_DISPLAY_SRGB_VALUES };

static int check_display_params(ptk_ctx* c, const char* who, const ptk_display_params* p)
{
    const std::string w = std::string(who) + ": ";
    if (!p) return fail(c, PTK_ERR_BAD_ARG, w + "null params");
    if (p->mode != PTK_EXPOSURE_MANUAL && p->mode != PTK_EXPOSURE_METERED) return fail(c, PTK_ERR_BAD_ARG, w + "unknown mode");
    if (p->op != PTK_DISPLAY_LINEAR && p->op != PTK_DISPLAY_REINHARD && p->op != PTK_DISPLAY_ACES) return fail(c, PTK_ERR_BAD_ARG, w + "unknown op");
    if (p->transfer != PTK_TRANSFER_LINEAR && p->transfer != PTK_TRANSFER_SRGB) return fail(c, PTK_ERR_BAD_ARG, w + "unknown transfer");
    if (p->mode == PTK_EXPOSURE_MANUAL && !(p->exposure > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, w + "the manual exposure is NaN or <= 0");
    if (!(p->key > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, w + "key is NaN or <= 0");
    if (!(p->white > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, w + "white is NaN or <= 0");
    if (!std::isfinite(p->min_exposure) || !std::isfinite(p->max_exposure) || !(p->min_exposure > 0.0f) || !(p->max_exposure > 0.0f))
        return fail(c, PTK_ERR_BAD_ARG, w + "min_exposure or max_exposure is not a finite positive number");
    if (!std::isfinite(p->min_lum) || !std::isfinite(p->max_lum)) return fail(c, PTK_ERR_BAD_ARG, w + "min_lum or max_lum is not finite");
    if (p->min_lum < 1.17549435e-38f || p->min_lum > p->max_lum) return fail(c, PTK_ERR_BAD_ARG, w + "min_lum below 2^-126 or above max_lum");
    if (!(0 <= p->low_permille && p->low_permille < p->high_permille && p->high_permille <= 1000))
        return fail(c, PTK_ERR_BAD_ARG, w + "permilles outside 0 <= low < high <= 1000");
    if (!(p->adapt >= 0.0f)) return fail(c, PTK_ERR_BAD_ARG, w + "adapt is NaN or negative");
    return PTK_OK;
}

// The argument checks the planes entries share; PTK_OK with *nothing = true: the call is legal and has nothing to do.
static int check_planes_args(ptk_ctx* c, int width, int height, const float* color, const ptk_display_params* p, const uint8_t* rgb8_out,
                             bool* nothing)
{
    *nothing = false;
    if (!c) return PTK_ERR_BAD_ARG;
    if (width < 0 || height < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_display_planes: negative size");
    if (const int rc = check_display_params(c, "ptk_display_planes", p); rc != PTK_OK) return rc;
    if (width == 0 || height == 0) { *nothing = true; return PTK_OK; }
    if (!color || !rgb8_out) return fail(c, PTK_ERR_BAD_ARG, "ptk_display_planes: null plane");
    if ((int64_t)width * height > (1ll << 28)) return fail(c, PTK_ERR_LIMIT, "ptk_display_planes: more than 2^28 pixels");
    return PTK_OK;
}

static ptk_exposure_state* state_ptr(const ptk_ctx* c) { return (ptk_exposure_state*)(c->d_display_hist + DISPLAY_BINS); }

// the context's histogram and state, made and zeroed by the first call
static int ensure_state(ptk_ctx* c)
{
    if (c->d_display_hist) return PTK_OK;
    const size_t bytes = DISPLAY_BINS * sizeof(uint32_t) + sizeof(ptk_exposure_state);
    HIPCHK(c, hipMalloc(&c->d_display_hist.p, bytes));
    HIPCHK(c, hipMemsetAsync(c->d_display_hist, 0, bytes, c->stream));
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory: events [0] before the meter, [1] behind it,
// [2] behind the exposure step, [3] behind the apply kernel (a manual call launches the last alone).
static int display_on_stream(ptk_ctx* c, const DisplaySource& src, const ptk_display_params& p, uint8_t* d_rgb8, ptk_exposure_state* d_state_out)
{
    c->ev_display.begin();
    if (const int rc = ensure_state(c); rc != PTK_OK) return rc;
    const bool metered = p.mode == PTK_EXPOSURE_METERED;
    if (const int rm = c->ev_display.mark(c, 0, c->stream); rm != PTK_OK) return rm;
    if (metered)
    {
        DisplayMeterParams m = {};
        m.src = src; m.hist = c->d_display_hist; m.min_lum = p.min_lum; m.max_lum = p.max_lum;
        launch_display_meter(m, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (const int rm = c->ev_display.mark(c, 1, c->stream); rm != PTK_OK) return rm;
    if (metered)
    {
        DisplayExposureParams x = {};
        x.hist = c->d_display_hist; x.state = state_ptr(c);
        x.low_permille = (uint32_t)p.low_permille; x.high_permille = (uint32_t)p.high_permille;
        x.key = p.key; x.min_exposure = p.min_exposure; x.max_exposure = p.max_exposure; x.adapt = p.adapt;
        launch_display_exposure(x, c->stream);
        HIPCHK(c, hipGetLastError());
    }
    if (const int rm = c->ev_display.mark(c, 2, c->stream); rm != PTK_OK) return rm;
    DisplayApplyParams a = {};
    a.src = src; a.rgb8 = d_rgb8; a.state = metered ? state_ptr(c) : nullptr; a.exposure = p.exposure;
    a.iw2 = 1.0f / (p.white * p.white); a.op = p.op; a.transfer = p.transfer;
    launch_display_apply(a, c->stream);
    HIPCHK(c, hipGetLastError());
    if (const int rm = c->ev_display.mark(c, 3, c->stream); rm != PTK_OK) return rm;
    c->ev_display.done();
    if (d_state_out) HIPCHK(c, hipMemcpyAsync(d_state_out, state_ptr(c), sizeof(ptk_exposure_state), hipMemcpyDeviceToDevice, c->stream));
    return PTK_OK;
}

static DisplaySource plane_source(const float* d_color, int width, int height)
{
    DisplaySource s = {};
    s.color = d_color; s.width = width; s.height = height; s.world = 1; s.kind = DISPLAY_SRC_PLANE;
    return s;
}

static bool have_display(const ptk_ctx* c) { return c->d_display && c->disp_w == c->width && c->disp_h == c->height && c->disp_w > 0; }

extern "C" {

int ptk_display_srgb_table(float* out)
{
    if (!out) return PTK_ERR_BAD_ARG;
    std::memcpy(out, kSrgbTable, sizeof(kSrgbTable));
    return PTK_OK;
}

int ptk_display_check_params(const ptk_display_params* params) { return check_display_params(nullptr, "ptk_display_check_params", params); }

int ptk_display_planes_device(ptk_ctx* c, int width, int height, const float* d_color, const ptk_display_params* params, uint8_t* d_rgb8_out,
                              ptk_exposure_state* d_state_out)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, d_color, params, d_rgb8_out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    return display_on_stream(c, plane_source(d_color, width, height), *params, d_rgb8_out, d_state_out);
}

// The host entry: the plane and the outputs staged for the length of the call
int ptk_display_planes(ptk_ctx* c, int width, int height, const float* color, const ptk_display_params* params, uint8_t* rgb8_out,
                       ptk_exposure_state* state_out)
{
    bool nothing;
    const int rc = check_planes_args(c, width, height, color, params, rgb8_out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t px = (size_t)width * height;
    Stage s(c);
    const auto d_color = s.in(color, 3 * px);
    const auto d_rgb8 = s.out(rgb8_out, 3 * px);
    const auto d_state = s.out(state_out, 1);
    return s.run([&] { return display_on_stream(c, plane_source(d_color, width, height), *params, d_rgb8, d_state); });
}

int ptk_display_frame(ptk_ctx* c, int source, const ptk_display_params* params)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (const int rc = check_display_params(c, "ptk_display_frame", params); rc != PTK_OK) return rc;
    if (source != PTK_DISPLAY_ACCUM && source != PTK_DISPLAY_DENOISED && source != PTK_DISPLAY_TEMPORAL)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_display_frame: unknown source");
    if (!c->d_primary || !accum_ptr(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_set_frame has not been called");
    const size_t px = (size_t)c->width * c->height;
    DisplaySource src = plane_source(nullptr, c->width, c->height);
    if (source == PTK_DISPLAY_DENOISED)
    {
        if (!c->d_denoised || c->den_w != c->width || c->den_h != c->height || c->den_w == 0)
            return fail(c, PTK_ERR_BAD_ARG, "ptk_display_frame: no denoised frame at the current resolution");
        src.color = c->d_denoised;
    }
    else if (source == PTK_DISPLAY_TEMPORAL)
    {
        if (!have_temporal(c)) return fail(c, PTK_ERR_BAD_ARG, "ptk_display_frame: no temporal frame at the current resolution");
        src.color = temporal_color(c, px);
    }
    else
    {
        const bool adaptive = c->adaptive_accum && c->d_counts && c->d_moments;
        src.color = accum_ptr(c);
        src.counts = adaptive ? c->d_counts : nullptr;
        src.samples = c->samples.load(); src.rank = c->rank; src.world = c->world;
        src.kind = adaptive ? DISPLAY_SRC_ACCUM_COUNTS : DISPLAY_SRC_ACCUM_SAMPLES;
    }
    HIPCHK(c, hipSetDevice(c->device));
    if (!c->d_display) HIPCHK(c, hipMalloc(&c->d_display.p, px * 3));
    const int rc = display_on_stream(c, src, *params, c->d_display, nullptr);
    if (rc == PTK_OK) { c->disp_w = c->width; c->disp_h = c->height; }
    return rc;
}

int ptk_read_display(ptk_ctx* c, uint8_t* host_out)
{
    if (!c || !host_out) return PTK_ERR_BAD_ARG;
    if (!have_display(c)) return fail(c, PTK_ERR_BAD_ARG, "no display image at the current resolution: ptk_display_frame first");
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(host_out, c->d_display, (size_t)c->disp_w * c->disp_h * 3, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_display_device_ptr(ptk_ctx* c, void** dev_ptr, size_t* bytes)
{
    if (!c || !dev_ptr) return PTK_ERR_BAD_ARG;
    if (!have_display(c)) return fail(c, PTK_ERR_BAD_ARG, "no display image at the current resolution: ptk_display_frame first");
    *dev_ptr = c->d_display;
    if (bytes) *bytes = (size_t)c->disp_w * c->disp_h * 3;
    return PTK_OK;
}

int ptk_display_state(ptk_ctx* c, ptk_exposure_state* out)
{
    if (!c || !out) return PTK_ERR_BAD_ARG;
    std::memset(out, 0, sizeof(*out));
    if (!c->d_display_hist) return PTK_OK;       // no call yet: nothing remembered
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemcpyAsync(out, state_ptr(c), sizeof(*out), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

int ptk_display_reset(ptk_ctx* c)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->d_display_hist) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    HIPCHK(c, hipMemsetAsync(state_ptr(c), 0, sizeof(ptk_exposure_state), c->stream));
    return PTK_OK;
}

int ptk_last_display_ms(ptk_ctx* c, float* meter_ms, float* exposure_ms, float* apply_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float t[3] = { 0.0f, 0.0f, 0.0f };
    const int rc = c->ev_display.spans(c, 0, 3, t);
    if (meter_ms) *meter_ms = t[0];
    if (exposure_ms) *exposure_ms = t[1];
    if (apply_ms) *apply_ms = t[2];
    return rc;
}

}  // extern "C"
