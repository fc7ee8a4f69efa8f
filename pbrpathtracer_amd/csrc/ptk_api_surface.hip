// Host side of the ptk C-ABI: surface sampling - the weight table and area-weighted points on the triangles (ptk.h
// ptk_sample_surface).
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstring>
#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_surface.h"

using namespace ptk;

namespace ptk {

void surface_release(ptk_ctx* c)
{
    c->d_surf_table.release(); c->d_surf_weights.release(); c->d_surf_sums.release(); c->d_surf_red.release();
    c->surf_valid = false; c->surf_info_pending = false;
    c->ev_surf_table.begin(); c->ev_surface.begin();
}

static int ensure_surface_red(ptk_ctx* c)
{
    if (!c->d_surf_red) HIPCHK(c, hipMalloc(&c->d_surf_red.p, SURF_RED_WORDS * sizeof(uint32_t)));
    return PTK_OK;
}

// The table of the rule for the resident vertices and the weights in force, on the context's stream - behind every geometry update
// queued so far.  The one host wait is for the eight bytes that decide the exponent.
int ensure_surface_table(ptk_ctx* c)
{
    c->ev_surf_table.begin();
    if (c->surf_valid) return PTK_OK;
    const int n = c->num_tris;
    if (n <= 0 || !c->d_verts_res) return fail(c, PTK_ERR_BAD_ARG, "ptk_sample_surface: the uploaded scene has no triangles: nothing to sample");
    if (!c->d_surf_table) HIPCHK(c, hipMalloc(&c->d_surf_table.p, ((size_t)n + SURF_COARSE_WORDS) * sizeof(uint64_t)));
    if (!c->d_surf_sums) HIPCHK(c, hipMalloc(&c->d_surf_sums.p, (scan_u64_sums((size_t)n, SURF_SCAN_ITEMS) + 1) * sizeof(uint64_t)));
    if (int rc = ensure_surface_red(c); rc != PTK_OK) return rc;
    if (int rc = c->ev_surf_table.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    HIPCHK(c, hipMemsetAsync(c->d_surf_red, 0, SURF_RED_WORDS * sizeof(uint32_t), c->stream));
    launch_surface_weights(c->d_verts_res, c->d_surf_weights, n, c->d_surf_table, c->d_surf_red, c->stream);
    HIPCHK(c, hipGetLastError());
    uint32_t red[2] = { 0, 0 };
    HIPCHK(c, hipMemcpyAsync(red, c->d_surf_red, sizeof(red), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    if (red[SURF_RED_FLAG] & SURF_FLAG_WEIGHT) return fail(c, PTK_ERR_BAD_ARG, "ptk_sample_surface: a negative or non-finite weight");
    if (red[SURF_RED_FLAG] & SURF_FLAG_AREA) return fail(c, PTK_ERR_LIMIT, "ptk_sample_surface: a triangle's weight is not finite");
    float m; std::memcpy(&m, &red[SURF_RED_MAX], 4);
    if (!(m > 0.0f)) return fail(c, PTK_ERR_BAD_ARG, "ptk_sample_surface: every triangle's weight is zero: nothing to sample");
    const int E = std::ilogb(m);                                           // floor(log2 m), subnormals included
    launch_surface_quantise(c->d_surf_table, n, 35 - E, c->d_surf_red, c->stream);
    launch_scan_u64(c->d_surf_table, c->d_surf_table, (size_t)n, SURF_SCAN_ITEMS, c->d_surf_sums, c->stream);
    launch_surface_coarse(c->d_surf_table, n, c->stream);
    HIPCHK(c, hipGetLastError());
    if (int rc = c->ev_surf_table.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->surf_exponent = E; c->surf_max = m;
    c->surf_info_pending = true;
    c->surf_valid = true; c->ev_surf_table.done();
    return PTK_OK;
}

}  // namespace ptk

static int check_sample_args(ptk_ctx* c, int32_t n)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (n < 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_sample_surface: negative count");
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    return PTK_OK;
}

// The call proper, on the context's stream, every pointer into this GPU's memory; the kernel between ev_surface's two events
static int sample_on_stream(ptk_ctx* c, SurfaceSampleParams& p)
{
    c->ev_surface.begin();
    if (int rc = ensure_surface_table(c); rc != PTK_OK) return rc;
    p.incl = c->d_surf_table; p.verts = c->d_verts_res; p.shade = c->d_shade; p.num_tris = c->num_tris;
    if (int rc = c->ev_surface.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch_surface_sample(p, c->opt_surface_variant, c->stream);
    HIPCHK(c, hipGetLastError());
    if (int rc = c->ev_surface.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_surface.done();
    return PTK_OK;
}

static SurfaceSampleParams sample_params(int32_t n, uint32_t key_base, uint32_t sample, uint64_t seed, int32_t* tri, float* bary, float* position,
                                         float* normal, int32_t* material)
{
    SurfaceSampleParams p = {};
    p.num = n; p.key_base = key_base; p.sample = sample; p.seed_lo = (uint32_t)seed; p.seed_hi = (uint32_t)(seed >> 32);
    p.tri = tri; p.bary = bary; p.position = position; p.normal = normal; p.material = material;
    return p;
}

static bool bad_weight(float w) { return !(w >= 0.0f) || std::isinf(w); }

// the validated weights (device memory, or null to clear) become the context's
static int adopt_weights(ptk_ctx* c, const float* w, hipMemcpyKind kind)
{
    if (!w) { if (c->d_surf_weights) { HIPCHK(c, hipStreamSynchronize(c->stream)); c->d_surf_weights.release(); c->surf_valid = false; } return PTK_OK; }
    if (!c->d_surf_weights) HIPCHK(c, hipMalloc(&c->d_surf_weights.p, (size_t)c->num_tris * sizeof(float)));
    HIPCHK(c, hipMemcpyAsync(c->d_surf_weights, w, (size_t)c->num_tris * sizeof(float), kind, c->stream));
    if (kind == hipMemcpyHostToDevice) HIPCHK(c, hipStreamSynchronize(c->stream));     // (the caller's array is free again)
    c->surf_valid = false;
    return PTK_OK;
}

extern "C" {

int ptk_surface_weights(ptk_ctx* c, const float* w)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (w)
        for (int32_t i = 0; i < c->num_tris; i++)
            if (bad_weight(w[i])) return fail(c, PTK_ERR_BAD_ARG, "ptk_surface_weights: weight " + std::to_string(i) + " is negative or not finite");
    if (w && c->num_tris == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    return adopt_weights(c, w, hipMemcpyHostToDevice);
}

int ptk_surface_weights_device(ptk_ctx* c, const float* d_w)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (d_w && c->num_tris == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    if (d_w)
    {
        // checked where they lie, before anything of the context's changes: one word comes back, a word of its own - the other
        // words hold the table in force's build (its drawable count is read only when ptk_surface_info asks) and stay
        if (int rc = ensure_surface_red(c); rc != PTK_OK) return rc;
        uint32_t flag = 0;
        HIPCHK(c, hipMemsetAsync(c->d_surf_red + SURF_RED_CHECK, 0, sizeof(uint32_t), c->stream));
        launch_surface_check_weights(d_w, c->num_tris, c->d_surf_red + SURF_RED_CHECK, c->stream);
        HIPCHK(c, hipGetLastError());
        HIPCHK(c, hipMemcpyAsync(&flag, c->d_surf_red + SURF_RED_CHECK, sizeof(flag), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        if (flag) return fail(c, PTK_ERR_BAD_ARG, "ptk_surface_weights_device: a weight is negative or not finite");
    }
    return adopt_weights(c, d_w, hipMemcpyDeviceToDevice);
}

int ptk_sample_surface_device(ptk_ctx* c, int32_t n, uint32_t key_base, uint32_t sample, uint64_t seed, int32_t* d_tri, float* d_bary,
                              float* d_position, float* d_normal, int32_t* d_material)
{
    const int rc = check_sample_args(c, n);
    if (rc != PTK_OK || n == 0) return rc;
    if ((uintptr_t)d_bary % 8 != 0) return fail(c, PTK_ERR_BAD_ARG, "ptk_sample_surface_device: d_bary must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    SurfaceSampleParams p = sample_params(n, key_base, sample, seed, d_tri, d_bary, d_position, d_normal, d_material);
    return sample_on_stream(c, p);
}

int ptk_sample_surface(ptk_ctx* c, int32_t n, uint32_t key_base, uint32_t sample, uint64_t seed, int32_t* tri, float* bary, float* position,
                       float* normal, int32_t* material)
{
    const int rc = check_sample_args(c, n);
    if (rc != PTK_OK || n == 0) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)n;
    Stage s(c);
    const auto d_tri = s.out(tri, N), d_material = s.out(material, N);
    const auto d_bary = s.out(bary, 2 * N), d_position = s.out(position, 3 * N), d_normal = s.out(normal, 3 * N);
    return s.run([&] { return ptk_sample_surface_device(c, n, key_base, sample, seed, d_tri, d_bary, d_position, d_normal, d_material); });
}

int ptk_surface_info(ptk_ctx* c, uint64_t* total, int32_t* exponent, int32_t* drawable, float* max_weight)
{
    if (!c) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    const int was_table_timed = c->ev_surf_table.timed;
    if (int rc = ensure_surface_table(c); rc != PTK_OK) return rc;
    if (was_table_timed) c->ev_surf_table.done();
    if (c->surf_info_pending)
    {
        uint32_t dr = 0; uint64_t tot = 0;
        HIPCHK(c, hipMemcpyAsync(&dr, c->d_surf_red + SURF_RED_DRAWABLE, sizeof(dr), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipMemcpyAsync(&tot, c->d_surf_table + (c->num_tris - 1), sizeof(tot), hipMemcpyDeviceToHost, c->stream));
        HIPCHK(c, hipStreamSynchronize(c->stream));
        c->surf_drawable = (int)dr; c->surf_total = tot; c->surf_info_pending = false;
    }
    if (total) *total = c->surf_total;
    if (exponent) *exponent = c->surf_exponent;
    if (drawable) *drawable = c->surf_drawable;
    if (max_weight) *max_weight = c->surf_max;
    return PTK_OK;
}

int ptk_last_surface_ms(ptk_ctx* c, float* table_ms, float* sample_ms)
{
    if (!c) return PTK_ERR_BAD_ARG;
    float tt = 0.0f, ts = 0.0f;
    int rc = c->ev_surf_table.elapsed(c, 0, 1, &tt);
    if (rc == PTK_OK) rc = c->ev_surface.elapsed(c, 0, 1, &ts);
    if (table_ms) *table_ms = tt;
    if (sample_ms) *sample_ms = ts;
    return rc;
}

}  // extern "C"
