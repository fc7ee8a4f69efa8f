// Host side of the ptk C-ABI: surface attribute queries - the shading data at caller-supplied (triangle, bary) pairs (ptk.h
// ptk_surface_attributes).
#include <hip/hip_runtime.h>

#include <string>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_attributes.h"

using namespace ptk;

static bool any_output(const ptk_surface_attrs* o)
{
    return o && (o->material || o->uv || o->position || o->normal_geom || o->normal || o->albedo || o->emission || o->gloss || o->opacity);
}

// The shared argument checks (check_query_args); a null block of outputs counts as no output
static int check_attribute_args(ptk_ctx* c, int32_t n, const void* tri, const void* bary, const ptk_surface_attrs* out, bool* nothing)
{
    return check_query_args(c, "ptk_surface_attributes", "query count", n, tri, bary, any_output(out), nothing);
}

// The call proper, on the context's stream, every pointer into this GPU's memory; the kernel between ev_attributes' two events
static int attributes_on_stream(ptk_ctx* c, AttributeParams& p)
{
    c->ev_attributes.begin();
    p.shade = c->d_shade; p.mats = c->d_mats; p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.verts = c->d_verts_res;
    p.num_tris = c->d_verts_res ? c->num_tris : 0;
    if (int rc = c->ev_attributes.mark(c, 0, c->stream); rc != PTK_OK) return rc;
    launch_attributes(p, c->stream);
    HIPCHK(c, hipGetLastError());
    if (int rc = c->ev_attributes.mark(c, 1, c->stream); rc != PTK_OK) return rc;
    c->ev_attributes.done();
    return PTK_OK;
}

extern "C" {

int ptk_attribute_info(int attr, int* channels, int* is_int)
{
    static const int ch[PTK_ATTR_COUNT] = { 1, 2, 3, 3, 3, 3, 3, 2, 1 };
    if (attr < 0 || attr >= PTK_ATTR_COUNT) return PTK_ERR_BAD_ARG;
    if (channels) *channels = ch[attr];
    if (is_int) *is_int = attr == PTK_ATTR_MATERIAL ? 1 : 0;
    return PTK_OK;
}

int ptk_surface_attributes_device(ptk_ctx* c, int32_t n, const int32_t* d_tri, const float* d_bary, const float* d_dirs, const ptk_surface_attrs* out)
{
    bool nothing;
    const int rc = check_attribute_args(c, n, d_tri, d_bary, out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    if ((uintptr_t)d_bary % 8 != 0 || (uintptr_t)out->uv % 8 != 0 || (uintptr_t)out->gloss % 8 != 0)
        return fail(c, PTK_ERR_BAD_ARG, "ptk_surface_attributes_device: d_bary, uv and gloss must be 8-byte aligned");
    HIPCHK(c, hipSetDevice(c->device));
    AttributeParams p = {};
    p.tri = d_tri; p.bary = d_bary; p.dirs = d_dirs; p.num = n;
    p.material = out->material; p.uv = out->uv; p.position = out->position; p.normal_geom = out->normal_geom; p.normal = out->normal;
    p.albedo = out->albedo; p.emission = out->emission; p.gloss = out->gloss; p.opacity = out->opacity;
    return attributes_on_stream(c, p);
}

// The host entry: the queries and the requested outputs staged for the length of the call
int ptk_surface_attributes(ptk_ctx* c, int32_t n, const int32_t* tri, const float* bary, const float* dirs, const ptk_surface_attrs* out)
{
    bool nothing;
    const int rc = check_attribute_args(c, n, tri, bary, out, &nothing);
    if (rc != PTK_OK || nothing) return rc;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t N = (size_t)n;
    Stage s(c);
    const auto d_tri = s.in(tri, N);
    const auto d_bary = s.in(bary, 2 * N), d_dirs = s.in(dirs, 3 * N);
    const auto d_material = s.out(out->material, N);
    const auto d_uv = s.out(out->uv, 2 * N), d_position = s.out(out->position, 3 * N), d_normal_geom = s.out(out->normal_geom, 3 * N);
    const auto d_normal = s.out(out->normal, 3 * N), d_albedo = s.out(out->albedo, 3 * N), d_emission = s.out(out->emission, 3 * N);
    const auto d_gloss = s.out(out->gloss, 2 * N), d_opacity = s.out(out->opacity, N);
    return s.run([&] {
        const ptk_surface_attrs d = { d_material, d_uv, d_position, d_normal_geom, d_normal, d_albedo, d_emission, d_gloss, d_opacity };
        return ptk_surface_attributes_device(c, n, d_tri, d_bary, d_dirs, &d);
    });
}

int ptk_last_attributes_ms(ptk_ctx* c, float* ms) { return last_ms(c, &ptk_ctx::ev_attributes, ms); }

}  // extern "C"
