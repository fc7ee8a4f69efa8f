// Host side of the ptk C-ABI: parity probes of the walk, the direct-light estimator, the kernels' arithmetic and the primary rays.
#include <hip/hip_runtime.h>

#include <vector>

#include "ptk_ctx.h"
#include "ptk_stage.h"
#include "ptk_surface.h"

using namespace ptk;

extern "C" {

int ptk_probe_hits(ptk_ctx* c, int n, const float* ro, const float* rd, int32_t* tri, float* tuv)
{
    if (!c || n < 0 || (n > 0 && (!ro || !rd || !tri || !tuv))) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)n * 3;
    Stage s(c);
    const auto d_tri = s.out(tri, (size_t)n);
    const auto d_ro = s.in(ro, n3), d_rd = s.in(rd, n3), d_tuv = s.out(tuv, n3);
    return s.run([&] {
        ProbeParams p = {};
        p.nodes = c->d_nodes; p.tris = c->d_tris; p.shade = c->d_shade; p.mats = c->d_mats;
        p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.ro = d_ro; p.rd = d_rd; p.tri = d_tri; p.tuv = d_tuv;
        p.n = n; p.num_nodes = c->num_nodes; p.scene_bound = c->scene_bound;
        launch_probe(p, c->stream);
        return s.launched();
    });
}

int ptk_probe_direct(ptk_ctx* c, int n, const float* pts, const float* normals, const float* diffuse, const float* tape3, float* out3)
{
    if (!c || n < 0 || (n > 0 && (!pts || !normals || !diffuse || !tape3 || !out3))) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n3 = (size_t)n * 3;
    Stage s(c);
    const auto d_pts = s.in(pts, n3), d_normals = s.in(normals, n3), d_diffuse = s.in(diffuse, n3), d_tape = s.in(tape3, n3), d_out = s.out(out3, n3);
    return s.run([&] {
        ProbeParams p = {};
        p.nodes = c->d_nodes; p.tris = c->d_tris; p.shade = c->d_shade; p.mats = c->d_mats;
        p.texinfo = c->d_texinfo; p.texels = c->d_texels; p.lights = c->d_lights; p.num_lights = c->num_lights;
        p.n = n; p.num_nodes = c->num_nodes; p.scene_bound = c->scene_bound;
        launch_probe_direct(p, d_pts, d_normals, d_diffuse, d_tape, d_out, c->stream);
        return s.launched();
    });
}

int ptk_probe_math(ptk_ctx* c, int op, int n, const float* in, float* out)
{
    if (!c || op < 0 || op > 7 || n < 0 || (n > 0 && (!in || !out))) return PTK_ERR_BAD_ARG;
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Stage s(c);
    const auto d_in = s.in(in, (size_t)n), d_out = s.out(out, (size_t)n);
    return s.run([&] {
        // the build the "contract" option selects for the trace kernels
        if (c->opt_contract == 1) fma::launch_probe_math(op, d_in, d_out, n, c->stream);
        else if (c->opt_contract == 2) fast::launch_probe_math(op, d_in, d_out, n, c->stream);
        else launch_probe_math(op, d_in, d_out, n, c->stream);
        return s.launched();
    });
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

// the surface sampler's table as ptk_sample_surface would use it now (built where missing or stale): incl[num_tris]
int ptk_probe_surface_table(ptk_ctx* c, uint64_t* incl)
{
    if (!c || !incl) return PTK_ERR_BAD_ARG;
    if (!c->have_scene) return fail(c, PTK_ERR_BAD_ARG, "ptk_upload_scene has not been called");
    HIPCHK(c, hipSetDevice(c->device));
    if (const int rc = ensure_surface_table(c); rc != PTK_OK) return rc;
    HIPCHK(c, hipMemcpyAsync(incl, c->d_surf_table, (size_t)c->num_tris * sizeof(uint64_t), hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return PTK_OK;
}

// the table's prefix sum (launch_scan_u64) on caller data: out[i] = in[0] + .. + in[i] mod 2^64; items_per_workgroup 0: the table's own
int ptk_probe_scan_u64(ptk_ctx* c, int32_t n, const uint64_t* in, uint64_t* out, int32_t items_per_workgroup)
{
    if (!c || n < 0 || (n > 0 && (!in || !out))) return PTK_ERR_BAD_ARG;
    const int items = items_per_workgroup == 0 ? SURF_SCAN_ITEMS : items_per_workgroup;
    if (items < 2) return fail(c, PTK_ERR_BAD_ARG, "ptk_probe_scan_u64: at least two items per workgroup");
    if (n == 0) return PTK_OK;
    HIPCHK(c, hipSetDevice(c->device));
    Buf<uint64_t> d_sums;                        // (freed behind run()'s wait for the stream)
    if (const int rc = d_sums.alloc(c, scan_u64_sums((size_t)n, items) + 1); rc != PTK_OK) return rc;
    Stage s(c);
    const auto d_in = s.in(in, (size_t)n), d_out = s.out(out, (size_t)n);
    return s.run([&] {
        launch_scan_u64(d_in, d_out, (size_t)n, items, d_sums, c->stream);
        return s.launched();
    });
}

}  // extern "C"
