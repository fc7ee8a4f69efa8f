// C wrapper over the C++ host layer — see include/ptk_host.h.
#include "ptk_host.h"

#include <algorithm>
#include <cstring>
#include <string>

#include "host_scene.h"
#include "pathtracer.h"

using namespace ptkhost;

bool ptk_write_png_rgb8_bottom_up(const char* path, const unsigned char* rgb, int w, int h);   // image.cpp

struct pth_tracer {
    PathTracer pt;
    std::string error;
};

extern "C" {

pth_tracer* pth_create(int device_ordinal)
{
    pth_tracer* t = new (std::nothrow) pth_tracer();
    if (t) t->pt.SetDevice(device_ordinal);
    return t;
}
void pth_destroy(pth_tracer* t) { delete t; }

void pth_load_object(pth_tracer* t, const char* file, const float* mm)
{
    glm::mat4 M(1.0f);
    for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) M[c][r] = mm[c * 4 + r];
    t->pt.LoadObject(file, M);
}
void pth_set_object_transform(pth_tracer* t, int obj, const float* mm)
{
    glm::mat4 M(1.0f);
    for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) M[c][r] = mm[c * 4 + r];
    t->pt.SetObjectTransform(obj, M);
}
int pth_get_object_transform(pth_tracer* t, int obj, float* mm)
{
    glm::mat4 M(1.0f);
    if (!mm || !t->pt.GetObjectTransform(obj, &M)) return 0;
    for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) mm[c * 4 + r] = M[c][r];
    return 1;
}
void pth_set_material(pth_tracer* t, int obj, int elem, const float* m)
{
    Material mat;
    mat.type = m[0] != 0.0f ? MaterialType::TRANSLUCENT : MaterialType::OPAQUE;
    mat.diffuse = glm::vec3(m[1], m[2], m[3]);
    mat.specular = glm::vec3(m[4], m[5], m[6]);
    mat.emissive = glm::vec3(m[7], m[8], m[9]);
    mat.emissiveIntensity = m[10]; mat.roughness = m[11]; mat.reflectiveness = m[12];
    mat.translucency = m[13]; mat.ior = m[14];
    t->pt.SetMaterial(obj, elem, mat);
}
void pth_set_texture(pth_tracer* t, int obj, int elem, int slot, const char* file)
{
    switch (slot)
    {
    case 0: t->pt.SetDiffuseTextureForElement(obj, elem, file); break;
    case 1: t->pt.SetNormalTextureForElement(obj, elem, file); break;
    case 2: t->pt.SetEmissTextureForElement(obj, elem, file); break;
    case 3: t->pt.SetRoughnessTextureForElement(obj, elem, file); break;
    case 4: t->pt.SetMetallicTextureForElement(obj, elem, file); break;
    case 5: t->pt.SetOpacityTextureForElement(obj, elem, file); break;
    default: break;
    }
}
void pth_build_bvh(pth_tracer* t) { t->pt.BuildBVH(); }
void pth_reset_image(pth_tracer* t) { t->pt.ResetImage(); }
void pth_clear_scene(pth_tracer* t) { t->pt.ClearScene(); }
int pth_get_samples(pth_tracer* t) { return t->pt.GetSamples(); }
int pth_get_triangle_count(pth_tracer* t) { return t->pt.GetTriangleCount(); }
int pth_get_trace_depth(pth_tracer* t) { return t->pt.GetTraceDepth(); }
void pth_set_trace_depth(pth_tracer* t, int d) { t->pt.SetTraceDepth(d); }
void pth_set_out_image(pth_tracer* t, uint8_t* out) { t->pt.SetOutImage(out); }
void pth_set_out_gl_buffer(pth_tracer* t, unsigned int gl_buffer) { t->pt.SetOutGLBuffer(gl_buffer); }
void pth_set_out_device_image(pth_tracer* t, void* device_rgb8) { t->pt.SetOutDeviceImage(device_rgb8); }
void pth_set_resolution(pth_tracer* t, int w, int h) { t->pt.SetResolution(glm::ivec2(w, h)); }
void pth_get_resolution(pth_tracer* t, int* w, int* h) { glm::ivec2 r = t->pt.GetResolution(); *w = r.x; *h = r.y; }
int pth_num_objects(pth_tracer* t) { return (int)t->pt.GetLoadedObjects().size(); }
int pth_num_elements(pth_tracer* t, int obj)
{
    auto o = t->pt.GetLoadedObjects();
    return obj >= 0 && obj < (int)o.size() ? (int)o[obj].elements.size() : 0;
}
int pth_name(pth_tracer* t, int obj, int elem, char* out, int cap)
{
    const auto objs = t->pt.GetLoadedObjects();
    if (obj < 0 || obj >= (int)objs.size() || elem >= (int)objs[obj].elements.size()) return -1;
    const std::string& n = elem < 0 ? objs[obj].name : objs[obj].elements[elem].name;
    const int len = (int)std::min<size_t>(n.size(), (size_t)std::max(cap - 1, 0));
    std::memcpy(out, n.data(), (size_t)len);
    if (cap > 0) out[len] = 0;
    return (int)n.size();
}
void pth_set_camera(pth_tracer* t, const float* p, const float* d, const float* u)
{
    t->pt.SetCamera(glm::vec3(p[0], p[1], p[2]), glm::vec3(d[0], d[1], d[2]), glm::vec3(u[0], u[1], u[2]));
}
void pth_set_projection(pth_tracer* t, float f, float fovy) { t->pt.SetProjection(f, fovy); }
void pth_set_focal_dist(pth_tracer* t, float d) { t->pt.SetCameraFocalDist(d); }
void pth_set_aperture(pth_tracer* t, float a) { t->pt.SetCameraAperture(a); }
void pth_render_frame(pth_tracer* t) { t->pt.RenderFrame(); }
void pth_exit(pth_tracer* t) { t->pt.Exit(); }

void pth_set_seed(pth_tracer* t, uint64_t seed) { t->pt.SetSeed(seed); }
void pth_set_tile(pth_tracer* t, int rank, int world) { t->pt.SetTile(rank, world); }
void pth_render_frames(pth_tracer* t, int count) { t->pt.RenderFrames(count); }
int pth_read_accum(pth_tracer* t, float* out) { return t->pt.ReadAccumulation(out) ? 1 : 0; }
int pth_render_adaptive(pth_tracer* t, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, ptk_adaptive_result* out)
{
    return t->pt.RenderAdaptive(threshold, min_spp, step, max_spp, out) ? 1 : 0;
}
int pth_read_sample_counts(pth_tracer* t, uint32_t* out) { return t->pt.ReadSampleCounts(out) ? 1 : 0; }
int pth_render_features(pth_tracer* t, uint32_t mask, uint32_t sample) { return t->pt.RenderFeatures(mask, sample) ? 1 : 0; }
int pth_read_feature(pth_tracer* t, int feature, void* out) { return t->pt.ReadFeature(feature, out) ? 1 : 0; }
int pth_pick(pth_tracer* t, int x, int y, int* obj, int* elem, int* tri) { return t->pt.Pick(x, y, obj, elem, tri) ? 1 : 0; }
int pth_trace_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, uint32_t first_sample, uint32_t spp,
                   uint32_t key_base, uint32_t flags, float* out)
{
    return t->pt.TraceRays(num_rays, origins, dirs, first_sample, spp, key_base, flags, out) ? 1 : 0;
}
int pth_intersect_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, uint32_t sample, uint32_t key_base, int32_t* tri,
                       float* thit, float* bary, int32_t* material)
{
    return t->pt.IntersectRays(num_rays, origins, dirs, sample, key_base, tri, thit, bary, material) ? 1 : 0;
}
int pth_occluded_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample, uint32_t key_base,
                      uint8_t* occluded)
{
    return t->pt.OccludedRays(num_rays, origins, dirs, tmax, sample, key_base, occluded) ? 1 : 0;
}
int pth_denoise_frame(pth_tracer* t, const ptk_denoise_params* params, int variance)
{
    return params && t->pt.DenoiseFrame(*params, variance != 0) ? 1 : 0;
}
int pth_read_denoised(pth_tracer* t, float* out) { return t->pt.ReadDenoised(out) ? 1 : 0; }
int pth_resolve_denoised(pth_tracer* t, unsigned char* out) { return t->pt.ResolveDenoised(out) ? 1 : 0; }
int pth_temporal_frame(pth_tracer* t, const ptk_temporal_params* params, int reset)
{
    return params && t->pt.TemporalFrame(*params, reset != 0) ? 1 : 0;
}
int pth_read_temporal(pth_tracer* t, float* color, float* count) { return t->pt.ReadTemporal(color, count) ? 1 : 0; }
void pth_track_motion(pth_tracer* t, int on) { t->pt.TrackMotion(on != 0); }
int pth_temporal_frame_moving(pth_tracer* t, const ptk_temporal_params* params, int reset)
{
    return params && t->pt.TemporalFrameMoving(*params, reset != 0) ? 1 : 0;
}
int pth_temporal_frame_moments(pth_tracer* t, const ptk_temporal_params* params, int reset, int moving)
{
    return params && t->pt.TemporalFrameMoments(*params, reset != 0, moving != 0) ? 1 : 0;
}
int pth_temporal_variance(pth_tracer* t, const ptk_variance_params* params) { return params && t->pt.TemporalVariance(*params) ? 1 : 0; }
int pth_read_temporal_variance(pth_tracer* t, float* moments, float* variance) { return t->pt.ReadTemporalVariance(moments, variance) ? 1 : 0; }
int pth_denoise_temporal(pth_tracer* t, const ptk_denoise_params* params, int variance)
{
    return params && t->pt.DenoiseTemporal(*params, variance != 0) ? 1 : 0;
}
int pth_display_frame(pth_tracer* t, int source, const ptk_display_params* params)
{
    return params && t->pt.DisplayFrame(source, *params) ? 1 : 0;
}
int pth_read_display(pth_tracer* t, unsigned char* out) { return t->pt.ReadDisplay(out) ? 1 : 0; }
int pth_display_state(pth_tracer* t, ptk_exposure_state* out) { return t->pt.DisplayState(out) ? 1 : 0; }
int pth_display_reset(pth_tracer* t) { return t->pt.ResetDisplay() ? 1 : 0; }
int pth_render_guides(pth_tracer* t, int width, int height) { return t->pt.RenderGuides(width, height) ? 1 : 0; }
int pth_read_guide(pth_tracer* t, int feature, void* out) { return t->pt.ReadGuide(feature, out) ? 1 : 0; }
int pth_upsample_frame(pth_tracer* t, int source, const ptk_upsample_params* params)
{
    return params && t->pt.UpsampleFrame(source, *params) ? 1 : 0;
}
int pth_read_upsampled(pth_tracer* t, float* color, int32_t* cls) { return t->pt.ReadUpsampled(color, cls) ? 1 : 0; }
int pth_read_motion(pth_tracer* t, float* prev_position, float* prev_normal, float* motion)
{
    return t->pt.ReadMotion(prev_position, prev_normal, motion) ? 1 : 0;
}
int pth_get_view(pth_tracer* t, ptk_view* out) { return t->pt.GetView(out) ? 1 : 0; }
int pth_closest_points(pth_tracer* t, int num_points, const float* points, const float* max_dist, int32_t* tri, float* dist, float* point, float* bary)
{
    return t->pt.ClosestPoints(num_points, points, max_dist, tri, dist, point, bary) ? 1 : 0;
}
int pth_crossings_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, int32_t* front, int32_t* back)
{
    return t->pt.CrossingsRays(num_rays, origins, dirs, tmax, front, back) ? 1 : 0;
}
int pth_multihit_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, int max_hits, int32_t* count,
                      int32_t* tri, float* hit_t, float* bary, int8_t* side)
{
    return t->pt.MultiHitRays(num_rays, origins, dirs, tmax, max_hits, count, tri, hit_t, bary, side) ? 1 : 0;
}
int pth_overlap_boxes(pth_tracer* t, int num, const float* lo, const float* hi, const int32_t* tri_from, int k, int32_t* count, int32_t* tris)
{
    return t->pt.OverlapBoxes(num, lo, hi, tri_from, k, count, tris) ? 1 : 0;
}
int pth_overlap_spheres(pth_tracer* t, int num, const float* centers, const float* radius, const int32_t* tri_from, int k, int32_t* count, int32_t* tris)
{
    return t->pt.OverlapSpheres(num, centers, radius, tri_from, k, count, tris) ? 1 : 0;
}
int pth_nearest_triangles(pth_tracer* t, int num_points, const float* points, const float* max_dist, int k, int32_t* count, int32_t* tri,
                          float* dist, float* point, float* bary)
{
    return t->pt.NearestTriangles(num_points, points, max_dist, k, count, tri, dist, point, bary) ? 1 : 0;
}
int pth_sample_surface(pth_tracer* t, int num_samples, uint32_t key_base, uint32_t sample, int32_t* tri, float* bary, float* position,
                       float* normal, int32_t* material)
{
    return t->pt.SampleSurface(num_samples, key_base, sample, tri, bary, position, normal, material) ? 1 : 0;
}
int pth_set_surface_weights(pth_tracer* t, const float* weights) { return t->pt.SetSurfaceWeights(weights) ? 1 : 0; }
int pth_surface_info(pth_tracer* t, uint64_t* total, int32_t* exponent, int32_t* drawable, float* max_weight)
{
    return t->pt.SurfaceInfo(total, exponent, drawable, max_weight) ? 1 : 0;
}
int pth_surface_attributes(pth_tracer* t, int num, const int32_t* tri, const float* bary, const float* dirs, int32_t* material, float* uv,
                           float* position, float* normal_geom, float* normal, float* albedo, float* emission, float* gloss, float* opacity)
{
    return t->pt.SurfaceAttributes(num, tri, bary, dirs, material, uv, position, normal_geom, normal, albedo, emission, gloss, opacity) ? 1 : 0;
}
int pth_contains_points(pth_tracer* t, int num_points, const float* points, int num_dirs, const float* dirs, int mode, uint8_t* inside, int32_t* winding)
{
    return t->pt.ContainsPoints(num_points, points, num_dirs, dirs, mode, inside, winding) ? 1 : 0;
}
int pth_signed_distance(pth_tracer* t, int num_points, const float* points, const float* max_dist, int num_dirs, const float* dirs, int mode,
                        int32_t* tri, float* dist, float* point, float* bary)
{
    return t->pt.SignedDistance(num_points, points, max_dist, num_dirs, dirs, mode, tri, dist, point, bary) ? 1 : 0;
}
int pth_bake_lightmap(pth_tracer* t, int width, int height, const float* uvs, float offset, uint32_t first_sample, uint32_t spp,
                      uint32_t key_base, uint32_t flags, float* out, int32_t* owner)
{
    return t->pt.BakeLightmap(width, height, uvs, offset, first_sample, spp, key_base, flags, out, owner) ? 1 : 0;
}
int pth_trace_rays_adaptive(pth_tracer* t, int num_rays, const float* origins, const float* dirs, float threshold, uint32_t min_spp, uint32_t step,
                            uint32_t max_spp, uint32_t key_base, uint32_t flags, float* sum, float* sumsq, uint32_t* counts, ptk_rays_adaptive_result* res)
{
    return t->pt.TraceRaysAdaptive(num_rays, origins, dirs, threshold, min_spp, step, max_spp, key_base, flags, sum, sumsq, counts, res) ? 1 : 0;
}
int pth_bake_lightmap_adaptive(pth_tracer* t, int width, int height, const float* uvs, float offset, float threshold, uint32_t min_spp, uint32_t step,
                               uint32_t max_spp, uint32_t key_base, uint32_t flags, float* out, uint32_t* counts, int32_t* owner,
                               ptk_rays_adaptive_result* res)
{
    return t->pt.BakeLightmapAdaptive(width, height, uvs, offset, threshold, min_spp, step, max_spp, key_base, flags, out, counts, owner, res) ? 1 : 0;
}
int pth_bake_coverage(pth_tracer* t, int width, int height, const float* uvs, int32_t* owner, float* bary, float* pos)
{
    return t->pt.BakeCoverage(width, height, uvs, owner, bary, pos) ? 1 : 0;
}
int pth_lightmap_dilate(pth_tracer* t, int width, int height, int passes, float* image, int32_t* owner)
{
    return t->pt.DilateLightmap(width, height, passes, image, owner) ? 1 : 0;
}
int pth_bake_probes(pth_tracer* t, int num_probes, const float* positions, int num_dirs, const float* dirs, uint32_t first_sample, uint32_t spp,
                    uint32_t key_base, uint32_t flags, float weight, float* radiance, float* coefs)
{
    return t->pt.BakeProbes(num_probes, positions, num_dirs, dirs, first_sample, spp, key_base, flags, weight, radiance, coefs) ? 1 : 0;
}
int pth_sample_probes(pth_tracer* t, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int num_points,
                      const float* points, const float* normals, float* out)
{
    return t->pt.SampleProbes(dims, origin, spacing, coefs, num_points, points, normals, out) ? 1 : 0;
}
int pth_bake_probe_visibility(pth_tracer* t, int num_probes, const float* positions, int num_dirs, const float* dirs, int res, float max_dist,
                              uint32_t sample, uint32_t key_base, float* depth, float* moments)
{
    return t->pt.BakeProbeVisibility(num_probes, positions, num_dirs, dirs, res, max_dist, depth, moments, sample, key_base) ? 1 : 0;
}
int pth_sample_probes_visible(pth_tracer* t, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int res,
                              const float* moments, float normal_bias, int num_points, const float* points, const float* normals, float* out)
{
    return t->pt.SampleProbesVisible(dims, origin, spacing, coefs, res, moments, normal_bias, num_points, points, normals, out) ? 1 : 0;
}
void pth_get_camera(pth_tracer* t, float* pos, float* dir, float* up) { t->pt.GetCamera(pos, dir, up); }
const char* pth_last_error(pth_tracer* t)
{
    std::string e = t->pt.LastError();
    if (!e.empty()) t->error = e;
    return t->error.c_str();
}
ptk_ctx* pth_context(pth_tracer* t) { return t->pt.Context(); }
const ptk_scene_desc* pth_staged_scene(pth_tracer* t) { return t->pt.StagedScene(); }

int pth_load_scene_file(pth_tracer* t, const char* path)
{
    SceneFile s; std::string err;
    if (!read_pts(path, s, &err)) { t->error = std::string(path) + ": " + err; return -1; }
    send_scene(s, t->pt);
    return 0;
}
int pth_pts_roundtrip(const char* in_path, const char* out_path)
{
    SceneFile s;
    if (!read_pts(in_path, s, 0)) return -1;
    return write_pts(out_path, s) ? 0 : -2;
}

void pth_trs_matrix(const float* loc, const float* rot, const float* scl, float* out16)
{
    glm::mat4 M = trs_matrix(loc, rot, scl);
    for (int c = 0; c < 4; c++) for (int r = 0; r < 4; r++) out16[c * 4 + r] = M[c][r];
}
void pth_euler_camera(const float* rot, float* out6) { euler_camera(rot, out6, out6 + 3); }
void pth_triangle_init(const float* in, float* out9)
{
    StagedTriangle t;
    std::memset(&t, 0, sizeof(t));
    for (int k = 0; k < 3; k++) { for (int a = 0; a < 3; a++) t.v[k][a] = in[k * 3 + a]; t.uv[k][0] = in[9 + k * 2]; t.uv[k][1] = in[10 + k * 2]; }
    triangle_init(t);
    for (int a = 0; a < 3; a++) { out9[a] = t.normal[a]; out9[3 + a] = t.tangent[a]; out9[6 + a] = t.bitangent[a]; }
}
int pth_export_png(const char* path, const uint8_t* rgb8_bottom_up, int w, int h)
{
    return ptk_write_png_rgb8_bottom_up(path, rgb8_bottom_up, w, h) ? 1 : 0;
}
static Image g_img;
int pth_image_load(const char* file, int* w, int* h)
{
    g_img.Load(file);
    *w = g_img.width(); *h = g_img.height();
    return g_img.data() ? 1 : 0;
}
void pth_image_data(uint8_t* out) { if (g_img.data()) std::memcpy(out, g_img.data(), (size_t)g_img.width() * g_img.height() * 4); }
void pth_image_tex2d(float u, float v, float* out4)
{
    glm::vec4 r = g_img.tex2D(glm::vec2(u, v));
    out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}

}  // extern "C"
