/* ptk_host — C wrapper over the C++ host layer (include/pathtracer.h + the headless scene layer), so the
 * reference-compatible `PathTracer` class can be driven from C, Python (ctypes) or any other FFI.
 * One pth_tracer = one PathTracer instance = one GPU.  Functions mirror the class's methods one to
 * one (reference PathTracing/src/pathtracer.h:100-130); like them they return nothing and ignore bad
 * ids — pth_last_error() exposes the device layer's last error text.
 */
#ifndef PTK_HOST_H
#define PTK_HOST_H

#include <stdint.h>

#include "ptk.h"

#ifdef __cplusplus
extern "C" {
#endif

typedef struct pth_tracer pth_tracer;

pth_tracer* pth_create(int device_ordinal);               /* no GPU work until the first BuildBVH / render */
void pth_destroy(pth_tracer* t);

/* PathTracer API */
void pth_load_object(pth_tracer* t, const char* file, const float model_colmajor[16]);
/* SetObjectTransform (extension): stage object `obj` again under another matrix; after BuildBVH the next render call refits */
void pth_set_object_transform(pth_tracer* t, int obj, const float model_colmajor[16]);
/* GetObjectTransform (extension): the matrix object `obj` is staged under; 1 on success, 0 for a bad id */
int  pth_get_object_transform(pth_tracer* t, int obj, float model_colmajor[16]);
void pth_set_material(pth_tracer* t, int obj, int elem, const float m15[15]);  /* type, diffuse3, specular3, emissive3, I, roughness, reflectiveness, translucency, ior */
void pth_set_texture(pth_tracer* t, int obj, int elem, int slot, const char* file); /* slot 0..5: diffuse normal emissive roughness metallic opacity */
void pth_build_bvh(pth_tracer* t);
void pth_reset_image(pth_tracer* t);
void pth_clear_scene(pth_tracer* t);
int  pth_get_samples(pth_tracer* t);
int  pth_get_triangle_count(pth_tracer* t);
int  pth_get_trace_depth(pth_tracer* t);
void pth_set_trace_depth(pth_tracer* t, int depth);
void pth_set_out_image(pth_tracer* t, uint8_t* out);      /* caller-owned W*H*3 buffer (may be NULL) */
void pth_set_out_gl_buffer(pth_tracer* t, unsigned int gl_buffer);   /* SetOutGLBuffer (extension): 0 switches back */
void pth_set_out_device_image(pth_tracer* t, void* device_rgb8);      /* SetOutDeviceImage (extension): NULL switches back */
void pth_set_resolution(pth_tracer* t, int w, int h);
void pth_get_resolution(pth_tracer* t, int* w, int* h);
int  pth_num_objects(pth_tracer* t);
int  pth_num_elements(pth_tracer* t, int obj);
int  pth_name(pth_tracer* t, int obj, int elem, char* out, int cap);   /* name of object `obj` (elem < 0) or of its element; returns its length, -1 if there is none */
void pth_set_camera(pth_tracer* t, const float pos[3], const float dir[3], const float up[3]);
void pth_set_projection(pth_tracer* t, float f, float fovy);
void pth_set_focal_dist(pth_tracer* t, float d);
void pth_set_aperture(pth_tracer* t, float a);
void pth_render_frame(pth_tracer* t);
void pth_exit(pth_tracer* t);

/* extensions */
void pth_set_seed(pth_tracer* t, uint64_t seed);
void pth_set_tile(pth_tracer* t, int rank, int world);
void pth_render_frames(pth_tracer* t, int count);
int  pth_read_accum(pth_tracer* t, float* out);           /* 1 on success */
/* RenderAdaptive: 1 on success (the result may be NULL); ReadSampleCounts: W*H counts, rows bottom-up, 1 on success */
int  pth_render_adaptive(pth_tracer* t, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, ptk_adaptive_result* out);
int  pth_read_sample_counts(pth_tracer* t, uint32_t* out);
/* RenderFeatures / ReadFeature / Pick (first-hit feature planes, include/ptk.h): 1 on success; pth_pick: y from the top row,
 * obj = elem = tri = -1 where the pixel sees nothing (outputs may be NULL) */
int  pth_render_features(pth_tracer* t, uint32_t mask, uint32_t sample);
int  pth_read_feature(pth_tracer* t, int feature, void* out);
int  pth_pick(pth_tracer* t, int x, int y, int* obj, int* elem, int* tri);
/* TraceRays (radiance along caller-supplied rays, include/ptk.h ptk_trace_rays with the tracer's seed and trace depth): 1 on success */
int  pth_trace_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, uint32_t first_sample, uint32_t spp,
                    uint32_t key_base, uint32_t flags, float* out);
/* IntersectRays / OccludedRays (closest hits and occlusion along caller-supplied rays, include/ptk.h ptk_intersect_rays /
 * ptk_occluded_rays with the tracer's seed): 1 on success; tri, t, bary, material may be NULL but not all four, tmax may be NULL */
int  pth_intersect_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, uint32_t sample, uint32_t key_base,
                        int32_t* tri, float* thit, float* bary, int32_t* material);
int  pth_occluded_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample,
                       uint32_t key_base, uint8_t* occluded);
/* DenoiseFrame / ReadDenoised / ResolveDenoised (the a-trous denoiser over the frame, include/ptk.h ptk_denoise_frame; the guide
 * planes are rendered first when missing or stale): 1 on success */
int  pth_denoise_frame(pth_tracer* t, const ptk_denoise_params* params, int variance);
int  pth_read_denoised(pth_tracer* t, float* out);
int  pth_resolve_denoised(pth_tracer* t, unsigned char* out);
/* TemporalFrame / ReadTemporal / GetView (temporal reprojection of the frame, include/ptk.h ptk_temporal_frame; the guide planes are
 * rendered first when missing or stale): 1 on success; color or count may be NULL */
int  pth_temporal_frame(pth_tracer* t, const ptk_temporal_params* params, int reset);
int  pth_read_temporal(pth_tracer* t, float* color, float* count);
int  pth_get_view(pth_tracer* t, ptk_view* out);
/* TrackMotion / TemporalFrameMoving / ReadMotion (temporal reprojection over moving objects, include/ptk.h
 * ptk_temporal_frame_moving): 1 on success; any pointer of pth_read_motion may be NULL */
void pth_track_motion(pth_tracer* t, int on);
int  pth_temporal_frame_moving(pth_tracer* t, const ptk_temporal_params* params, int reset);
int  pth_read_motion(pth_tracer* t, float* prev_position, float* prev_normal, float* motion);
/* TemporalFrameMoments / TemporalVariance / ReadTemporalVariance / DenoiseTemporal (the moments of demodulated luminance through
 * the reprojection, the variance made of them and the denoiser over the temporal result; include/ptk.h ptk_temporal_frame_moments):
 * 1 on success; either pointer of pth_read_temporal_variance may be NULL */
int  pth_temporal_frame_moments(pth_tracer* t, const ptk_temporal_params* params, int reset, int moving);
int  pth_temporal_variance(pth_tracer* t, const ptk_variance_params* params);
int  pth_read_temporal_variance(pth_tracer* t, float* moments, float* variance);
int  pth_denoise_temporal(pth_tracer* t, const ptk_denoise_params* params, int variance);
/* DisplayFrame / ReadDisplay / DisplayState / ResetDisplay (the display transform over the frame, include/ptk.h ptk_display_frame;
 * source: PTK_DISPLAY_ACCUM, _DENOISED or _TEMPORAL): 1 on success */
int  pth_display_frame(pth_tracer* t, int source, const ptk_display_params* params);
int  pth_read_display(pth_tracer* t, unsigned char* out);
int  pth_display_state(pth_tracer* t, ptk_exposure_state* out);
int  pth_display_reset(pth_tracer* t);
/* RenderGuides / ReadGuide / UpsampleFrame / ReadUpsampled (guided upsampling of the frame to the resolution of guide planes of
 * their own, include/ptk.h ptk_render_guides, ptk_upsample_frame; source: PTK_UPSAMPLE_ACCUM, _DENOISED or _TEMPORAL): 1 on success;
 * either pointer of pth_read_upsampled may be NULL */
int  pth_render_guides(pth_tracer* t, int width, int height);
int  pth_read_guide(pth_tracer* t, int feature, void* out);
int  pth_upsample_frame(pth_tracer* t, int source, const ptk_upsample_params* params);
int  pth_read_upsampled(pth_tracer* t, float* color, int32_t* cls);
/* ClosestPoints (the nearest surface point to caller-supplied points, include/ptk.h ptk_closest_points): 1 on success */
int  pth_closest_points(pth_tracer* t, int num_points, const float* points, const float* max_dist, int32_t* tri, float* dist, float* point,
                        float* bary);
/* CrossingsRays / ContainsPoints / SignedDistance (crossing counts, point containment and the signed distance, include/ptk.h
 * ptk_crossings_rays, ptk_contains_points, ptk_signed_distance): 1 on success; tmax, dirs (then num_dirs = 3) and winding may be NULL */
int  pth_crossings_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, int32_t* front, int32_t* back);
int  pth_contains_points(pth_tracer* t, int num_points, const float* points, int num_dirs, const float* dirs, int mode, uint8_t* inside,
                         int32_t* winding);
int  pth_signed_distance(pth_tracer* t, int num_points, const float* points, const float* max_dist, int num_dirs, const float* dirs, int mode,
                         int32_t* tri, float* dist, float* point, float* bary);
/* MultiHitRays (the first max_hits crossings of each ray in order, include/ptk.h ptk_multihit_rays): 1 on success; tmax and any
 * output but one may be NULL */
int  pth_multihit_rays(pth_tracer* t, int num_rays, const float* origins, const float* dirs, const float* tmax, int max_hits, int32_t* count,
                       int32_t* tri, float* hit_t, float* bary, int8_t* side);
/* OverlapBoxes / OverlapSpheres (the triangles that meet each box [lo, hi] / each sphere, include/ptk.h ptk_overlap_boxes,
 * ptk_overlap_spheres): 1 on success; tri_from may be NULL, tris with k == 0, count with k > 0 */
int  pth_overlap_boxes(pth_tracer* t, int num, const float* lo, const float* hi, const int32_t* tri_from, int k, int32_t* count, int32_t* tris);
int  pth_overlap_spheres(pth_tracer* t, int num, const float* centers, const float* radius, const int32_t* tri_from, int k, int32_t* count,
                         int32_t* tris);
/* NearestTriangles (the k nearest triangles of each point in order, include/ptk.h ptk_nearest_triangles): 1 on success; max_dist
 * and any output but one may be NULL */
int  pth_nearest_triangles(pth_tracer* t, int num_points, const float* points, const float* max_dist, int k, int32_t* count, int32_t* tri,
                           float* dist, float* point, float* bary);
/* SampleSurface / SetSurfaceWeights (area-weighted points on the scene's triangles at the tracer's seed, include/ptk.h
 * ptk_sample_surface / ptk_surface_weights): 1 on success; any output and the weights may be NULL */
int  pth_sample_surface(pth_tracer* t, int num_samples, uint32_t key_base, uint32_t sample, int32_t* tri, float* bary, float* position,
                        float* normal, int32_t* material);
int  pth_set_surface_weights(pth_tracer* t, const float* weights);
int  pth_surface_info(pth_tracer* t, uint64_t* total, int32_t* exponent, int32_t* drawable, float* max_weight);
/* SurfaceAttributes (the shading data at (triangle, bary) pairs, include/ptk.h ptk_surface_attributes): 1 on success; dirs and any
 * output but one may be NULL */
int  pth_surface_attributes(pth_tracer* t, int num, const int32_t* tri, const float* bary, const float* dirs, int32_t* material, float* uv,
                            float* position, float* normal_geom, float* normal, float* albedo, float* emission, float* gloss, float* opacity);
/* BakeLightmap / BakeCoverage / DilateLightmap (lightmap baking, include/ptk.h ptk_bake_lightmap with the tracer's seed and trace
 * depth): 1 on success */
int  pth_bake_lightmap(pth_tracer* t, int width, int height, const float* uvs, float offset, uint32_t first_sample, uint32_t spp,
                       uint32_t key_base, uint32_t flags, float* out, int32_t* owner);
/* TraceRaysAdaptive / BakeLightmapAdaptive (include/ptk.h ptk_trace_rays_adaptive / ptk_bake_lightmap_adaptive with the tracer's seed
 * and trace depth): 1 on success; sumsq, owner and res may be NULL */
int  pth_trace_rays_adaptive(pth_tracer* t, int num_rays, const float* origins, const float* dirs, float threshold, uint32_t min_spp,
                             uint32_t step, uint32_t max_spp, uint32_t key_base, uint32_t flags, float* sum, float* sumsq, uint32_t* counts,
                             ptk_rays_adaptive_result* res);
int  pth_bake_lightmap_adaptive(pth_tracer* t, int width, int height, const float* uvs, float offset, float threshold, uint32_t min_spp,
                                uint32_t step, uint32_t max_spp, uint32_t key_base, uint32_t flags, float* out, uint32_t* counts,
                                int32_t* owner, ptk_rays_adaptive_result* res);
int  pth_bake_coverage(pth_tracer* t, int width, int height, const float* uvs, int32_t* owner, float* bary, float* pos);
int  pth_lightmap_dilate(pth_tracer* t, int width, int height, int passes, float* image, int32_t* owner);
/* BakeProbes / SampleProbes (irradiance probes, include/ptk.h ptk_bake_probes / ptk_probes_irradiance with the tracer's seed and
 * trace depth): 1 on success */
int  pth_bake_probes(pth_tracer* t, int num_probes, const float* positions, int num_dirs, const float* dirs, uint32_t first_sample,
                     uint32_t spp, uint32_t key_base, uint32_t flags, float weight, float* radiance, float* coefs);
int  pth_sample_probes(pth_tracer* t, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs,
                       int num_points, const float* points, const float* normals, float* out);
/* BakeProbeVisibility / SampleProbesVisible (include/ptk.h ptk_bake_probe_visibility / ptk_probes_irradiance_visible with the
 * tracer's seed): 1 on success; depth may be NULL */
int  pth_bake_probe_visibility(pth_tracer* t, int num_probes, const float* positions, int num_dirs, const float* dirs, int res, float max_dist,
                               uint32_t sample, uint32_t key_base, float* depth, float* moments);
int  pth_sample_probes_visible(pth_tracer* t, const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int res,
                               const float* moments, float normal_bias, int num_points, const float* points, const float* normals, float* out);
void pth_get_camera(pth_tracer* t, float pos[3], float dir[3], float up[3]);   /* GetCamera (extension): what SetCamera last received */
const char* pth_last_error(pth_tracer* t);
ptk_ctx* pth_context(pth_tracer* t);
const ptk_scene_desc* pth_staged_scene(pth_tracer* t);    /* flat arrays of the staged scene (host only) */

/* headless scene layer: .pts file -> PathTracer (LoadScene + SendObjectsToPathTracer + SetPathTracerCamera) */
int  pth_load_scene_file(pth_tracer* t, const char* pts_path);   /* 0 ok, <0 parse error (text via pth_last_error) */
int  pth_pts_roundtrip(const char* in_path, const char* out_path); /* read_pts + write_pts, 0 ok */

/* ExportAt (main.cpp:760-771): write the bottom-up RGB8 hand-off buffer as a top-down PNG; 1 on success */
int  pth_export_png(const char* path, const uint8_t* rgb8_bottom_up, int w, int h);

/* host-only probes (no GPU): glm-0.9.3.1-compatible TRS / Euler camera, Triangle::Init, Image */
void pth_trs_matrix(const float loc[3], const float rot_deg[3], const float scl[3], float out16[16]);
void pth_euler_camera(const float rot_deg[3], float out6[6]);
void pth_triangle_init(const float in15[15], float out9[9]);
int  pth_image_load(const char* file, int* w, int* h);    /* loads into a process-wide scratch image; 1 ok */
void pth_image_data(uint8_t* out_rgba);
void pth_image_tex2d(float u, float v, float out4[4]);

#ifdef __cplusplus
}
#endif
#endif
