// Drop-in C++ host API for the MI355X render path: the public surface of the reference's
// `class PathTracer` (reference PathTracing/src/pathtracer.h:48-131), `Material` / `MaterialType`
// (mesh.h:15-59), `Image` (image.h:7-28) and `PathTracerLoader::{Object,Element}` (pathtracer.h:13-46),
// with the same names, argument meaning, call-order contract and silent error behaviour.
// The bodies stage the scene into flat arrays and call the C-ABI of include/ptk.h; the per-pixel
// render loop runs in HIP kernels on the GPU (there is no CPU render path in this library).
//
//   Load*/Set*  ->  BuildBVH()  ->  SetResolution  ->  SetOutImage  ->  ResetImage  ->  RenderFrame() x N
//
// Extensions that the reference does not have are grouped at the end of the class and marked.
#ifndef PTK_PATHTRACER_H
#define PTK_PATHTRACER_H

#include <cstdint>
#include <string>
#include <vector>

#include "ptk_glm.h"

#ifndef __glew_h__
typedef unsigned char GLubyte;   // the only thing the reference takes from <GL/glew.h> here (pathtracer.h:8,59)
#endif

struct ptk_ctx;
struct ptk_scene_desc;
struct ptk_adaptive_result;
struct ptk_rays_adaptive_result;
struct ptk_denoise_params;
struct ptk_temporal_params;
struct ptk_variance_params;
struct ptk_display_params;
struct ptk_upsample_params;
struct ptk_exposure_state;
struct ptk_view;

const float EPS = 0.00001f;      // mesh.h:12
const float INF = (float)0xFFFF; // mesh.h:13

// image.h:7-28 — RGBA8 image, longest side <= 1024 after Load (image.cpp:38-61)
class Image
{
private:
    std::string mFilename;
    int mWidth;
    int mHeight;
    unsigned char* mData;

public:
    Image();
    Image(const std::string& filename);
    ~Image();
    Image(const Image&) = delete;
    Image& operator=(const Image&) = delete;

    const int width() const;
    const int height() const;
    void Load(const std::string& filename);
    glm::vec4 tex2D(const glm::vec2& uv);   // host-side probe of the sampler semantics (image.cpp:63-86)
    unsigned char* data();
};

enum class MaterialType
{
    OPAQUE,
    TRANSLUCENT
};

// mesh.h:21-59, same field names and defaults
struct Material
{
    MaterialType type;
    glm::vec3 diffuse;
    glm::vec3 specular;
    glm::vec3 emissive;

    float emissiveIntensity;
    float roughness;
    float reflectiveness;
    float translucency;
    float ior;

    Image* diffuseTex;
    Image* normalTex;
    Image* emissTex;
    Image* roughnessTex;
    Image* metallicTex;
    Image* opacityTex;

    Material() :
        type(MaterialType::OPAQUE),
        emissiveIntensity(1.0f),
        roughness(1.0f),
        reflectiveness(0.0f),
        translucency(1.0f),
        ior(1.5f),
        diffuseTex(0),
        normalTex(0),
        emissTex(0),
        roughnessTex(0),
        metallicTex(0),
        opacityTex(0)
    {
        diffuse = glm::vec3(1.0f);
        specular = glm::vec3(1.0f);
        emissive = glm::vec3(0.0f);
    }
};

namespace PathTracerLoader
{
    struct Element
    {
        std::string name;
        Material material;
        Element() { name = ""; }
        Element(const std::string& name) { this->name = name; }
    };

    struct Object
    {
        std::string name;
        std::vector<Element> elements;
        Object() { name = ""; }
        Object(const std::string& name) { this->name = name; }
    };
}

class PathTracer
{
public:
    PathTracer();
    ~PathTracer();
    PathTracer(const PathTracer&) = delete;
    PathTracer& operator=(const PathTracer&) = delete;

    // ---- the reference's public API (pathtracer.h:100-130), unchanged ----
    void LoadObject(const std::string& file, const glm::mat4& model);

    void SetDiffuseTextureForElement(int objId, int elementId, const std::string& file);
    void SetNormalTextureForElement(int objId, int elementId, const std::string& file);
    void SetEmissTextureForElement(int objId, int elementId, const std::string& file);
    void SetRoughnessTextureForElement(int objId, int elementId, const std::string& file);
    void SetMetallicTextureForElement(int objId, int elementId, const std::string& file);
    void SetOpacityTextureForElement(int objId, int elementId, const std::string& file);

    void SetMaterial(int objId, int elementId, Material& material);

    void BuildBVH();
    void ResetImage();
    void ClearScene();

    const int GetSamples() const;
    const int GetTriangleCount() const;
    const int GetTraceDepth() const;
    void SetTraceDepth(int depth);
    void SetOutImage(GLubyte* out);
    void SetResolution(const glm::ivec2& res);
    const glm::ivec2 GetResolution() const;
    std::vector<PathTracerLoader::Object> GetLoadedObjects() const;

    void SetCamera(const glm::vec3& pos, const glm::vec3& dir, const glm::vec3& up);
    void SetProjection(float f, float fovy);
    void SetCameraFocalDist(float dist);
    void SetCameraAperture(float aperture);
    void RenderFrame();
    void Exit();

    // ---- extensions (not in the reference) ----
    // The reference seeds one std::mt19937 from std::random_device (pathtracer.cpp:11); here the RNG
    // is counter-based and keyed on (seed, pixel, sample index), default seed 0.
    void SetSeed(uint64_t seed);
    // Moves a loaded object: its triangles are staged again under `model` from the object-space data kept at LoadObject, bit for
    // bit what LoadObject(file, model) stages.  Before BuildBVH() this changes what will be built.  After BuildBVH() the next
    // RenderFrame() / RenderFeatures() / Pick() / RenderAdaptive() sends the object's triangle range to the device
    // (ptk_update_geometry, include/ptk.h): records are rewritten and the BVH refitted in place, no rebuild.  The image is not
    // reset (ResetImage() stays the caller's) and the light list stays BuildBVH's.  A bad id is ignored.
    void SetObjectTransform(int objId, const glm::mat4& model);
    // The matrix object `objId` is staged under: LoadObject's, or the last SetObjectTransform's.  false for a bad id.
    bool GetObjectTransform(int objId, glm::mat4* model);
    // EXPERIMENTAL (never executed: headless build boxes).  SetOutImage for a display path that stays on the GPU: the 8-bit image
    // (the layout of texData) is written into this OpenGL buffer object - the viewer's GL_PIXEL_UNPACK_BUFFER - instead of a host
    // buffer.  Call it on the thread whose OpenGL context is current (the viewer's GUI thread): the buffer is registered HERE
    // (ptk_bind_gl_buffer, include/ptk.h), not inside RenderFrame(), which the viewer runs on a thread without a context; the call
    // waits for a RenderFrame() in flight.  Read the buffer only between two RenderFrame() calls.  0 lets it go (same thread).
    void SetOutGLBuffer(unsigned int gl_buffer);
    // ... or into W*H*3 bytes of this GPU's memory (ptk_bind_out_device); NULL or SetOutImage(ptr) switches back.
    void SetOutDeviceImage(void* device_rgb8);
    // One process per GPU: which device this instance drives, and which 16x16 pixel tiles it owns.
    void SetDevice(int ordinal);
    void SetTile(int rank, int world);
    // `count` RenderFrame() calls in one kernel launch (identical image; the accumulator stays in
    // registers between samples).  The RGB8 host copy happens once at the end.
    void RenderFrames(int count);
    // Adaptive render (include/ptk.h ptk_render_adaptive): ResetImage(), then rounds of `step` samples; a pixel stops once its
    // noise meets `threshold` (from min_spp on) or at max_spp.  Each pixel then holds exactly what a plain render of its own
    // sample count puts there; RenderFrame() refuses to add to it until ResetImage().
    // The result (rounds, max_count, pixel_samples, active_pixels) goes to *out when it is not NULL.
    bool RenderAdaptive(float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp, ptk_adaptive_result* out = nullptr);
    // samples per pixel (W*H, rows bottom-up, 0 = not owned)
    bool ReadSampleCounts(uint32_t* out);
    // First-hit feature planes (include/ptk.h ptk_render_features: depth, ids, normals, albedo ... of what each pixel's camera ray
    // sees with the lens closed): computes the planes of `mask` (bit k = PTK_FEAT_k) for sample `sample` of the class's seed.
    // Pending material / camera / resolution edits apply as for RenderFrame(); the image and the sample count are not touched.
    bool RenderFeatures(uint32_t mask, uint32_t sample = 0);
    // one plane of the last RenderFeatures(): W*H*channels elements of 4 bytes (ptk_feature_info), rows bottom-up
    bool ReadFeature(int feature, void* out);
    // Extensions: the a-trous denoiser over the frame as last rendered (include/ptk.h ptk_denoise_frame; variance: the
    // variance-guided mode, legal after RenderAdaptive()).  A convenience over the C-ABI call: the five guide planes (TRIANGLE,
    // POSITION, NORMAL, ALBEDO, EMISSION) are rendered first - sample 0 of the class's seed, replacing the planes of an earlier
    // RenderFeatures() - when they are missing or older than the last scene, camera, resolution or seed change a render call
    // applied.  Pending edits are NOT applied: the accumulator does not hold them either.  The image, the sample count and the
    // hand-off buffer are not touched.  ReadDenoised: W*H*3 floats, rows bottom-up; ResolveDenoised: W*H*3 bytes, the layout of
    // the out image.
    bool DenoiseFrame(const ptk_denoise_params& params, bool variance = false);
    bool ReadDenoised(float* out);
    bool ResolveDenoised(GLubyte* out);
    // Extensions: temporal reprojection of the frame as last rendered (include/ptk.h ptk_temporal_frame): the result of the previous
    // TemporalFrame() is carried into the current camera's frame and blended with it by sample counts; reset drops that history.
    // The use: after a camera move ResetImage(), a few RenderFrame()s, TemporalFrame(), then DenoiseFrame() or the planes denoiser
    // over the result.  The guide planes are rendered first, as DenoiseFrame() does it, when MATERIAL, POSITION or NORMAL is missing
    // or stale (the denoiser's five come along, so that the two calls share one set).  Pending edits are NOT applied; the image,
    // the sample count and the hand-off buffer are not touched.  ReadTemporal: W*H*3 floats and W*H floats (the samples behind
    // each pixel), rows bottom-up, either may be NULL.  GetView: the image-plane set-up of the device layer's current camera and
    // resolution (ptk_get_view).
    bool TemporalFrame(const ptk_temporal_params& params, bool reset = false);
    bool ReadTemporal(float* color, float* count);
    bool GetView(ptk_view* out);
    // Extensions: temporal reprojection over objects that move (include/ptk.h ptk_temporal_frame_moving).  TrackMotion(true): the
    // render call that applies SetObjectTransform() edits first keeps the resident geometry (ptk_geometry_snapshot) - once per
    // TemporalFrame*() call, ahead of the first batch of edits after it, so that several batches between two temporal calls keep
    // the geometry that matches the history.  TemporalFrameMoving() is TemporalFrame() whose history follows the moved triangles;
    // it renders the guide planes (TemporalFrame()'s with BARY) when they are missing or stale, shares history, result and
    // ReadTemporal with TemporalFrame(), and the two may alternate.  ReadMotion: where each pixel's surface point was in the
    // history's geometry (W*H*3 floats), its normal there (W*H*3) and its screen-space motion vector under the history's view
    // (W*H*2: columns, top-down rows; NaN where the pixel sees nothing or there was no history), rows bottom-up, any may be NULL.
    void TrackMotion(bool on);
    bool TemporalFrameMoving(const ptk_temporal_params& params, bool reset = false);
    bool ReadMotion(float* prev_position, float* prev_normal, float* motion);
    // Extensions: the temporal half of SVGF up to the filter (include/ptk.h ptk_temporal_frame_moments, ptk_temporal_variance,
    // ptk_denoise_temporal).  TemporalFrameMoments() is TemporalFrame() - moving: TemporalFrameMoving() - that also carries the
    // first and second moment of demodulated luminance; it shares history, result and ReadTemporal with the two, but a moments
    // call behind a plain one starts its history over.  It renders the guide planes (that call's with ALBEDO; TRIANGLE and
    // EMISSION come along for DenoiseTemporal()) when they are missing or stale.  TemporalVariance(): the per-pixel variance of
    // the accumulated value from those moments.  ReadTemporalVariance: W*H*2 floats and W*H floats, rows bottom-up, either may be
    // NULL.  DenoiseTemporal(): the a-trous filter over the temporal result on the device - variance: guided by
    // TemporalVariance()'s plane - into the plane ReadDenoised and ResolveDenoised serve.  Pending edits are NOT applied; the
    // image, the sample count and the hand-off buffer are not touched.
    bool TemporalFrameMoments(const ptk_temporal_params& params, bool reset = false, bool moving = false);
    bool TemporalVariance(const ptk_variance_params& params);
    bool ReadTemporalVariance(float* moments, float* variance);
    bool DenoiseTemporal(const ptk_denoise_params& params, bool variance = true);
    // Extensions: the display transform (include/ptk.h ptk_display_frame) - exposure, given or metered from a luminance histogram
    // and adapted from call to call on the device, a tone curve and the sRGB transfer function - over the frame as last rendered
    // (source PTK_DISPLAY_ACCUM), the DenoiseFrame() / DenoiseTemporal() result (PTK_DISPLAY_DENOISED) or the TemporalFrame*()
    // result (PTK_DISPLAY_TEMPORAL); false when the source does not exist at the current resolution.  ReadDisplay: W*H*3 bytes,
    // the layout of the out image.  DisplayState: the exposure state behind the last call.  ResetDisplay forgets it.  Pending
    // edits are NOT applied; the image, the sample count and the hand-off buffer (SetOutImage) are not touched.
    bool DisplayFrame(int source, const ptk_display_params& params);
    bool ReadDisplay(GLubyte* out);
    bool DisplayState(ptk_exposure_state* out);
    bool ResetDisplay();
    // Extensions: guided upsampling (include/ptk.h ptk_render_guides, ptk_upsample_frame) - trace at a low resolution, show at a
    // higher one.  RenderGuides: the first-hit planes MATERIAL, POSITION, NORMAL and ALBEDO of the current camera at width x height,
    // whatever SetResolution set (sample 0 of the seed).  ReadGuide: one of them, width*height elements of the feature's type, rows
    // bottom-up.  UpsampleFrame: the frame as last rendered (source PTK_UPSAMPLE_ACCUM), the DenoiseFrame() / DenoiseTemporal()
    // result (PTK_UPSAMPLE_DENOISED) or the TemporalFrame*() result (PTK_UPSAMPLE_TEMPORAL) up to the guides' resolution; the
    // frame's own guide planes are rendered first when missing or stale.  False without RenderGuides, when the two resolutions
    // differ in aspect ratio or the source does not exist.  ReadUpsampled: width*height*3 floats and width*height classes (0
    // bilinear, 1 wide ring, 2 a hole that holds the nearest low pixel), either may be NULL.  Pending edits are NOT applied; the
    // image, the sample count and the hand-off buffer are not touched.
    bool RenderGuides(int width, int height);
    bool ReadGuide(int feature, void* out);
    bool UpsampleFrame(int source, const ptk_upsample_params& params);
    bool ReadUpsampled(float* color, int32_t* cls);
    // The (object, element) under pixel (x, y), y counted from the top row: one ray (ptk_pick), pending edits applied first.
    // A pixel that sees nothing gives -1 / -1 (and triangle -1) and true; false: no scene / resolution yet, or (x, y) outside the frame.
    bool Pick(int x, int y, int* objId, int* elementId, int* triangle = nullptr);
    // Radiance along caller-supplied rays (include/ptk.h ptk_trace_rays, host arrays, synchronous): out[i] = the float32 in-order
    // sum over samples [first_sample, first_sample + spp) of what Trace returns for the ray (origins[i], dirs[i]) - unit
    // directions - at the class's trace depth, on the streams of (the class's seed, RNG pixel key_base + i, sample);
    // flags = PTK_RAYS_ACCUMULATE | PTK_RAYS_LENS_DRAWS.  Valid after BuildBVH(): needs neither a resolution nor a camera; pending
    // material and geometry edits apply as for RenderFrame(); the image and the sample count are not touched.
    bool TraceRays(int num_rays, const float* origins, const float* dirs, uint32_t first_sample, uint32_t spp, uint32_t key_base,
                   uint32_t flags, float* out);
    // Extensions: closest-hit and occlusion queries for caller-supplied rays (include/ptk.h ptk_intersect_rays / ptk_occluded_rays,
    // host arrays, synchronous) with the opacity draws of sample `sample` at the class's seed and RNG pixel key_base + i.  tri, t,
    // bary (2 per ray) and material may each be null, not all four; tmax null: +inf; directions are used as given, t in units of
    // |dir|.  Valid after BuildBVH() with no resolution set; pending material and geometry edits apply as for TraceRays; the image
    // and the sample count are not touched.
    bool IntersectRays(int num_rays, const float* origins, const float* dirs, uint32_t sample, uint32_t key_base, int32_t* tri, float* t,
                       float* bary, int32_t* material);
    bool OccludedRays(int num_rays, const float* origins, const float* dirs, const float* tmax, uint32_t sample, uint32_t key_base,
                      uint8_t* occluded);
    // Extension: closest-point queries (include/ptk.h ptk_closest_points, host arrays, synchronous): for each of the points the
    // nearest point of the scene's surface strictly nearer than max_dist[i] (null: no bound).  tri, dist, point (3 per point) and
    // bary (2 per point) may each be null, not all four.  A geometric query: seed and materials take no part.  Valid after
    // BuildBVH() with no resolution set; pending geometry edits apply as for TraceRays; the image and the sample count are not touched.
    bool ClosestPoints(int num_points, const float* points, const float* max_dist, int32_t* tri, float* dist, float* point, float* bary);
    // Extensions: crossing counts, point containment and a signed distance (include/ptk.h ptk_crossings_rays, ptk_contains_points,
    // ptk_signed_distance, host arrays, synchronous).  CrossingsRays: how many triangles each ray crosses before tmax[i] (null: no
    // bound) from their front and from their back; either output may be null, not both.  ContainsPoints: inside[i] = the majority
    // vote of num_dirs rays from the point (dirs null: the built-in three, num_dirs 3; mode PTK_INSIDE_WINDING or _PARITY), winding
    // (num_dirs per point) may be null.  SignedDistance: ClosestPoints with the sign bit of dist set inside.  Geometric queries:
    // seed and materials take no part.  Valid after BuildBVH() with no resolution set; pending geometry edits apply as for
    // TraceRays; the image and the sample count are not touched.
    bool CrossingsRays(int num_rays, const float* origins, const float* dirs, const float* tmax, int32_t* front, int32_t* back);
    bool ContainsPoints(int num_points, const float* points, int num_dirs, const float* dirs, int mode, uint8_t* inside, int32_t* winding);
    bool SignedDistance(int num_points, const float* points, const float* max_dist, int num_dirs, const float* dirs, int mode, int32_t* tri,
                        float* dist, float* point, float* bary);
    // Extension: ordered multi-hit queries (include/ptk.h ptk_multihit_rays, host arrays, synchronous): the first max_hits (1 .. 16)
    // triangles each ray crosses before tmax[i] (null: no bound), ascending by (t, triangle index).  count: 1 per ray; tri, t and
    // side: max_hits per ray; bary: 2 * max_hits per ray; each may be null, not all five.  A geometric query: seed and materials
    // take no part.  Valid after BuildBVH() with no resolution set; pending geometry edits apply as for CrossingsRays; the image and
    // the sample count are not touched.
    bool MultiHitRays(int num_rays, const float* origins, const float* dirs, const float* tmax, int max_hits, int32_t* count, int32_t* tri,
                      float* t, float* bary, int8_t* side);
    // Extension: overlap queries (include/ptk.h ptk_overlap_boxes, ptk_overlap_spheres, host arrays, synchronous): for each closed
    // box [lo, hi] / each sphere the number of triangles with index >= tri_from[i] (null: 0) that meet it, and the k (0 .. 16)
    // smallest of their indices, -1 behind the last.  count: 1 per query, may be null with k > 0; tris: k per query, may be null
    // with k == 0.  A geometric query: seed and materials take no part.  Valid after BuildBVH() with no resolution set; pending
    // geometry edits apply as for ClosestPoints; the image and the sample count are not touched.
    bool OverlapBoxes(int num, const float* lo, const float* hi, const int32_t* tri_from, int k, int32_t* count, int32_t* tris);
    bool OverlapSpheres(int num, const float* centers, const float* radius, const int32_t* tri_from, int k, int32_t* count, int32_t* tris);
    // Extension: K-nearest triangle queries (include/ptk.h ptk_nearest_triangles, host arrays, synchronous): for each of the points
    // the k (1 .. 16) nearest triangles within max_dist[i] (null: no bound), ascending by (distance, index) under ClosestPoints' rule.
    // count: 1 per point; tri, dist: k per point; point: 3 k; bary: 2 k; behind count -1, +inf, 0, 0.  Any output but one may be
    // null.  A geometric query: seed and materials take no part.  Valid after BuildBVH() with no resolution set; pending geometry
    // edits apply as for ClosestPoints; the image and the sample count are not touched.
    bool NearestTriangles(int num_points, const float* points, const float* max_dist, int k, int32_t* count, int32_t* tri, float* dist,
                          float* point, float* bary);
    // Extension: surface sampling (include/ptk.h ptk_sample_surface / ptk_surface_weights, host arrays, synchronous) at the class's
    // seed: num_samples points of the scene's surface, a triangle drawn in proportion to its area times its weight, the point
    // uniform on it; sample j is a function of (seed, key_base + j, sample) and the scene alone.  tri, material: 1 per sample; bary:
    // 2; position, normal: 3; each may be null.  SetSurfaceWeights: one weight per triangle, finite and >= 0, or null for the areas
    // alone; BuildBVH() drops them.  Valid after BuildBVH() with no resolution set; pending SetObjectTransform edits apply first, as
    // for the other queries; the image and the sample count are not touched.
    bool SampleSurface(int num_samples, uint32_t key_base, uint32_t sample, int32_t* tri, float* bary, float* position, float* normal,
                       int32_t* material);
    bool SetSurfaceWeights(const float* weights);
    // ... and the sampling table in force (ptk_surface_info): the sum of the quantised weights, the exponent E, the triangles that
    // can be drawn and the largest weight; each may be null
    bool SurfaceInfo(uint64_t* total, int32_t* exponent, int32_t* drawable, float* max_weight);
    // Extension: surface attribute queries (include/ptk.h ptk_surface_attributes, host arrays, synchronous): what is AT the surface
    // points (tri[i], bary[i] = u, v) the queries above answer with - material: 1 per query; uv, gloss: 2; position, normal_geom,
    // normal, albedo, emission: 3; opacity: 1; each may be null, but not all.  dirs (3 per query, may be null): the direction each
    // point is seen along; the shading normal is flipped against it.  A triangle index outside the scene - a missed ray's -1 - gives
    // material -1 and zeros.  Valid after BuildBVH() with no resolution set; pending material and geometry edits apply as for
    // TraceRays; the image and the sample count are not touched.
    bool SurfaceAttributes(int num, const int32_t* tri, const float* bary, const float* dirs, int32_t* material, float* uv, float* position,
                           float* normal_geom, float* normal, float* albedo, float* emission, float* gloss, float* opacity);
    // Extensions: lightmap baking (include/ptk.h ptk_bake_lightmap / ptk_bake_coverage / ptk_lightmap_dilate, host arrays,
    // synchronous) at the class's seed and trace depth.  uvs: [triangles][6] chart corners, or null for the scene's own uvs;
    // out: width*height*3 floats, rows bottom-up; owner (may be null): width*height triangle indices, -1 uncovered;
    // flags = PTK_BAKE_ACCUMULATE | PTK_BAKE_BACK.  Valid after BuildBVH() with no resolution set; pending material and geometry
    // edits apply as for TraceRays; the image and the sample count are not touched.
    bool BakeLightmap(int width, int height, const float* uvs, float offset, uint32_t first_sample, uint32_t spp, uint32_t key_base,
                      uint32_t flags, float* out, int32_t* owner = nullptr);
    // Extensions: the adaptive forms (include/ptk.h ptk_trace_rays_adaptive / ptk_bake_lightmap_adaptive, host arrays, synchronous)
    // at the class's seed and trace depth: rounds of `step` samples until a ray's / texel's noise meets `threshold`, or max_spp.
    // sum / out: the float32 sums, counts: the samples each ray / texel received (mean = sum / count); sumsq, owner, res may be
    // null.  flags = PTK_RAYS_LENS_DRAWS / PTK_BAKE_BACK.  Pending edits apply as for TraceRays; the image is not touched.
    bool TraceRaysAdaptive(int num_rays, const float* origins, const float* dirs, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp,
                           uint32_t key_base, uint32_t flags, float* sum, float* sumsq, uint32_t* counts, ptk_rays_adaptive_result* res = nullptr);
    bool BakeLightmapAdaptive(int width, int height, const float* uvs, float offset, float threshold, uint32_t min_spp, uint32_t step, uint32_t max_spp,
                              uint32_t key_base, uint32_t flags, float* out, uint32_t* counts, int32_t* owner = nullptr,
                              ptk_rays_adaptive_result* res = nullptr);
    bool BakeCoverage(int width, int height, const float* uvs, int32_t* owner, float* bary = nullptr, float* pos = nullptr);
    bool DilateLightmap(int width, int height, int passes, float* image, int32_t* owner);
    // Extensions: irradiance probe baking (include/ptk.h ptk_bake_probes / ptk_probes_irradiance, host arrays, synchronous) at the
    // class's seed and trace depth.  positions: num_probes*3 floats; dirs: num_dirs*3 floats, used as given; radiance (may be null
    // unless flags has PTK_PROBES_ACCUMULATE): num_probes*num_dirs*3 sums; coefs: num_probes*27 floats.  Valid after BuildBVH() with
    // no resolution set; pending material and geometry edits apply as for TraceRays; the image and the sample count are not touched.
    bool BakeProbes(int num_probes, const float* positions, int num_dirs, const float* dirs, uint32_t first_sample, uint32_t spp,
                    uint32_t key_base, uint32_t flags, float weight, float* radiance, float* coefs);
    // out[i] = the irradiance the probe grid (dims, origin, spacing; coefs as BakeProbes wrote them for its probes in x-fastest
    // order) gives at (points[i], normals[i]); needs no scene
    bool SampleProbes(const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int num_points,
                      const float* points, const float* normals, float* out);
    // Extensions: probe visibility (include/ptk.h ptk_bake_probe_visibility / ptk_probes_irradiance_visible, host arrays,
    // synchronous) at the class's seed.  depth (may be null): num_probes*num_dirs distances, +inf on a miss; moments:
    // num_probes*res*res*2 floats.  Valid after BuildBVH() with no resolution set; pending edits apply as for TraceRays.
    bool BakeProbeVisibility(int num_probes, const float* positions, int num_dirs, const float* dirs, int res, float max_dist, float* depth,
                             float* moments, uint32_t sample = 0, uint32_t key_base = 0);
    // SampleProbes with every corner probe weighted by its visibility from the point pushed normal_bias along its normal
    bool SampleProbesVisible(const int32_t dims[3], const float origin[3], const float spacing[3], const float* coefs, int res, const float* moments,
                             float normal_bias, int num_points, const float* points, const float* normals, float* out);
    // the camera as SetCamera last received it (position, direction, up; not normalised), 3 floats each
    void GetCamera(float* pos, float* dir, float* up) const;
    // mTotalImg (float RGB, rows bottom-up), W*H*3 floats
    bool ReadAccumulation(float* out);
    // last error text of the device layer ("" when none); the reference API itself stays silent
    std::string LastError() const;
    ptk_ctx* Context();
    // the staged scene as the flat arrays BuildBVH() uploads (include/ptk.h); valid until the scene changes
    const ptk_scene_desc* StagedScene();

    struct Impl;
private:
    Impl* m;
};

#endif
