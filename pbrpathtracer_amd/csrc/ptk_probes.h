// Irradiance probe baking and probe visibility (include/ptk.h ptk_bake_probes, ptk_probes_irradiance, ptk_bake_probe_visibility,
// ptk_probes_irradiance_visible): launchers of the kernels in ptk_probes.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

#define PTK_PROBE_COEFS 9           // real spherical harmonics of bands 0..2
#define PTK_PROBE_VIS_MAX_RES 16    // a probe's depth moments: at most 16 x 16 octahedral texels

// a regular grid of probes: probe (ix, iy, iz) has index (iz * ny + iy) * nx + ix and sits at origin + i * spacing
struct ProbeGrid {
    int dims[3];
    float origin[3];
    float spacing[3];
};

// basis[j][k] = Yk(dirs[j]), k = 0..8
void launch_probe_basis(const float* dirs, int num_dirs, float* basis, hipStream_t stream);
// the rays of num_probes whole probes: ray p * num_dirs + j = (positions[p], dirs[j])
void launch_probe_rays(const float* positions, const float* dirs, int num_probes, int num_dirs, float* origins, float* ray_dirs, hipStream_t stream);
// coefs[p][k][ch] = (sum over j ascending of radiance[p][j][ch] * basis[j][k]) * weight
void launch_probe_project(const float* radiance, const float* basis, int num_probes, int num_dirs, float weight, float* coefs, hipStream_t stream);
// out[i] = Lambertian irradiance of the trilinearly interpolated probes at (points[i], normals[i])
void launch_probe_irradiance(const ProbeGrid& grid, const float* coefs, int num_points, const float* points, const float* normals, float* out,
                             hipStream_t stream);
// moments[p][t] = the cos^32-weighted mean of min(depth[p][j], max_dist) and of its square about the direction of octahedral texel
// t of res x res, summed over j ascending; (max_dist, max_dist^2) where no direction has weight
void launch_probe_moments(const float* depth, const float* dirs, int num_probes, int num_dirs, int res, float max_dist, float* moments,
                          hipStream_t stream);
// out[i] = Lambertian irradiance at (points[i], normals[i]) of the eight corner probes, each weighted by its trilinear factor, a
// back-face term and the Chebyshev bound of its depth moments at the point pushed normal_bias along the normal
void launch_probe_irradiance_visible(const ProbeGrid& grid, const float* coefs, int res, const float* moments, float normal_bias, int num_points,
                                     const float* points, const float* normals, float* out, hipStream_t stream);

}  // namespace ptk
