// Irradiance probe baking (include/ptk.h ptk_bake_probes, ptk_probes_irradiance): launchers of the kernels in ptk_probes.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

#define PTK_PROBE_COEFS 9           // real spherical harmonics of bands 0..2

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

}  // namespace ptk
