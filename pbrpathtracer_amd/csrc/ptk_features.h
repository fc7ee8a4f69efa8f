// First-hit feature planes and picking (include/ptk.h ptk_render_features, ptk_pick): parameter block and launchers of the kernels
// in ptk_features.hip.
#pragma once

#include "ptk_device.h"

namespace ptk {

// One SoA plane per feature, [H][W][channels], rows bottom-up.  A null plane is not computed; the mask is the same for every
// wave of the launch.
constexpr int NUM_FEATURES = 10;
struct FeatureParams {
    float* depth;               // 0
    int32_t* triangle;          // 1
    int32_t* material;          // 2
    float* bary;                // 3  x2
    float* position;            // 4  x3
    float* normal_geom;         // 5  x3
    float* normal;              // 6  x3
    float* albedo;              // 7  x3
    float* emission;            // 8  x3
    float* gloss;               // 9  x2
    uint32_t sample;            // the sample whose opacity draws decide the hit
    uint32_t seed_lo, seed_hi;
};

void launch_features(const RenderParams& p, const FeatureParams& f, int owned_tiles, hipStream_t stream);
// the feature ray of ONE pixel (top-down index) for f.sample of the seed in f: out3[0] = triangle (-1: nothing), out3[1] = its
// material index (-1), out3[2] = the bits of t (+inf)
void launch_pick(const RenderParams& p, const FeatureParams& f, int pixel, int32_t* out3, hipStream_t stream);

}  // namespace ptk
