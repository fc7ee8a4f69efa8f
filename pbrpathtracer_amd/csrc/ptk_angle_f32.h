// The hemisphere sampler's angle and its sine / cosine: ang = 2 pi theta for a u01 draw theta, sincos_2pi(ang).  The one statement of
// the polynomial and the quadrant selects (every kernel's sincos_2pi, ptk_device_fn.h, ends in sincos_reduced), and of a FLOAT form of
// what comes before them, compiled by the cycle unit's shade block and by the host-side sweep (tests/cpp/angle_f32_sweep.cpp).  Plain
// C++: no HIP header, so a host compiler takes it as it stands.  Build with -ffp-contract=off: every operation below is one rounding.
//
// The double form (ptk_device_fn.h sample_in_basis / sincos_2pi, the oracle's sample_about) is
//   ang = (float)(2 pi_d * (double)theta),   k = (int)(ang * (2 / pi) + 0.5f),   r = (float)((double)ang - (double)k * (pi / 2)_d)
// - on gfx950 eight f64-class instructions.  theta is a u01 draw, i * 2^-24 with i < 2^24, and the sampler is the one caller, so the
// chain is a function of 24 bits, and over all 2^24 of them the float form below gives the same bits of ang, the same k and the same
// bits of r (the sweep holds it to zero mismatches; k never exceeds 4):
//   ang = fma(theta, c_hi, theta * c_lo)                       c_hi + c_lo: 2 pi_d in two floats, the small product rounded first
//   r   = fma(-k, p3, fma(-k, p2, fma(-k, p1, ang)))           p1 + p2 + p3: (pi / 2)_d in three floats (Cody-Waite)
// Forms that were swept and miss: two pieces of pi / 2 (once), fma(theta, c_lo, theta * c_hi) (5.5 M times).  Outside the draws'
// 2^24 values nothing is claimed: no other caller may use the float form.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define PTK_ANGLE_FN __host__ __device__ inline __attribute__((always_inline))
#else
#define PTK_ANGLE_FN inline
#endif

namespace ptk {

constexpr double ANGLE_PI_D = 3.14159265358979323846;
constexpr double ANGLE_2PI_D = 2.0 * ANGLE_PI_D, ANGLE_PIO2_D = 1.57079632679489661923;
constexpr float ANGLE_C_HI = (float)ANGLE_2PI_D;
constexpr float ANGLE_C_LO = (float)(ANGLE_2PI_D - (double)ANGLE_C_HI);
constexpr float ANGLE_P1 = (float)ANGLE_PIO2_D;
constexpr float ANGLE_P2 = (float)(ANGLE_PIO2_D - (double)ANGLE_P1);
constexpr float ANGLE_P3 = (float)(ANGLE_PIO2_D - (double)ANGLE_P1 - (double)ANGLE_P2);

// (float)(2 pi_d * theta) for a u01 draw theta
PTK_ANGLE_FN float angle_2pi_f32(float theta) { return __builtin_fmaf(theta, ANGLE_C_HI, theta * ANGLE_C_LO); }

// the quadrant of a in [0, 2 pi]: what every form of the reduction starts from
PTK_ANGLE_FN int angle_quadrant(float a) { return (int)(a * 0.636619772367581343f + 0.5f); }

// (float)((double)a - (double)k * (pi / 2)_d) for a = angle_2pi_f32(theta), k = angle_quadrant(a)
PTK_ANGLE_FN float angle_reduce_f32(float a, int k)
{
    const float nk = -(float)k;
    return __builtin_fmaf(nk, ANGLE_P3, __builtin_fmaf(nk, ANGLE_P2, __builtin_fmaf(nk, ANGLE_P1, a)));
}

// sine and cosine of k * pi / 2 + r from the reduced argument: fixed polynomial shared (by construction, not by source) with the oracle
PTK_ANGLE_FN void sincos_reduced(int k, float r, float& s, float& c)
{
    float z = r * r;
    float sp = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
    float cp = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z
               - 0.5f * z + 1.0f;
    int q = k & 3;
    float ss = (q & 1) ? cp : sp;
    float cc = (q & 1) ? sp : cp;
    s = (q & 2) ? -ss : ss;
    c = (q == 1 || q == 2) ? -cc : cc;
}

// sincos_2pi(angle_2pi_f32(theta)) without a double: the cycle unit's form
PTK_ANGLE_FN void sincos_2pi_theta_f32(float theta, float& s, float& c)
{
    const float a = angle_2pi_f32(theta);
    const int k = angle_quadrant(a);
    sincos_reduced(k, angle_reduce_f32(a, k), s, c);
}

}  // namespace ptk
