// The float form of the hemisphere sampler's angle (csrc/ptk_angle_f32.h, what the cycle unit's shade block compiles) against the
// double form as csrc/ptk_device_fn.h states it for every other kernel - restated here, operation for operation - over ALL 2^24 u01
// draws theta = i * 2^-24: the bits of ang, the quadrant k, the bits of the reduced argument r, and the bits of the sine and the
// cosine that leave sincos_2pi.  Build with -ffp-contract=off (every operation one rounding, as the kernels are built).
//   angle_f32_sweep            prints the counts; exit status 1 on any mismatch
#include <stdint.h>
#include <stdio.h>
#include <string.h>

#include "ptk_angle_f32.h"

static uint32_t bits(float x) { uint32_t u; memcpy(&u, &x, 4); return u; }

// ---- the double form: ptk_device_fn.h u01, sample_in_basis, sincos_2pi ----
#define REF_PI_D 3.14159265358979323846
static float ref_u01(uint32_t x) { return (float)(x >> 8) * 5.9604644775390625e-8f; }
static float ref_angle(float theta) { return (float)(2.0f * REF_PI_D * theta); }
static void ref_sincos_2pi(float a, int& k_out, float& r_out, float& s, float& c)
{
    int k = (int)(a * 0.636619772367581343f + 0.5f);
    float r = (float)((double)a - (double)k * 1.57079632679489661923);
    float z = r * r;
    float sp = ((-1.9515295891e-4f * z + 8.3321608736e-3f) * z - 1.6666654611e-1f) * z * r + r;
    float cp = ((2.443315711809948e-5f * z - 1.388731625493765e-3f) * z + 4.166664568298827e-2f) * z * z
               - 0.5f * z + 1.0f;
    int q = k & 3;
    float ss = (q & 1) ? cp : sp;
    float cc = (q & 1) ? sp : cp;
    s = (q & 2) ? -ss : ss;
    c = (q == 1 || q == 2) ? -cc : cc;
    k_out = k; r_out = r;
}

int main()
{
    uint64_t bad_ang = 0, bad_k = 0, bad_r = 0, bad_sin = 0, bad_cos = 0, bad_whole = 0;
    int k_max = 0;
    uint32_t first_bad = 0xffffffffu;
    for (uint32_t i = 0; i < (1u << 24); i++)
    {
        const float theta = ref_u01(i << 8);
        if (bits(theta) != bits((float)i * 5.9604644775390625e-8f)) { printf("u01 is not i * 2^-24 at %u\n", i); return 2; }
        const float a_ref = ref_angle(theta);
        int k_ref; float r_ref, s_ref, c_ref;
        ref_sincos_2pi(a_ref, k_ref, r_ref, s_ref, c_ref);

        const float a = ptk::angle_2pi_f32(theta);
        // each stage from the REFERENCE's input to it, so that one miss is counted once, where it happens ...
        const int k = ptk::angle_quadrant(a_ref);
        const float r = ptk::angle_reduce_f32(a_ref, k_ref);
        float s, c;
        ptk::sincos_reduced(k_ref, r_ref, s, c);
        // ... and the whole chain as the kernel calls it
        float sw, cw;
        ptk::sincos_2pi_theta_f32(theta, sw, cw);

        const bool miss = bits(a) != bits(a_ref) || k != k_ref || bits(r) != bits(r_ref) || bits(s) != bits(s_ref) || bits(c) != bits(c_ref) ||
                          bits(sw) != bits(s_ref) || bits(cw) != bits(c_ref);
        bad_ang += bits(a) != bits(a_ref);
        bad_k += k != k_ref;
        bad_r += bits(r) != bits(r_ref);
        bad_sin += bits(s) != bits(s_ref);
        bad_cos += bits(c) != bits(c_ref);
        bad_whole += bits(sw) != bits(s_ref) || bits(cw) != bits(c_ref);
        if (miss && first_bad == 0xffffffffu) first_bad = i;
        if (k_ref > k_max) k_max = k_ref;
    }
    printf("c_hi %a c_lo %a p1 %a p2 %a p3 %a\n", ptk::ANGLE_C_HI, ptk::ANGLE_C_LO, ptk::ANGLE_P1, ptk::ANGLE_P2, ptk::ANGLE_P3);
    printf("draws %u, largest quadrant %d\n", 1u << 24, k_max);
    printf("mismatches: ang %llu, k %llu, r %llu, sin %llu, cos %llu, whole chain %llu\n", (unsigned long long)bad_ang,
           (unsigned long long)bad_k, (unsigned long long)bad_r, (unsigned long long)bad_sin, (unsigned long long)bad_cos,
           (unsigned long long)bad_whole);
    const uint64_t bad = bad_ang + bad_k + bad_r + bad_sin + bad_cos + bad_whole;
    if (bad) { printf("first mismatch at draw %u\n", first_bad); return 1; }
    printf("ok\n");
    return 0;
}
