// Host-side check of the zero-class bodies of the FLAT pass's triangle test (pbrpathtracer_amd/csrc/ptk_flat_mt.h): for every
// built mask, the instance with the masked operations deleted against the full text (ZM = 0) on records whose masked words are
// stored zeros of either sign.  Same accept decision for both rays, same bits of t for every accepted hit, u and v equal as values;
// all-NaN directions rejected by both.  Build with -ffp-contract=off (the kernels' arithmetic); exit status 0 = no mismatch and at
// least MIN_HITS accepted hits per mask (fewer would mean the generator, not the test, is wrong).
//   g++ -O2 -std=c++17 -ffp-contract=off -I pbrpathtracer_amd/csrc tests/cpp/flat_mt_fuzz.cpp -o flat_mt_fuzz && ./flat_mt_fuzz [cases per mask]
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>

#include "ptk_flat_mt.h"

namespace {

struct F2 { float x, y; };
inline F2 operator*(F2 a, F2 b) { return F2{ a.x * b.x, a.y * b.y }; }
inline F2 operator*(F2 a, float b) { return F2{ a.x * b, a.y * b }; }
inline F2 operator*(float a, F2 b) { return F2{ a * b.x, a * b.y }; }
inline F2 operator+(F2 a, F2 b) { return F2{ a.x + b.x, a.y + b.y }; }
inline F2 operator-(F2 a, F2 b) { return F2{ a.x - b.x, a.y - b.y }; }
inline F2 operator-(F2 a) { return F2{ -a.x, -a.y }; }

const float EPS = 0.00001f;             // PTK_EPS

struct Rand {
    uint64_t s;
    uint32_t next() { s = s * 6364136223846793005ull + 1442695040888963407ull; return (uint32_t)(s >> 32); }
    float uni() { return (float)(next() >> 8) * 5.9604644775390625e-8f; }          // [0, 1)
    float sym(float r) { return (uni() * 2.0f - 1.0f) * r; }
    // a coordinate: mostly ordinary, with exact 0, -0, +-1, denormals and 2^+-60 mixed in
    float word()
    {
        const uint32_t k = next() % 40u;
        switch (k)
        {
            case 0: return 0.0f;
            case 1: return -0.0f;
            case 2: return 1.0f;
            case 3: return -1.0f;
            case 4: return 1.0e-41f;                    // denormal
            case 5: return -3.0e-42f;
            case 6: return 0x1p60f;
            case 7: return -0x1p60f;
            case 8: return 0x1p-60f;
            case 9: return -0x1p-60f;
            default: return sym(4.0f);
        }
    }
};

inline uint32_t bits(float f) { uint32_t u; std::memcpy(&u, &f, 4); return u; }

struct Tally { long cases = 0, hits = 0, bad_accept = 0, bad_t = 0, bad_uv = 0, nan_cases = 0, nan_accepted = 0; };

template <unsigned ZM>
void run_mask(int cls, long cases, uint64_t seed, bool check_uv, Tally& T)
{
    Rand R{ seed * 977u + ZM * 131u + 7u };
    const float nan = std::nanf("");
    auto rcp = [](const F2& x) { return F2{ 1.0f / x.x, 1.0f / x.y }; };
    for (long i = 0; i < cases; i++)
    {
        float e[6], v0[3], ro[3];
        for (int k = 0; k < 6; k++) e[k] = ((ZM >> k) & 1u) ? ((R.next() & 1u) ? 0.0f : -0.0f) : R.word();
        const bool tame = (R.next() & 3u) != 0u;        // three quarters: an ordinary origin and vertex, so aimed rays can hit
        for (int k = 0; k < 3; k++) { v0[k] = tame ? R.sym(4.0f) : R.word(); ro[k] = tame ? R.sym(4.0f) : R.word(); }
        float d[2][3];
        for (int r = 0; r < 2; r++)
        {
            if (R.next() & 1u)
            {
                // aimed at a point of the triangle (sometimes just outside), unit length like the kernel's directions
                const float bu = R.uni() * 1.1f - 0.05f, bv = R.uni() * (1.1f - bu) - 0.05f;
                float len2 = 0.0f;
                for (int k = 0; k < 3; k++) { d[r][k] = v0[k] + bu * e[k] + bv * e[3 + k] - ro[k]; len2 += d[r][k] * d[r][k]; }
                const float inv = 1.0f / std::sqrt(len2);
                for (int k = 0; k < 3; k++) d[r][k] *= inv;
            }
            else
                for (int k = 0; k < 3; k++) d[r][k] = R.word();
        }
        const bool all_nan = R.next() % 97u == 0u;      // normalize() of a degenerate vector: NaN in all three components
        if (all_nan) { const int r = (int)(R.next() & 1u); for (int k = 0; k < 3; k++) d[r][k] = nan; }
        const F2 dx{ d[0][0], d[1][0] }, dy{ d[0][1], d[1][1] }, dz{ d[0][2], d[1][2] };
        F2 a0, u0, w0, t0, a1, u1, w1, t1;
        ptk_mt::mt_pair<0u>(dx, dy, dz, ro[0], ro[1], ro[2], v0[0], v0[1], v0[2], e[0], e[1], e[2], e[3], e[4], e[5], rcp, a0, u0, w0, t0);
        ptk_mt::mt_pair<ZM>(dx, dy, dz, ro[0], ro[1], ro[2], v0[0], v0[1], v0[2], e[0], e[1], e[2], e[3], e[4], e[5], rcp, a1, u1, w1, t1);
        const float A0[2] = { a0.x, a0.y }, U0[2] = { u0.x, u0.y }, V0[2] = { w0.x, w0.y }, T0[2] = { t0.x, t0.y };
        const float A1[2] = { a1.x, a1.y }, U1[2] = { u1.x, u1.y }, V1[2] = { w1.x, w1.y }, T1[2] = { t1.x, t1.y };
        for (int r = 0; r < 2; r++)
        {
            const bool ok0 = ptk_mt::mt_accept(A0[r], U0[r], V0[r], U0[r] + V0[r], T0[r], EPS);
            const bool ok1 = ptk_mt::mt_accept(A1[r], U1[r], V1[r], U1[r] + V1[r], T1[r], EPS);
            T.cases++;
            if (std::isnan(d[r][0]) && std::isnan(d[r][1]) && std::isnan(d[r][2])) { T.nan_cases++; if (ok0 || ok1) T.nan_accepted++; }
            if (ok0 != ok1)
            {
                if (T.bad_accept++ < 5) std::printf("class %d mask %u: accept %d vs %d (a %a / %a, u %a / %a, v %a / %a, t %a / %a)\n", cls, ZM, ok0, ok1,
                                                    A0[r], A1[r], U0[r], U1[r], V0[r], V1[r], T0[r], T1[r]);
                continue;
            }
            if (!ok0) continue;
            T.hits++;
            if (bits(T0[r]) != bits(T1[r]) && T.bad_t++ < 5) std::printf("class %d mask %u: t %a vs %a\n", cls, ZM, T0[r], T1[r]);
            if (check_uv && !(U0[r] == U1[r] && V0[r] == V1[r]) && T.bad_uv++ < 5)
                std::printf("class %d mask %u: u %a vs %a, v %a vs %a\n", cls, ZM, U0[r], U1[r], V0[r], V1[r]);
        }
    }
}

}  // namespace

int main(int argc, char** argv)
{
    const long cases = argc > 1 ? std::atol(argv[1]) : 200000;
    const long MIN_HITS = 10000;
    int status = 0;
    // pass 0: the accept decision and the bits of t; pass 1 (other inputs): ... and u, v as values
    for (int pass = 0; pass < 2; pass++)
    {
        Tally all[ptk_mt::FLAT_ZERO_CLASSES];
#define RUN(c) run_mask<ptk_mt::flat_zero_mask(c)>(c, cases, 1000u + (uint64_t)pass, pass == 1, all[c]);
        RUN(0) RUN(1) RUN(2) RUN(3) RUN(4) RUN(5) RUN(6) RUN(7) RUN(8) RUN(9) RUN(10) RUN(11) RUN(12) RUN(13) RUN(14) RUN(15)
#undef RUN
        for (int c = 0; c < ptk_mt::FLAT_ZERO_CLASSES; c++)
        {
            const Tally& T = all[c];
            std::printf("pass %d class %2d mask %2u: %ld ray cases, %ld accepted, mismatches accept %ld t %ld uv %ld; all-NaN directions %ld, accepted %ld\n",
                        pass, c, ptk_mt::flat_zero_mask(c), T.cases, T.hits, T.bad_accept, T.bad_t, T.bad_uv, T.nan_cases, T.nan_accepted);
            if (T.bad_accept || T.bad_t || T.bad_uv || T.nan_accepted) status = 1;
            if (T.hits < MIN_HITS || T.nan_cases < 100) { std::printf("  too few accepted hits or NaN cases: the generator is wrong\n"); status = 2; }
        }
    }
    // the masks are what the header says they are: 16 distinct, the plane bits in every one above 0, never a whole edge
    for (int c = 0; c < ptk_mt::FLAT_ZERO_CLASSES; c++)
    {
        const unsigned m = ptk_mt::flat_zero_mask(c);
        int n = 0; for (int k = 0; k < 6; k++) n += (m >> k) & 1u;
        bool plane = false; for (int p = 0; p < 3; p++) plane |= (m & (9u << p)) == (9u << p);
        if (n != (c == 0 ? 0 : c < 4 ? 2 : 3) || (c > 0 && !plane) || (m & 7u) == 7u || (m & 56u) == 56u) { std::printf("mask of class %d is %u\n", c, m); status = 3; }
        for (int d = 0; d < c; d++) if (ptk_mt::flat_zero_mask(d) == m) { std::printf("classes %d and %d share mask %u\n", d, c, m); status = 3; }
    }
    std::printf(status ? "FAILED (%d)\n" : "ok\n", status);
    return status;
}
