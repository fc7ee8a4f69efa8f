// Exhaustive proof (all 2^32 float bit patterns, on the GPU the kernels run on) that the short reciprocal / square-root
// sequences of ptk_kernels.hip return the very bits of the IEEE-754 operations the CPU oracle and the reference compute
// (`1.0f / a`, `sqrtf(x)`, round-to-nearest-even), so that swapping them in cannot change a single accumulator bit.
//   rcp:  y = v_rcp_f32(a) (1 ulp);  two Newton steps with exact residuals (fma)            [Markstein's scheme]
//   sqrt: y = v_rsq_f32(x); g = x*y, h = y/2; one coupled Newton step, then a residual correction of g
// Anything the short form gets wrong shows up here with its input; the kernel's helpers take the IEEE path there.
// Rows 4-7 (profiles/r15/exact_math_rsq.json): the rsq root BEHIND THE RANGE TEST of ptk_device_fn.h sqrt_ieee_rsq (everything
// outside 2^-102 <= x < +inf goes to sqrtf) in the coupled form, two shorter candidates behind the same test - the first of them,
// (ii), is what the cycle unit ships - and 1 / sqrt with the reciprocal seeded by the coupled root's own 2 h instead of v_rcp_f32.
//   hipcc -O3 -ffp-contract=off --offload-arch=gfx950 -o exact_math exact_math.hip && ./exact_math
#include <hip/hip_runtime.h>

#include <cstdint>
#include <cstdio>
#include <cstdlib>

#define CHECK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { fprintf(stderr, "%s: %s\n", #x, hipGetErrorString(e_)); exit(1); } } while (0)

__device__ __forceinline__ float rcp_short(float a)
{
    float y = __builtin_amdgcn_rcpf(a);
    float e = __builtin_fmaf(-a, y, 1.0f);
    y = __builtin_fmaf(y, e, y);
    e = __builtin_fmaf(-a, y, 1.0f);
    y = __builtin_fmaf(y, e, y);
    return y;
}
__device__ __forceinline__ float rcp_short1(float a)     // one step only: is it enough?
{
    float y = __builtin_amdgcn_rcpf(a);
    float e = __builtin_fmaf(-a, y, 1.0f);
    return __builtin_fmaf(y, e, y);
}
__device__ __forceinline__ float sqrt_short(float x)
{
    float y = __builtin_amdgcn_rsqf(x);
    float g = x * y, h = 0.5f * y;
    float r = __builtin_fmaf(-g, h, 0.5f);
    g = __builtin_fmaf(g, r, g); h = __builtin_fmaf(h, r, h);
    float d = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(d, h, g);
}

// v_sqrt_f32 (1 ulp) and the two neighbour tests of the compiler's own IEEE expansion - exact residuals of the candidates
// one ulp below and above - WITHOUT that expansion's range scaling (x < 2^-96 is multiplied by 2^32 first) and special-case
// selects: which inputs need those?
__device__ __forceinline__ float sqrt_nb(float x)
{
    float s = __builtin_amdgcn_sqrtf(x);
    const float sm = __uint_as_float(__float_as_uint(s) - 1u), sp = __uint_as_float(__float_as_uint(s) + 1u);
    const float rm = __builtin_fmaf(-sm, s, x), rp = __builtin_fmaf(-sp, s, x);
    s = rm <= 0.0f ? sm : s;
    return rp > 0.0f ? sp : s;
}

// the range test of sqrt_ieee_rsq: as unsigned numbers the bit patterns of [2^-102, +inf) are consecutive
__device__ __forceinline__ bool rsq_range(float x) { return __float_as_uint(x) - 0x0c800000u < 0x7f800000u - 0x0c800000u; }
__device__ __forceinline__ float sqrt_rsq_guarded(float x) { return rsq_range(x) ? sqrt_short(x) : sqrtf(x); }
// (ii) no coupled step: the residual correction of g with the unrefined h
__device__ __forceinline__ float sqrt_rsq_ii(float x)
{
    if (!rsq_range(x)) return sqrtf(x);
    const float y = __builtin_amdgcn_rsqf(x);
    const float g = x * y, h = 0.5f * y;
    const float r = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(r, h, g);
}
// (iii) that correction twice
__device__ __forceinline__ float sqrt_rsq_iii(float x)
{
    if (!rsq_range(x)) return sqrtf(x);
    const float y = __builtin_amdgcn_rsqf(x);
    float g = x * y; const float h = 0.5f * y;
    float r = __builtin_fmaf(-g, g, x);
    g = __builtin_fmaf(r, h, g);
    r = __builtin_fmaf(-g, g, x);
    return __builtin_fmaf(r, h, g);
}
// 1 / sqrt(x) in two roundings with the reciprocal's Newton step started from 2 h (the coupled step's refined h) instead of v_rcp_f32(s)
__device__ __forceinline__ float inv_length_2h(float x)
{
    if (!rsq_range(x)) return 1.0f / sqrtf(x);
    const float y = __builtin_amdgcn_rsqf(x);
    float g = x * y, h = 0.5f * y;
    const float r = __builtin_fmaf(-g, h, 0.5f);
    g = __builtin_fmaf(g, r, g); h = __builtin_fmaf(h, r, h);
    const float d = __builtin_fmaf(-g, g, x);
    const float s = __builtin_fmaf(d, h, g);
    const float y0 = 2.0f * h;
    const float e = __builtin_fmaf(-s, y0, 1.0f);
    return __builtin_fmaf(y0, e, y0);
}

#define ROWS 8
struct Report { unsigned long long bad[ROWS]; unsigned first[ROWS][8]; unsigned long long lo_bad[ROWS], hi_bad[ROWS]; };

__device__ void note(Report* r, int which, unsigned bits, bool in_domain)
{
    const unsigned long long k = atomicAdd(&r->bad[which], 1ull);
    if (k < 8) r->first[which][k] = bits;
    if (in_domain) { atomicAdd(&r->lo_bad[which], 1ull); atomicMax(&r->hi_bad[which], (unsigned long long)bits); }
}

__global__ void sweep(Report* rep)
{
    const unsigned long long stride = (unsigned long long)gridDim.x * blockDim.x;
    for (unsigned long long b = (unsigned long long)blockIdx.x * blockDim.x + threadIdx.x; b < (1ull << 32); b += stride)
    {
        const unsigned bits = (unsigned)b;
        const float a = __uint_as_float(bits);
        const unsigned ex = (bits >> 23) & 255u;
        const bool is_nan = ex == 255u && (bits & 0x7fffffu);
        // reciprocal: domain = normal inputs whose reciprocal is normal too (2^-126 <= |a| <= 2^126)
        {
            const float ref = 1.0f / a;
            const bool dom = ex >= 1u && ex <= 252u;
            const float f2 = rcp_short(a), f1 = rcp_short1(a);
            const bool refnan = ref != ref;
            if (!(refnan ? (f2 != f2) : (__float_as_uint(f2) == __float_as_uint(ref)))) note(rep, 0, bits, dom && !is_nan);
            if (!(refnan ? (f1 != f1) : (__float_as_uint(f1) == __float_as_uint(ref)))) note(rep, 1, bits, dom && !is_nan);
        }
        {
            const float ref = sqrtf(a);
            const bool dom = ex >= 1u && ex <= 254u && !(bits >> 31);
            const float f = sqrt_short(a);
            const bool refnan = ref != ref;
            if (!(refnan ? (f != f) : (__float_as_uint(f) == __float_as_uint(ref)))) note(rep, 2, bits, dom);
            // neighbour-test form: domain = +0, positive normals, +inf (everything a squared length or a unit-interval draw can be)
            const bool dom_nb = bits == 0u || (!(bits >> 31) && ex >= 1u && !is_nan);
            const float g = sqrt_nb(a);
            if (!(refnan ? (g != g) : (__float_as_uint(g) == __float_as_uint(ref)))) note(rep, 3, bits, dom_nb);
            // the guarded forms: their domain is what passes the range test, and the whole function is held on every input
            const bool dom_g = rsq_range(a);
            const float f4 = sqrt_rsq_guarded(a), f5 = sqrt_rsq_ii(a), f6 = sqrt_rsq_iii(a);
            if (!(refnan ? (f4 != f4) : (__float_as_uint(f4) == __float_as_uint(ref)))) note(rep, 4, bits, dom_g);
            if (!(refnan ? (f5 != f5) : (__float_as_uint(f5) == __float_as_uint(ref)))) note(rep, 5, bits, dom_g);
            if (!(refnan ? (f6 != f6) : (__float_as_uint(f6) == __float_as_uint(ref)))) note(rep, 6, bits, dom_g);
            const float inv = 1.0f / ref, f7 = inv_length_2h(a);
            if (!(inv != inv ? (f7 != f7) : (__float_as_uint(f7) == __float_as_uint(inv)))) note(rep, 7, bits, dom_g);
        }
    }
}

int main()
{
    Report* d; Report h = {};
    CHECK(hipMalloc(&d, sizeof(Report)));
    CHECK(hipMemset(d, 0, sizeof(Report)));
    hipLaunchKernelGGL(sweep, dim3(256 * 16), dim3(256), 0, 0, d);
    CHECK(hipDeviceSynchronize());
    CHECK(hipMemcpy(&h, d, sizeof(h), hipMemcpyDeviceToHost));
    const char* names[ROWS] = { "rcp, two Newton steps", "rcp, one Newton step", "sqrt, rsq + coupled step + residual",
                                "sqrt, v_sqrt_f32 + residual tests of both neighbours, no range scaling",
                                "range test, rsq + coupled step + residual (Markstein), sqrtf outside",
                                "candidate (ii), shipped as sqrt_ieee_rsq: range test, rsq + residual with the unrefined h",
                                "candidate (iii): range test, rsq + that residual step twice",
                                "1 / sqrt: the coupled root, then one Newton step of the reciprocal from 2 h (against 1.0f / sqrtf(x))" };
    printf("{\"inputs\": 4294967296, \"rows\": [\n");
    for (int k = 0; k < ROWS; k++)
    {
        printf(" {\"sequence\": \"%s\", \"mismatches_all_inputs\": %llu, \"mismatches_in_domain\": %llu, \"largest_mismatching_input_in_domain_hex\": \"%08llx\", \"first_inputs_hex\": [", names[k], h.bad[k], h.lo_bad[k], h.hi_bad[k]);
        for (int j = 0; j < 8 && (unsigned long long)j < h.bad[k]; j++) printf("%s\"%08x\"", j ? ", " : "", h.first[k][j]);
        printf("]}%s\n", k < ROWS - 1 ? "," : "");
    }
    printf("], \"domain\": \"rcp: normal a with 2^-126 <= |a| <= 2^126 (biased exponent 1..252); sqrt: positive normal x; neighbour-test sqrt: +0, positive normal x, +inf; the four guarded rows: 2^-102 <= x < +inf, what the range test passes (outside it they are sqrtf)\"}\n");
    return 0;
}
