"""The kernels replace `1.0f / a` and `sqrtf(x)` by short sequences (v_rcp_f32 / v_sqrt_f32 + exact fma residuals) that must
return the very bits of the IEEE-754 operations the reference's CPU code performs (IntersectTriangle's `f = 1.0 / a`,
pathtracer.cpp:384; glm::normalize's inversesqrt; the samplers' sqrt, :606-611, :734-739).  The proof is the enumeration of
all 2^32 inputs in tools/microbench/exact_math.hip (profiles/r02/exact_math.json); this test holds the helpers AS COMPILED
INTO libptk.so (ptk_probe_math) against the host's correctly rounded float32 division and square root on a few million
inputs: random bit patterns, the edges of each helper's domain and the inputs the enumeration singled out.

ptk_probe_math runs the build the "contract" option selects, so the same probe also holds the contracted builds (level 1:
-ffp-contract=fast; level 2: ... with the hardware's v_rcp / v_sqrt / v_rsq) to their documented error, and the sin / cos
polynomial of every build (ops 4 / 5) over every angle the kernels can pass it."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float32).view(np.uint32)


def _same(got, want):
    """bit-identical, NaNs matching NaNs"""
    nan = np.isnan(want)
    return np.array_equal(np.isnan(got), nan) and np.array_equal(_bits(got)[~nan], _bits(want)[~nan])


def _random_floats(n, seed, lo_exp, hi_exp, signed=True):
    """uniform over bit patterns with biased exponent in [lo_exp, hi_exp]"""
    rng = np.random.default_rng(seed)
    e = rng.integers(lo_exp, hi_exp + 1, n, dtype=np.uint32)
    m = rng.integers(0, 1 << 23, n, dtype=np.uint32)
    s = rng.integers(0, 2, n, dtype=np.uint32) if signed else np.zeros(n, np.uint32)
    return ((s << 31) | (e << 23) | m).view(np.float32)


def test_short_reciprocal_is_the_ieee_quotient(ctx):
    x = np.concatenate([_random_floats(4_000_000, 1, 1, 252),
                        np.array([2.0 ** -126, -(2.0 ** -126), 2.0 ** 126, -(2.0 ** 126), 1.0, -1.0, 3.0, 1e-30, 1e30], np.float32),
                        (np.arange(1 << 16, dtype=np.uint32) + np.uint32(0x3F7F8000)).view(np.float32)])      # around 1.0
    with np.errstate(all="ignore"):
        want = (np.float32(1.0) / x).astype(np.float32)
    assert _same(ctx.probe_math(0, x), want)
    # ... and with the special cases the normalisations can meet: zeros, infinities, NaN
    y = np.concatenate([x[:500_000], np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)])
    with np.errstate(all="ignore"):
        want = (np.float32(1.0) / y).astype(np.float32)
    assert _same(ctx.probe_math(1, y), want)


def test_short_square_root_is_the_ieee_root(ctx):
    edge = np.array([0x00000000, 0x00000001, 0x007fffff, 0x00800000, 0x0b6e9372, 0x0b6e9373, 0x0b7fffff, 0x0b800000, 0x0b800001,
                     0x0c7fffff, 0x0c800000, 0x3f800000, 0x3f7fffff, 0x3f800001, 0x7f7fffff, 0x7f800000, 0x7fc00000, 0x80000000,
                     0xbf800000], np.uint32).view(np.float32)
    x = np.concatenate([_random_floats(4_000_000, 2, 0, 254, signed=False),            # denormals and tiny values included
                        _random_floats(200_000, 3, 0, 30, signed=False),               # the range the guard sends to sqrtf
                        np.float32(1.0) - np.arange(1 << 16, dtype=np.float32) * np.float32(2.0 ** -24),      # 1 - w * w shapes
                        np.arange(1 << 16, dtype=np.float32) * np.float32(2.0 ** -24),                         # unit-interval draws
                        edge])
    with np.errstate(all="ignore"):
        want = np.sqrt(x).astype(np.float32)
    assert _same(ctx.probe_math(2, x), want)


def test_normalisation_factor_is_one_over_the_rounded_root(ctx):
    """glm::normalize = v * inversesqrt(dot(v, v)) with inversesqrt(x) = 1 / sqrt(x): two roundings, in that order"""
    x = np.concatenate([_random_floats(2_000_000, 4, 27, 247, signed=False), np.array([0.0, np.inf, 1.0, 4.0, 2.0], np.float32)])
    with np.errstate(all="ignore"):
        want = (np.float32(1.0) / np.sqrt(x).astype(np.float32)).astype(np.float32)
    assert _same(ctx.probe_math(3, x), want)


# ---- sin / cos of sincos_2pi ----------------------------------------------------------------------------------------------
def _all_angles():
    """every angle the kernels pass to sincos_2pi: (float)(2 pi * u) for u = k 2^-24, k < 2^24 (u01's values; SampleCircle's
    (float)((double)r1 * 2 * pi) and the lobe sampler's (float)(2 pi * theta) round the same double product)"""
    k = np.arange(1 << 24, dtype=np.float64)
    return ((2.0 * np.pi) * (k * 2.0 ** -24)).astype(np.float32)


@pytest.fixture(scope="module")
def angles():
    a = _all_angles()
    a64 = a.astype(np.float64)
    return a, np.sin(a64), np.cos(a64)


def _sincos_error(ctx, angles):
    a, s64, c64 = angles
    s, c = ctx.probe_math(4, a), ctx.probe_math(5, a)
    return s, c, float(np.abs(s - s64).max()), float(np.abs(c - c64).max())


def test_sin_cos_polynomial_is_the_oracles_at_every_angle(ctx, oracle_mod, angles):
    """The exact build's sincos_2pi against the oracle's orc_sincos, bit for bit, at all 2^24 angles: a wrong coefficient or
    quadrant on one side fails here.  Both sides leave libm by construction (difference 6), so the
    polynomial is also held to float64 sin / cos: at most 2^-23 off (measured: 7.0e-8 sin, 7.8e-8 cos)."""
    s, c, es, ec = _sincos_error(ctx, angles)
    rs, rc = oracle_mod.sincos_many(angles[0])
    print(f"exact build sin / cos over 2^24 angles: max |error| vs float64 {es:.3e} / {ec:.3e}")
    assert np.array_equal(_bits(s), _bits(rs)) and np.array_equal(_bits(c), _bits(rc))
    assert es <= 2.0 ** -23 and ec <= 2.0 ** -23


def _ulps_from_rounded(got, want64):
    """distance in representable floats between got and the correctly rounded float32 of want64 (finite, same sign)"""
    w = want64.astype(np.float32)
    gi, wi = _bits(got).astype(np.int64), _bits(w).astype(np.int64)
    assert (np.signbit(got) == np.signbit(w)).all() and np.isfinite(got).all()
    return np.abs(gi - wi)


@pytest.fixture
def contract(ctx):
    yield lambda level: ctx.set_option("contract", level)
    ctx.set_option("contract", 0)


def test_level1_helpers_keep_the_exact_sequences(ctx, angles, contract):
    """Level 1 contracts a * b + c but keeps the explicit fma sequences of rcp_ieee / sqrt_ieee: ops 0-3 give the exact build's
    bits on the inputs of the tests above; its sin / cos (whose polynomial the compiler may fuse) stay within 2^-23."""
    ins = [_random_floats(1_000_000, 11, 1, 252),
           np.concatenate([_random_floats(1_000_000, 12, 1, 252), np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)]),
           np.concatenate([_random_floats(1_000_000, 13, 0, 254, signed=False), _random_floats(100_000, 14, 0, 30, signed=False)]),
           np.concatenate([_random_floats(1_000_000, 15, 27, 247, signed=False), np.array([0.0, np.inf, 1.0, 4.0], np.float32)])]
    exact = [ctx.probe_math(op, x) for op, x in enumerate(ins)]
    contract(1)
    for op, x in enumerate(ins):
        assert _same(ctx.probe_math(op, x), exact[op]), op
    _, _, es, ec = _sincos_error(ctx, angles)
    print(f"contract 1 sin / cos over 2^24 angles: max |error| vs float64 {es:.3e} / {ec:.3e}")
    assert es <= 2.0 ** -23 and ec <= 2.0 ** -23


def test_level2_hardware_helpers_are_within_one_ulp(ctx, angles, contract):
    """Level 2 takes 1 / x, sqrt and 1 / sqrt from v_rcp_f32 / v_sqrt_f32 / v_rsq_f32: within 1 ulp of the
    correctly rounded result on the domain each helper serves - rcp on 2^-126 <= |a| <= 2^126, sqrt and the normalisation
    factor (op 3 = inv_length, the factor normalize() multiplies by) on +0, +inf and x >= 2^-104; op 1 keeps the IEEE
    special cases the normalisations can meet.  Sin / cos within 2^-23 of float64."""
    contract(2)
    rcp_in = np.concatenate([_random_floats(2_000_000, 21, 1, 252),
                             np.array([2.0 ** -126, -(2.0 ** -126), 2.0 ** 126, -(2.0 ** 126), 1.0, -1.0, 3.0], np.float32),
                             (np.arange(1 << 16, dtype=np.uint32) + np.uint32(0x3F7F8000)).view(np.float32)])
    want = 1.0 / rcp_in.astype(np.float64)
    u0 = _ulps_from_rounded(ctx.probe_math(0, rcp_in), want)
    u1 = _ulps_from_rounded(ctx.probe_math(1, rcp_in), want)
    special = np.array([0.0, -0.0, np.inf, -np.inf, np.nan], np.float32)
    got = ctx.probe_math(1, special)
    assert _same(got, np.array([np.inf, -np.inf, 0.0, -0.0, np.nan], np.float32))
    edge = np.array([0x0b800000, 0x0b800001, 0x0c000000, 0x0c000001, 0x3f800000, 0x3f7fffff, 0x3f800001, 0x7f7fffff], np.uint32).view(np.float32)
    rt_in = np.concatenate([_random_floats(2_000_000, 22, 23, 254, signed=False),
                            np.float32(1.0) - np.arange(1 << 16, dtype=np.float32) * np.float32(2.0 ** -24),
                            np.arange(1, 1 << 16, dtype=np.float32) * np.float32(2.0 ** -24), edge])
    r64 = np.sqrt(rt_in.astype(np.float64))
    u2 = _ulps_from_rounded(ctx.probe_math(2, rt_in), r64)
    u3 = _ulps_from_rounded(ctx.probe_math(3, rt_in), 1.0 / r64)
    ends = np.array([0.0, np.inf], np.float32)
    assert _same(ctx.probe_math(2, ends), ends) and _same(ctx.probe_math(3, ends), np.array([np.inf, 0.0], np.float32))
    _, _, es, ec = _sincos_error(ctx, angles)
    print(f"contract 2: max ulps from the correctly rounded result: rcp {u0.max()} (off {np.mean(u0 != 0):.4f}), "
          f"rcp_any {u1.max()}, sqrt {u2.max()} (off {np.mean(u2 != 0):.4f}), 1/sqrt {u3.max()} (off {np.mean(u3 != 0):.4f}); "
          f"sin / cos max |error| vs float64 {es:.3e} / {ec:.3e}")
    assert u0.max() <= 1 and u1.max() <= 1 and u2.max() <= 1 and u3.max() <= 1
    assert es <= 2.0 ** -23 and ec <= 2.0 ** -23
