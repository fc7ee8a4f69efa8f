"""The cycle unit's square root (csrc/ptk_device_fn.h sqrt_ieee_rsq: x * v_rsq_f32(x) corrected once by its exact residual,
behind ONE range test that sends everything outside 2^-102 <= x < +inf to sqrtf) as compiled into libptk.so, through
ptk_probe_math's op 6, and the normalisation's factor over it (op 7).  The proof is the enumeration of all 2^32 inputs
(tools/microbench/exact_math.hip, profiles/r15/exact_math_rsq.json); this test holds the library's own code on every mantissa of
eight binades - the three about the range test's edge (biased exponents 24, 25 = 2^-102, 26), the three about 1 (126, 127, 128:
both exponent parities, where 1 - w * w and the unit-interval draws lie) and the two largest (253, 254) - and on the special
values, against numpy's correctly rounded float32 root AND against the neighbour-test forms every other unit keeps (ops 2 / 3):
the same bits, so the cycle unit's samples cannot move."""
import numpy as np
import pytest

pytestmark = pytest.mark.gpu

EXPONENTS = (24, 25, 26, 126, 127, 128, 253, 254)


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


def _first_difference(x, got, want):
    nan = np.isnan(want)
    bad = np.flatnonzero((np.isnan(got) != nan) | (~nan & (_bits(got) != _bits(want))))
    return [(hex(int(_bits(x)[i])), hex(int(_bits(got)[i])), hex(int(_bits(want)[i]))) for i in bad[:5]], bad.size


def _check(ctx, x):
    with np.errstate(all="ignore"):
        root = np.sqrt(x).astype(np.float32)
    r6 = ctx.probe_math(6, x)
    assert _same(r6, root), _first_difference(x, r6, root)
    r2 = ctx.probe_math(2, x)
    assert _same(r6, r2), _first_difference(x, r6, r2)
    r7, r3 = ctx.probe_math(7, x), ctx.probe_math(3, x)
    assert _same(r7, r3), _first_difference(x, r7, r3)
    return root, r7


@pytest.mark.parametrize("exponent", EXPONENTS)
def test_every_mantissa_of_a_binade(ctx, exponent):
    x = (np.arange(1 << 23, dtype=np.uint32) | np.uint32(exponent << 23)).view(np.float32)
    root, inv = _check(ctx, x)
    # ... and the factor is the IEEE quotient of the rounded root (two roundings, glm's inversesqrt)
    with np.errstate(all="ignore"):
        assert _same(inv, (np.float32(1.0) / root).astype(np.float32))


def test_special_values_and_the_edge_of_the_range_test(ctx):
    x = np.array([0x00000000, 0x80000000,                               # +-0
                  0x0c7fffff, 0x0c800000, 0x0c800001,                   # 2^-102 and both neighbours
                  0x00000001, 0x00000002, 0x00400000, 0x007fffff, 0x00800000, 0x80000001,      # denormals, the smallest normal
                  0x7f7fffff, 0x7f800000, 0x7fc00000, 0xffc00000, 0x7f800001, 0xff800000,      # the largest finite, +inf, NaNs, -inf
                  0xbf800000, 0x3f800000, 0x40800000], np.uint32).view(np.float32)               # -1, 1, 4
    root, _ = _check(ctx, x)
    assert _bits(root[:2]).tolist() == [0x00000000, 0x80000000] and root[12] == np.inf and np.isnan(root[17]) and root[19] == 2.0
