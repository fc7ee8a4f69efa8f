"""The display transform (include/ptk.h ptk_display_planes, ptk_display_frame) without a GPU: the entry points
exist; the sRGB threshold table the library returns is what the header says it is; tests/display_rule.py - the numpy mirror the GPU
tests hold the kernels to bit for bit - encodes like the double-precision formula, reduces to the plain resolve, meters what the
header says within the bounds a bin's width allows, and adapts by the formula; the library refuses what the header lists."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import display_rule as DR

f32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW_PTK = ("ptk_display_planes", "ptk_display_planes_device", "ptk_display_frame", "ptk_read_display", "ptk_display_device_ptr",
           "ptk_display_state", "ptk_display_reset", "ptk_display_srgb_table", "ptk_display_check_params", "ptk_last_display_ms")
NEW_PTH = ("pth_display_frame", "pth_read_display", "pth_display_state", "pth_display_reset")
PTK_OK, PTK_ERR_BAD_ARG = 0, -1


@pytest.fixture(scope="module")
def table():
    from pbrpathtracer_amd import ptk
    return ptk.display_srgb_table()


def grey(L, w=96, h=54):
    return np.full((h, w, 3), L, f32)


def lognormal(seed=5, w=96, h=54, sigma=2.0):
    rng = np.random.default_rng(seed)
    return np.exp(rng.normal(0.0, sigma, (h, w, 3))).astype(f32)


def test_symbols_are_exported_and_declared():
    from pbrpathtracer_amd import ptk, pathtracer
    L = ptk.load()
    text = open(os.path.join(ROOT, "include", "ptk.h")).read() + open(os.path.join(ROOT, "include", "ptk_host.h")).read()
    declared = set(re.findall(r"\b(p(?:tk|th)_[a-z0-9_]+)\s*\(", text))
    for name in NEW_PTK + NEW_PTH:
        assert name in declared, name
        assert hasattr(L, name), name
        assert name in ptk.SYMBOLS + pathtracer.HOST_SYMBOLS, name


def test_defaults_are_the_documented_ones():
    from pbrpathtracer_amd import ptk
    d = ptk.display_defaults().as_dict()
    ref = DR.params()
    assert set(d) == set(ref)
    for k, v in ref.items():
        assert d[k] == (f32(v) if isinstance(v, float) else v), k
    assert (d["mode"], d["op"], d["transfer"]) == (ptk.EXPOSURE_METERED, ptk.DISPLAY_ACES, ptk.TRANSFER_SRGB)
    assert ptk.display_check_params(None) == PTK_OK


def test_table_is_the_srgb_decoding(table):
    assert table.dtype == f32 and table.shape == (256,)
    assert table[0] == 0 and table[255] == 1
    assert np.all(np.diff(table) > 0)                        # strictly increasing in float32
    v = np.arange(256, dtype=np.float64) / 255.0
    exact = np.where(v < 0.04045, v / 12.92, ((v + 0.055) / 1.055) ** 2.4)
    ulp = np.spacing(np.maximum(table, np.finfo(f32).tiny)).astype(np.float64)
    assert np.all(np.abs(table.astype(np.float64) - exact) <= ulp)


def test_srgb_bytes_are_the_truncated_oetf(table):
    y = np.random.default_rng(1).random(10 ** 6, dtype=f32)
    got = DR.apply(y.reshape(-1, 1, 1).repeat(3, 2), 1.0, DR.params(mode=DR.MANUAL, op=DR.LINEAR), table)[:, 0, 0].astype(np.int64)
    yd = y.astype(np.float64)
    oetf = np.where(yd <= 0.0031308, 12.92 * yd, 1.055 * yd ** (1 / 2.4) - 0.055)
    ref = np.floor(255.0 * oetf).astype(np.int64)
    diff = np.abs(got - ref)
    print("differing samples:", int((diff > 0).sum()), "largest difference:", int(diff.max()))
    assert diff.max() <= 1
    assert (diff > 0).mean() <= 1e-4


def test_manual_linear_linear_is_the_plain_resolve(table):
    rng = np.random.default_rng(2)
    x = rng.normal(0.5, 0.6, (33, 67, 3)).astype(f32)
    x[0, :8, 0] = (np.nan, np.inf, -np.inf, 0.0, -0.0, 1.0, np.nextafter(f32(1), f32(0)), 1e-40)
    p = DR.params(mode=DR.MANUAL, exposure=1.0, op=DR.LINEAR, transfer=DR.T_LINEAR)
    got, state = DR.display(x, p, table)
    ref = (np.where(np.isnan(x), f32(0), x).clip(0, 1) * f32(255)).astype(np.uint8)
    assert np.array_equal(got, ref)
    assert state == DR.NO_STATE


@pytest.mark.parametrize("L", (0.18, 1.0, 3.7, 1e-3, 900.0))
def test_constant_image_meters_its_luminance_within_a_bin(table, L):
    img = grey(L)
    _, st = DR.display(img, DR.params(), table)
    ratio = float(st["lavg"]) / float(DR.luminance(img)[0, 0])
    print("Lavg / L =", ratio)
    # a bin spans [m, m + 1/8) of the mantissa and is read back at its centre
    assert 1.0625 / 1.125 <= ratio <= 1.0625
    assert st["counted"] == img.shape[0] * img.shape[1] and st["kept"] == st["counted"] * 950 // 1000 - st["counted"] * 100 // 1000
    want = min(max(f32(0.18) / st["lavg"], f32(2.0 ** -10)), f32(2.0 ** 10))     # (L = 900 meets the lower clamp)
    assert DR.bits(st["exposure"]) == DR.bits(want) and st["has_prev"] == 1


def test_lognormal_image_meters_near_the_geometric_mean(table):
    img = lognormal()
    p = DR.params()
    _, st = DR.display(img, p, table)
    L = np.sort(DR.luminance(img).reshape(-1).astype(np.float64))
    assert L[0] >= p["min_lum"] and L[-1] <= p["max_lum"]
    N = len(L)
    kept = L[N * 100 // 1000: N * 950 // 1000]
    assert st["counted"] == N and st["kept"] == len(kept)
    gm = float(np.exp(np.mean(np.log(kept))))
    ratio = float(st["lavg"]) / gm
    print("Lavg / geometric mean =", ratio)
    # log2(1 + m) - m <= 0.086 between the piecewise-linear and the true logarithm, plus 0.09 for the half-bin re-centring
    assert 2.0 ** -0.18 <= ratio <= 2.0 ** 0.18


@pytest.mark.parametrize("fill", (0.0, np.nan, -1.0, np.inf))
def test_nothing_counted_keeps_the_previous_exposure_or_gives_one(table, fill):
    img = grey(fill)
    out, st = DR.display(img, DR.params(), table)
    assert st["counted"] == 0 and st["kept"] == 0 and st["has_prev"] == 0
    assert DR.bits(st["exposure"]) == DR.bits(f32(1)) and DR.bits(st["target"]) == DR.bits(f32(1))
    _, lit = DR.display(grey(2.5), DR.params(), table)
    _, st2 = DR.display(img, DR.params(adapt=0.25), table, prev=lit)
    assert DR.bits(st2["exposure"]) == DR.bits(lit["exposure"]) and st2["has_prev"] == 1 and st2["counted"] == 0
    # a black frame in front of the first lit one is no anchor: the lit frame lands on its target
    _, st3 = DR.display(grey(2.5), DR.params(adapt=0.25), table, prev=st)
    assert DR.bits(st3["exposure"]) == DR.bits(lit["exposure"])


def test_adaptation_walks_toward_the_target_by_the_formula(table):
    _, st = DR.display(grey(0.5), DR.params(adapt=0.25), table)
    assert DR.bits(st["exposure"]) == DR.bits(st["target"])            # no previous exposure: the target itself
    e = st["exposure"]
    bright = grey(4.0)
    target = DR.display(bright, DR.params(), table)[1]["target"]
    assert target < e
    for _ in range(4):
        _, st = DR.display(bright, DR.params(adapt=0.25), table, prev=st)
        e = f32(e + f32(f32(target - e) * f32(0.25)))
        assert DR.bits(st["target"]) == DR.bits(target) and DR.bits(st["exposure"]) == DR.bits(e)
    assert target < e < f32(0.18) / f32(0.5)


@pytest.mark.parametrize("adapt", (1.0, 1.5, np.inf))
def test_adapt_of_one_or_more_lands_on_the_target(table, adapt):
    _, st = DR.display(grey(0.5), DR.params(), table)
    _, st = DR.display(grey(4.0), DR.params(adapt=adapt), table, prev=st)
    assert DR.bits(st["exposure"]) == DR.bits(st["target"])
    assert DR.bits(st["target"]) == DR.bits(DR.display(grey(4.0), DR.params(), table)[1]["target"])


def test_metered_target_is_clamped(table):
    _, st = DR.display(grey(1e-5), DR.params(), table)
    assert DR.bits(st["exposure"]) == DR.bits(f32(2.0 ** 10))
    _, st = DR.display(grey(1e5), DR.params(), table)
    assert DR.bits(st["exposure"]) == DR.bits(f32(2.0 ** -10))


def test_one_counted_pixel_takes_the_lo_plus_one_arm(table):
    img = grey(0.0, 7, 5)
    img[3, 2] = 0.75
    for lo, hi in ((100, 950), (0, 1000), (499, 500)):
        _, st = DR.display(img, DR.params(low_permille=lo, high_permille=hi), table)
        assert st["counted"] == 1 and st["kept"] == 1
        assert 1.0625 / 1.125 <= float(st["lavg"]) / float(DR.luminance(img)[3, 2]) <= 1.0625


REFUSED = [dict(mode=2), dict(mode=-1), dict(op=3), dict(op=-1), dict(transfer=2), dict(transfer=-1),
           dict(mode=0, exposure=0.0), dict(mode=0, exposure=-1.0), dict(mode=0, exposure=np.nan),
           dict(key=0.0), dict(key=np.nan), dict(white=0.0), dict(white=-2.0), dict(white=np.nan),
           dict(min_exposure=0.0), dict(min_exposure=np.nan), dict(min_exposure=np.inf),
           dict(max_exposure=-1.0), dict(max_exposure=np.nan), dict(max_exposure=np.inf),
           dict(min_lum=np.inf), dict(min_lum=np.nan), dict(max_lum=np.inf), dict(max_lum=np.nan),
           dict(min_lum=0.0), dict(min_lum=1e-39), dict(min_lum=2.0, max_lum=1.0),
           dict(low_permille=-1), dict(high_permille=1001), dict(low_permille=500, high_permille=500),
           dict(low_permille=600, high_permille=400), dict(adapt=-0.5), dict(adapt=np.nan)]
ACCEPTED = [dict(), dict(white=np.inf), dict(mode=1, exposure=0.0), dict(min_lum=2.0 ** -126), dict(min_lum=1.0, max_lum=1.0),
            dict(low_permille=0, high_permille=1000), dict(low_permille=499, high_permille=500), dict(adapt=0.0), dict(adapt=np.inf),
            dict(key=np.inf), dict(mode=0, exposure=np.inf)]


@pytest.mark.parametrize("edit", REFUSED, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()))
def test_library_refuses(edit):
    from pbrpathtracer_amd import ptk
    assert ptk.display_check_params(ptk.display_defaults(**edit)) == PTK_ERR_BAD_ARG


@pytest.mark.parametrize("edit", ACCEPTED, ids=lambda e: ",".join(f"{k}={v}" for k, v in e.items()) or "defaults")
def test_library_accepts(edit):
    from pbrpathtracer_amd import ptk
    assert ptk.display_check_params(ptk.display_defaults(**edit)) == PTK_OK


def test_null_arguments_are_refused_without_a_device():
    from pbrpathtracer_amd import ptk
    L = ptk.load()
    prm = ptk.display_defaults()
    img, out = np.zeros((2, 2, 3), f32), np.zeros((2, 2, 3), np.uint8)
    assert L.ptk_display_check_params(None) == PTK_ERR_BAD_ARG
    assert L.ptk_display_srgb_table(None) == PTK_ERR_BAD_ARG
    for fn in (L.ptk_display_planes, L.ptk_display_planes_device):
        assert fn(None, 2, 2, img.ctypes.data, C.byref(prm), out.ctypes.data, None) == PTK_ERR_BAD_ARG
    assert L.ptk_display_frame(None, 0, C.byref(prm)) == PTK_ERR_BAD_ARG
    assert L.ptk_read_display(None, out.ctypes.data) == PTK_ERR_BAD_ARG
    assert L.ptk_display_device_ptr(None, None, None) == PTK_ERR_BAD_ARG
    assert L.ptk_display_state(None, None) == PTK_ERR_BAD_ARG
    assert L.ptk_display_reset(None) == PTK_ERR_BAD_ARG
    assert L.ptk_last_display_ms(None, None, None, None) == PTK_ERR_BAD_ARG
    assert not out.any()
