"""The table half of the LAMBERT predicate (csrc/ptk_api.hip lambert_tables, include/ptk.h ptk_scene_is_lambert), on staged tables
with no device: a scene is Lambert when it is plain and no material has reflectiveness > 0.0f.

The kernel level the predicate selects drops the specular draw's comparison `draw < reflectiveness`, draw in [0, 1).  That is
exact precisely when the comparison is false for every draw: for zeros of either sign, negatives and NaN, and for nothing positive -
a draw of exactly 0 is below the smallest positive denormal.  So the boundary cases here are those values, on the 12-triangle
Cornell box, plus every edit that breaks plainness."""
import numpy as np

from conftest import load_golden, scene_from_golden

DENORMAL = np.float32(1.401298464324817e-45)       # 2^-149, the smallest positive float32


def _base():
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    rs = np.random.RandomState(5)
    a["uvs"] = rs.rand(len(a["verts"]), 6).astype(np.float32)
    return a


def _with_reflectiveness(a, value, which=None):
    b = dict(a); m = a["materials"].copy()
    if which is None: m["reflectiveness"][:] = value
    else: m["reflectiveness"][which] = value
    b["materials"] = m
    return b


def _with_texture(a, slot):
    from pbrpathtracer_amd import ptk
    b = dict(a)
    b["texels"] = np.random.RandomState(9).randint(0, 256, 16 * 16 * 4).astype(np.uint8)
    b["textures"] = np.array([(16, 16, 0)], dtype=ptk.TEXTURE_DTYPE)
    b["materials"] = a["materials"].copy()
    b["materials"]["tex"][0, slot] = 0
    return b


def test_the_cornell_golden_is_lambert():
    from pbrpathtracer_amd import ptk
    a = _base()
    assert DENORMAL > 0 and DENORMAL.view(np.uint32) == 1
    assert (a["materials"]["reflectiveness"] == 0).all()
    assert ptk.scene_is_plain(a) and ptk.scene_is_lambert(a)


def test_zeros_negatives_and_nan_qualify():
    from pbrpathtracer_amd import ptk
    a = _base()
    for value in (np.float32(0.0), np.float32(-0.0), np.float32(-1.0), np.float32(np.nan), np.float32(-np.inf), -DENORMAL):
        b = _with_reflectiveness(a, value)
        assert np.array_equal(b["materials"]["reflectiveness"].view(np.uint32),
                              np.full(len(b["materials"]), value.view(np.uint32), np.uint32))      # the bits reach the table
        assert ptk.scene_is_plain(b) and ptk.scene_is_lambert(b), value
        for which in range(len(a["materials"])):                   # ... and on one material among zeros
            assert ptk.scene_is_lambert(_with_reflectiveness(a, value, which)), (value, which)


def test_anything_positive_on_one_material_does_not():
    from pbrpathtracer_amd import ptk
    a = _base()
    for value in (DENORMAL, np.float32(1.1754944e-38), np.float32(0.7), np.float32(1.0), np.float32(np.inf)):
        for which in range(len(a["materials"])):
            b = _with_reflectiveness(a, value, which)
            assert ptk.scene_is_plain(b) and not ptk.scene_is_lambert(b), (value, which)
    # "no material": one that no triangle uses counts as well, as a glass one does for plainness
    b = dict(a); b["materials"] = np.concatenate([a["materials"], a["materials"][:1]]); b["materials"]["reflectiveness"][-1] = DENORMAL
    assert ptk.scene_is_plain(b) and not ptk.scene_is_lambert(b)
    b["materials"]["reflectiveness"][-1] = -0.0
    assert ptk.scene_is_lambert(b)


def test_every_edit_that_breaks_plain_breaks_lambert():
    from pbrpathtracer_amd import ptk
    a = _base()
    edits = {}
    b = dict(a); b["materials"] = a["materials"].copy()
    b["materials"]["type"][1] = 1; b["materials"]["translucency"][1] = 0.8; b["materials"]["roughness"][1] = 0.3
    edits["glass"] = b
    for slot in range(6):                                          # five shading slots and the opacity slot
        edits[f"texture slot {slot}"] = _with_texture(a, slot)
    b = dict(a); b["smoothing"] = a["smoothing"].copy(); b["smoothing"][4] = 1
    edits["smoothing"] = b
    b = dict(a); b["materials"] = np.concatenate([a["materials"], a["materials"][:1]]); b["materials"]["type"][-1] = 1
    edits["unused glass material"] = b
    per_tri = ("verts", "normals", "uvs", "tbn", "smoothing", "material")
    edits["17 triangles"] = {k: (np.concatenate([v, v[:5]]) if k in per_tri else v) for k, v in a.items()}
    edits["no triangle"] = {k: (v[:0] if k in per_tri + ("lights",) else v) for k, v in a.items()}
    for name, b in edits.items():
        assert not ptk.scene_is_plain(b), name
        assert not ptk.scene_is_lambert(b), name
    sixteen = {k: (np.concatenate([v, v[:4]]) if k in per_tri else v) for k, v in a.items()}
    assert len(sixteen["verts"]) == 16 and ptk.scene_is_lambert(sixteen)
    assert not ptk.scene_is_lambert(scene_from_golden(load_golden("tier_s_glass.npz")))
