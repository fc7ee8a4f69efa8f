"""The frame table of the exact PLAIN trace kernel (csrc/ptk_device.h FLAT_FRAMES_AT, csrc/ptk_frame.hip fill_flat_frames_kernel,
csrc/ptk_device_fn.h sample_basis): the hemisphere sampler's tangent frame about a plain triangle's normal is read from a table
with one entry per (triangle, side of its stored normal) instead of being computed at every diffuse interaction.

The table holds what the kernel used to compute, so nothing may change: every accumulator word is compared with == against the
CPU oracle and against the generic FLAT kernel ("plain_kernel" 0), which still computes the frame.  The scenes are chosen for
the ways a table can be wrong: the side (open scenes, so that triangles are shaded from both sides), the axis choice of the
sampler (normals at and around |n.x| = 1 - PTK_EPS), degenerate triangles, lanes of one wave on three sampler routes, a table
gone stale after ptk_update_geometry, and an update that was refused."""
import numpy as np
import pytest

from conftest import load_golden, scene_from_golden
from test_gpu_random_scenes import random_scene

gpu = pytest.mark.gpu

W, H, D, SPP, SEED = 64, 48, 8, 8, 21
THR = np.float32(1.0) - np.float32(0.00001)             # 1.0f - PTK_EPS, the hemisphere sampler's axis threshold on |n.x|
OPEN_SCENES = ((30, 9), (30, 16))                       # (scene seed, triangles): chosen so that the oracle shades both sides >= 50 times


def _unit(v):
    return v / np.maximum(np.linalg.norm(v, axis=-1, keepdims=True), 1e-20)


def _tbn_of(verts):
    """face normal, tangent, bitangent from the winding, as test_gpu_random_scenes.random_scene builds them"""
    v = verts.reshape(-1, 3, 3)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    fn = _unit(np.cross(e1, e2)).astype(np.float32)
    tg = _unit(e1).astype(np.float32)
    bt = _unit(np.cross(fn, tg)).astype(np.float32)
    return np.concatenate([fn, tg, bt], axis=1).astype(np.float32)


def open_plain_scene(seed, n):
    """random_scene made plain (opaque untextured type-0 materials, nothing smoothed, a pinhole) and open - big triangles at random
    angles, seen from both sides - with four special triangles at the end: a normal of exactly (1, 0, 0), normals with |n.x| one
    ulp under and exactly at 1 - PTK_EPS (the two arms of `fabsf(n.x) < thr`), and a zero-area triangle"""
    arrays, cam = random_scene(seed, n, False)
    a = {k: np.array(v) for k, v in arrays.items()}
    a["materials"]["type"] = 0
    a["smoothing"][:] = 0
    cam = dict(cam); cam["aperture"] = 0.0
    v = a["verts"].reshape(n, 3, 3)
    tbn = a["tbn"].copy()

    def plane_tri(k, nrm, centre, size):
        nrm = np.asarray(nrm, np.float64)
        t1 = _unit(np.array([-nrm[1], nrm[0], 0.0])); t2 = np.array([0.0, 0.0, 1.0])
        c = np.asarray(centre, np.float64)
        v[k] = np.array([c - size * t1 - size * t2, c + size * t1 - size * t2, c + size * t2], np.float64).astype(np.float32)
        tbn[k] = np.concatenate([np.asarray(nrm, np.float32), t1.astype(np.float32), t2.astype(np.float32)])
        tbn[k, 0:3] = np.asarray(nrm, np.float32)

    under, over = np.nextafter(THR, np.float32(0)), THR
    plane_tri(n - 4, (1.0, 0.0, 0.0), (-1.1, 0.1, 0.4), 1.3)
    plane_tri(n - 3, (under, np.sqrt(1.0 - float(under) ** 2), 0.0), (1.2, -0.2, 0.2), 1.2)
    plane_tri(n - 2, (-float(over), np.sqrt(1.0 - float(over) ** 2), 0.0), (0.4, 0.3, -0.6), 0.9)
    v[n - 1] = np.float32([0.3, 0.2, 0.1])                               # zero area: never hit, its frames are NaN
    tbn[n - 1] = 0.0
    a["verts"] = v.reshape(n, 9); a["tbn"] = tbn
    assert tbn[n - 4, 0] == 1.0 and abs(tbn[n - 3, 0]) < THR and not abs(tbn[n - 2, 0]) < THR
    return a, cam


def three_sampler_cornell():
    """the tier-S Cornell box with one material a rough lobe (sampler 2), one a mirror (0) and one a fully rough reflector (1, from
    the reflective branch), beside the diffuse ones (1): the routes meet in one wave"""
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    m = a["materials"]
    m["reflectiveness"][1] = 0.5; m["roughness"][1] = 0.5
    m["reflectiveness"][2] = 0.5; m["roughness"][2] = 0.0
    m["reflectiveness"][3] = 0.5; m["roughness"][3] = 1.0
    camz = z["cam"]; proj = z["proj"]
    cam = dict(pos=camz[0:3], dir=camz[3:6], up=camz[6:9], focal=float(proj[0]), fovy=float(proj[1]),
               focal_dist=float(z["focal_dist"]), aperture=0.0)
    return a, cam


def _rot_y(deg):
    r = np.deg2rad(deg)
    return np.array([[np.cos(r), 0, np.sin(r)], [0, 1, 0], [-np.sin(r), 0, np.cos(r)]])


def moved_scenes():
    """name -> (first, verts, normals, tbn, whole moved scene) from three_sampler_cornell: a rotation that takes the side walls'
    normals (+-1, 0, 0) from the |n.x| >= 1 - PTK_EPS arm to the other, and a mirroring in x, which reverses every winding"""
    a, _ = three_sampler_cornell()
    n = len(a["verts"])
    out = {}
    R = _rot_y(25.0)
    nv = (a["verts"].reshape(n, 3, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(n, 9)
    nn = (a["normals"].reshape(n, 3, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(n, 9)
    tb = (a["tbn"].reshape(n, 3, 3).astype(np.float64) @ R.T).astype(np.float32).reshape(n, 9)
    out["rotation"] = (0, nv, nn, tb)
    first, last = 2, n - 1                                  # a range, not the whole scene: the table's other entries stay
    mv = (a["verts"][first:last].reshape(-1, 3, 3) * np.float32([-1, 1, 1])).reshape(-1, 9)
    mt = _tbn_of(mv)
    mn = np.tile(mt[:, 0:3], (1, 3))
    out["mirroring"] = (first, mv, mn, mt)
    for name, (f, v, nn, tb) in list(out.items()):
        m = dict(a)
        for key, val in (("verts", v), ("normals", nn), ("tbn", tb)):
            m[key] = a[key].copy(); m[key][f:f + len(v)] = val
        out[name] = (f, v, nn, tb, m)
    return out


def plain_scenes():
    """every scene this file renders with the PLAIN kernel"""
    s = {"open%d" % n: open_plain_scene(seed, n)[0] for seed, n in OPEN_SCENES}
    s["cornell3"] = three_sampler_cornell()[0]
    for name, mv in moved_scenes().items():
        s[name] = mv[4]
    return s


def _ocam(OB, cam):
    return OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])


def _oracle(OB, arrays, cam, spp=SPP):
    o = OB.Oracle(arrays)
    tot, rgb = o.render(_ocam(OB, cam), W, H, D, 0, spp, SEED)
    o.close()
    return tot, rgb


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum(), ctx.resolve_rgb8(), ctx.trace_variant()


def _same(a, b):
    return np.array_equal(a.view(np.uint32), b.view(np.uint32))


def sides_shaded(OB, arrays, cam):
    """how often the oracle samples a direction at a hit on the stored normal's side (0) and on the other (1): hits of camera and
    bounce rays that another ray of the same path follows"""
    o = OB.Oracle(arrays)
    r = o.render_counted(_ocam(OB, cam), W, H, D, 0, SPP, SEED, dump=True)["rays"]
    o.close()
    path = r["pixel"].astype(np.int64) * 4096 + r["sample"]
    followed = np.zeros(len(r), bool); followed[:-1] = path[:-1] == path[1:]
    sel = (r["kind"] != OB.RAY_SHADOW) & (r["tri"] >= 0) & followed
    nrm = arrays["tbn"][r["tri"][sel], 0:3]
    back = (nrm * r["rd"][sel]).sum(axis=1) > 0
    return int((~back).sum()), int(back.sum())


@pytest.fixture(scope="module")
def ctxs():
    from pbrpathtracer_amd import ptk
    a, b = ptk.Context(0), ptk.Context(0)
    yield a, b
    a.close(); b.close()


def _setup(c, arrays, cam):
    c.upload_scene(arrays); c.set_camera(**cam); c.set_frame(W, H, D); c.set_tile(0, 1); c.reset()


# ---- no device needed -----------------------------------------------------------------------------------------------------------
def test_every_scene_here_is_plain_on_its_staged_tables():
    from pbrpathtracer_amd import ptk
    for name, arrays in plain_scenes().items():
        assert len(arrays["verts"]) <= 16 and ptk.scene_is_plain(arrays), name


@pytest.mark.parametrize("seed,n", OPEN_SCENES)
def test_open_scenes_are_shaded_from_both_sides(oracle_mod, seed, n):
    arrays, cam = open_plain_scene(seed, n)
    front, back = sides_shaded(oracle_mod, arrays, cam)
    assert front >= 50 and back >= 50, (front, back)


# ---- against the oracle and the generic FLAT kernel -----------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("scene", ["open9", "open16", "cornell3"])
def test_plain_equals_generic_equals_oracle(ctxs, oracle_mod, scene):
    """both work distributions, and a render of several passes (32 samples: 1 MiB of pass_bytes holds 21 of this frame)"""
    from pbrpathtracer_amd import ptk
    a, _ = ctxs
    arrays, cam = three_sampler_cornell() if scene == "cornell3" else open_plain_scene(*[s for s in OPEN_SCENES if s[1] == int(scene[4:])][0])
    ref, ref8 = _oracle(oracle_mod, arrays, cam)
    assert (ref != 0).any()
    try:
        _setup(a, arrays, cam)
        for persistent in (1, 0):
            a.set_option("persistent", persistent)
            acc_p, rgb_p, var_p = _render(a)
            a.set_option("plain_kernel", 0)
            acc_g, rgb_g, var_g = _render(a)
            a.set_option("plain_kernel", 1)
            assert (var_p, var_g) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT), persistent
            assert _same(acc_p, ref) and np.array_equal(rgb_p, ref8), persistent
            assert _same(acc_p, acc_g) and np.array_equal(rgb_p, rgb_g), persistent
        a.set_option("persistent", -1)
        ref32, ref32_8 = _oracle(oracle_mod, arrays, cam, spp=32)
        a.set_option("pass_bytes", 1 << 20)
        acc_p, rgb_p, var_p = _render(a, spp=32)
        assert a.last_render_ms()[1] >= 6                    # two passes at least
        assert var_p == ptk.TRACE_FLAT_PLAIN
        assert _same(acc_p, ref32) and np.array_equal(rgb_p, ref32_8)
    finally:
        a.set_option("persistent", -1); a.set_option("plain_kernel", 1); a.set_option("pass_bytes", float(16 << 30))


@gpu
@pytest.mark.parametrize("contract", [1, 2])
def test_contracted_plain_equals_contracted_generic(ctxs, contract):
    """the contracted builds compute the frame at run time in both kernels: PLAIN reproduces generic FLAT bit for bit"""
    from pbrpathtracer_amd import ptk
    a, _ = ctxs
    try:
        a.set_option("contract", contract)
        for arrays, cam in [open_plain_scene(*s) for s in OPEN_SCENES] + [three_sampler_cornell()]:
            _setup(a, arrays, cam)
            acc_p, rgb_p, var_p = _render(a)
            a.set_option("plain_kernel", 0)
            acc_g, rgb_g, var_g = _render(a)
            a.set_option("plain_kernel", 1)
            assert (var_p, var_g) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT)
            assert (acc_p != 0).any()
            assert _same(acc_p, acc_g) and np.array_equal(rgb_p, rgb_g)
    finally:
        a.set_option("contract", 0); a.set_option("plain_kernel", 1)


# ---- the table follows ptk_update_geometry ---------------------------------------------------------------------------------------
@gpu
@pytest.mark.parametrize("motion", ["rotation", "mirroring"])
def test_table_follows_a_geometry_update(ctxs, oracle_mod, motion):
    from pbrpathtracer_amd import ptk
    a, b = ctxs
    arrays, cam = three_sampler_cornell()
    first, nv, nn, tb, moved = moved_scenes()[motion]
    if motion == "rotation":                                 # the side walls change arm
        was, now = np.abs(arrays["tbn"][:, 0]), np.abs(moved["tbn"][:, 0])
        assert ((was >= THR) & (now < THR)).any()
    else:                                                    # the windings, and with them the normals, are reversed
        k = slice(first, first + len(nv))
        assert (np.abs((arrays["tbn"][k, 0:3] * np.float32([-1, 1, 1]) * moved["tbn"][k, 0:3]).sum(axis=1) + 1) < 1e-5).all()
    ref, ref8 = _oracle(oracle_mod, moved, cam)
    assert (ref != 0).any() and not _same(ref, _oracle(oracle_mod, arrays, cam)[0])
    _setup(a, arrays, cam)
    _render(a)
    a.update_geometry(first, nv, nn, tb)
    acc_a, rgb_a, var_a = _render(a)
    _setup(b, moved, cam)
    acc_b, rgb_b, var_b = _render(b)
    assert (var_a, var_b) == (ptk.TRACE_FLAT_PLAIN, ptk.TRACE_FLAT_PLAIN)
    assert _same(acc_a, acc_b) and np.array_equal(rgb_a, rgb_b)
    assert _same(acc_a, ref) and np.array_equal(rgb_a, ref8)
    a.set_option("plain_kernel", 0)
    try:
        acc_g, _, var_g = _render(a)
    finally:
        a.set_option("plain_kernel", 1)
    assert var_g == ptk.TRACE_FLAT and _same(acc_a, acc_g)


@gpu
def test_refused_update_leaves_the_table(ctxs, oracle_mod):
    from pbrpathtracer_amd import ptk
    a, _ = ctxs
    arrays, cam = three_sampler_cornell()
    first, nv, nn, tb, _ = moved_scenes()["rotation"]
    ref, ref8 = _oracle(oracle_mod, arrays, cam)
    _setup(a, arrays, cam)
    bad = nv.copy(); bad[5, 4] = np.inf
    with pytest.raises(ptk.PtkError, match=r"\(-4\)"):
        a.update_geometry(first, bad, nn, tb)
    acc, rgb, var = _render(a)
    assert var == ptk.TRACE_FLAT_PLAIN
    assert _same(acc, ref) and np.array_equal(rgb, ref8)
