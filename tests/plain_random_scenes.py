"""Helper of tests/test_plain_random_cpu.py, tests/test_gpu_plain_random.py and tools/soak_plain_scenes.py - no tests of its own: a
seeded generator of PLAIN scenes (16 triangles or fewer, opaque untextured type-0 materials, nothing smoothed, a pinhole) and the
fixed family of them that the two test files render.

The hand-made PLAIN scenes are all edits of the golden Cornell box: a closed room of round numbers seen from one camera.  A scene of
plain_scene() is a shuffled list of groups cut to n records - a light rectangle facing down, for n >= 6 a large floor and back wall,
fan-split rectangles and triangles in random axis planes, oblique triangles, now and then a zero-area record - at non-round float
coordinates, open, from a camera that moves with the seed.  The groups are what the PLAIN pass tells apart: the sixteen zero classes
and the six pair kinds of csrc/ptk_flat_mt.h, pair prefixes of every length, single records right behind a prefix.

variant (the stress forms of tools/soak_random_scenes.py's vary, and the directed compositions):
    0   as generated
    1   vertices snapped to a grid of 1/4: coplanar faces, shared edges, rays through exact edges
    2,3 scene and camera scaled by 0.03 / by 1e3
    4   the last one or two records are bitwise copies of the first (coincident twins with equal t: a pair against singles), of
        another material and not lights: a tie that goes to the larger index shows in the image
    5   axis-plane groups moved to the plane coordinate 0 with zeros of either sign at their vertices: stored edge words of -0.0
    6   an empty light list
    7   the camera's position takes one rectangle's plane coordinate, its direction is exactly -z: rays with zero direction
        components, a zero determinant against that plane
    8   the last two records are test_gpu_plain_frames.open_plain_scene's threshold triangles: |n.x| one ulp under and exactly at
        1 - PTK_EPS, the second of them on a material picked by the seed's parity (the lobe or the roughness-1 reflector)
    9   rectangles only: a pair prefix of n // 2
    10  one oblique record in front of rectangles only (n >= 3): an empty prefix with pairs behind it
The floor and the wall are there when the random part has six records or more (variants 4 and 8 take their last records from it); a
scene of one record is the light's first half."""
import numpy as np

from test_gpu_plain_frames import _tbn_of, open_plain_scene

F32 = np.float32
VARIANTS = tuple(range(11))
LIGHT, LOBE, BRIGHT, ROUGH_ONE, MATT = 0, 1, 2, 3, 4          # the five materials
BOX_LO = np.array([-2.0, -1.4, -2.0]); BOX_HI = np.array([2.0, 1.4, 1.2])     # where the random groups lie


def _glm_unit(x):
    """glm::normalize in float32: x * (1 / sqrt(dot))"""
    x = np.asarray(x, F32)
    sqr = F32(F32(F32(x[0] * x[0]) + F32(x[1] * x[1])) + F32(x[2] * x[2]))
    inv = F32(F32(1.0) / F32(np.sqrt(sqr)))
    return np.array([F32(x[0] * inv), F32(x[1] * inv), F32(x[2] * inv)], F32)


def _camera_dir(rng):
    """a random direction about -z that glm::normalize reproduces bit for bit: ptk_set_camera normalises what it is given, the
    oracle's camera takes it as it is, and in float32 normalising twice is not always a no-op"""
    for _ in range(1000):
        d = _glm_unit(_glm_unit(np.array([-0.03, 0.05, -1.0]) + rng.uniform(-0.08, 0.08, 3)))
        if np.array_equal(_glm_unit(d), d):
            return d
    raise AssertionError("no direction that normalises to itself")


def _signed_zero(rng):
    return F32(-0.0) if rng.integers(0, 2) else F32(0.0)


def _lift(rng, p, c, pts2, zeros):
    """in-plane points [k, 2] on axes (p + 1) % 3, (p + 2) % 3 -> vertices [k, 3] float32 in the plane x_p = c; zeros: c is 0 and
    every vertex gets its own sign of it"""
    v = np.zeros((len(pts2), 3), F32)
    v[:, (p + 1) % 3] = pts2[:, 0]; v[:, (p + 2) % 3] = pts2[:, 1]
    for k in range(len(v)):
        v[k, p] = _signed_zero(rng) if zeros else F32(c)
    return v


def _rect(rng, p, c, lo2, size2, zeros=False, facing=0):
    """the two records of a fan-split rectangle in the plane x_p = c: corner lo2, sides size2 on the two other axes (sums formed
    once in float32, so that equal coordinates are equal bits), a random fan start and winding; facing = +-1 asks for the sign of
    the winding's normal on axis p instead of a random one"""
    a0, b0 = F32(lo2[0]), F32(lo2[1])
    a1, b1 = F32(a0 + F32(size2[0])), F32(b0 + F32(size2[1]))
    q = _lift(rng, p, c, np.array([[a0, b0], [a1, b0], [a1, b1], [a0, b1]], F32), zeros)
    if rng.integers(0, 2):
        q = q[::-1]
    if facing:
        nrm = np.cross(q[1].astype(np.float64) - q[0], q[2].astype(np.float64) - q[0])[p]
        if nrm * facing < 0:
            q = q[::-1]
    q = np.roll(q, -int(rng.integers(0, 4)), axis=0)
    return np.array([[q[0], q[1], q[2]], [q[0], q[2], q[3]]], F32)


def _random_rect(rng, zeros=False):
    p = int(rng.integers(0, 3)); i, j = (p + 1) % 3, (p + 2) % 3
    c = rng.uniform(BOX_LO[p], BOX_HI[p])
    size = rng.uniform(0.5, 1.8, 2)
    lo = np.array([rng.uniform(BOX_LO[i], BOX_HI[i] - 0.5 * size[0]), rng.uniform(BOX_LO[j], BOX_HI[j] - 0.5 * size[1])])
    return _rect(rng, p, c, lo, size, zeros)


def _plane_triangle(rng, zeros=False):
    """a triangle in a random axis plane: a third each with no axis-parallel edge, with e1 and with e2 parallel to an in-plane axis"""
    p = int(rng.integers(0, 3)); i, j = (p + 1) % 3, (p + 2) % 3
    c = rng.uniform(BOX_LO[p], BOX_HI[p])
    centre = np.array([rng.uniform(BOX_LO[i], BOX_HI[i]), rng.uniform(BOX_LO[j], BOX_HI[j])])
    pts = (centre + rng.uniform(-1.2, 1.2, (3, 2))).astype(F32)
    form = int(rng.integers(0, 3))
    if form:
        ax = int(rng.integers(0, 2))                         # the in-plane axis the edge is parallel to: the OTHER coordinate is v0's
        pts[form, 1 - ax] = pts[0, 1 - ax]
    return _lift(rng, p, c, pts, zeros)[None]


def _oblique(rng):
    centre = rng.uniform(BOX_LO, BOX_HI)
    return (centre + rng.uniform(-1.3, 1.3, (3, 3))).astype(F32)[None]


def _zero_area(rng):
    v0 = rng.uniform(BOX_LO, BOX_HI).astype(F32)
    v2 = v0 if rng.integers(0, 2) else rng.uniform(BOX_LO, BOX_HI).astype(F32)
    return np.array([[v0, v0, v2]], F32)                     # e1 is all zero: general class, never hit


def _materials(rng, lambert):
    from pbrpathtracer_amd import ptk
    m = np.zeros(5, ptk.MATERIAL_DTYPE)
    m["type"] = 0; m["tex"] = -1
    m["diffuse"] = rng.uniform(0.2, 0.9, (5, 3))
    m["specular"] = rng.uniform(0.3, 1.0, (5, 3))
    m["emissive_intensity"] = 1.0
    m["translucency"] = rng.choice([0.0, 0.6, 1.0], 5)      # (no meaning for an opaque material: "whatever its other fields hold")
    m["ior"] = rng.uniform(1.1, 1.9, 5)
    refl = rng.choice([0.0, 0.5, 1.0], 5); rough = rng.choice([0.0, 0.4, 1.0], 5)
    refl[LIGHT] = 0.0
    if refl[LOBE] == 0.0: refl[LOBE] = 0.5
    rough[LOBE] = 0.4                                        # the lobe sampler: reflectiveness > 0, 0 < roughness < 1
    m["reflectiveness"] = 0.0 if lambert else refl
    m["roughness"] = rough
    m["diffuse"][BRIGHT, int(rng.integers(0, 3))] = rng.uniform(0.97, 1.0)    # above Russian roulette's cap of 0.95
    m["emissive"][LIGHT] = (1.0, 0.9, 0.8); m["emissive_intensity"][LIGHT] = 8.0
    return m


def plain_scene(seed, n, variant=0, lambert=False):
    """-> (arrays, cam): the arrays of test_gpu_random_scenes.random_scene, the camera a dict for Context.set_camera"""
    assert 1 <= n <= 16 and variant in VARIANTS
    rng = np.random.default_rng([int(seed), int(n), int(variant)])
    mats = _materials(rng, lambert)
    tail = {4: 0 if n == 1 else 1 if n < 4 else 2, 8: min(2, n - 1)}.get(variant, 0)
    body = n - tail
    zeros = variant == 5
    only_rects = variant in (9, 10)

    # ---- the groups: (records [k, 3, 3], material, is light, mandatory) -----------------------------------------------------------
    light = (_rect(rng, 1, rng.uniform(1.2, 1.45), (rng.uniform(-1.4, -0.9), rng.uniform(-1.9, -1.5)),
                   (rng.uniform(1.9, 2.6), rng.uniform(1.7, 2.3)), facing=-1), LIGHT, True, True)
    chosen = [light]
    if body >= (7 if variant == 10 else 6):
        chosen.append((_rect(rng, 1, rng.uniform(-1.75, -1.5), (rng.uniform(-4.4, -3.8), rng.uniform(-2.45, -2.25)),
                             (rng.uniform(7.7, 8.6), rng.uniform(5.6, 6.2))), BRIGHT, False, True))          # the floor
        chosen.append((_rect(rng, 2, rng.uniform(-2.3, -2.05), (rng.uniform(-4.4, -3.8), rng.uniform(-3.3, -2.8)),
                             (rng.uniform(7.7, 8.6), rng.uniform(5.7, 6.4))), LOBE, False, True))            # the back wall
    if variant == 10 and body >= 3:
        chosen.append((_oblique(rng), LOBE, False, True))
    while sum(len(g[0]) for g in chosen) < body:
        kind = 0 if only_rects else int(rng.choice([0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 2, 3]))      # a zero-area record: sometimes
        z = zeros and bool(rng.integers(0, 2))
        rec = (_random_rect, _plane_triangle, _oblique, _zero_area)[kind](rng, *((z,) if kind < 2 else ()))
        used_lobe = any(g[1] == LOBE for g in chosen)
        chosen.append((rec, int(rng.integers(1, 5)) if used_lobe else LOBE, False, False))                   # the lobe material is used

    # ---- shuffled and cut to `body` records: the cut may halve a free rectangle, never a mandatory group -------------------------
    order = [chosen[k] for k in rng.permutation(len(chosen))]
    if variant == 10 and body >= 3:
        order.sort(key=lambda g: len(g[0]) != 1)                                 # (stable: the one single record comes first)
    if sum(len(g[0]) for g in order) > body and body >= 2 and (order[-1][3] or len(order[-1][0]) == 1):
        k = [k for k, g in enumerate(order) if not g[3] and len(g[0]) == 2][-1]  # (the overshoot came from a free rectangle)
        order.append(order.pop(k))
    verts = np.concatenate([g[0] for g in order])[:body]
    material = np.concatenate([[g[1]] * len(g[0]) for g in order])[:body].astype(np.int32)
    is_light = np.concatenate([[g[2]] * len(g[0]) for g in order])[:body]

    # ---- the variants ---------------------------------------------------------------------------------------------------------
    cam = dict(pos=(np.array([0.1, -0.2, 3.2]) + rng.uniform(-0.3, 0.3, 3)).astype(F32),
               dir=_camera_dir(rng), up=np.array([0.0, 1.0, 0.0], F32),
               focal=0.05, fovy=float(rng.uniform(45.0, 68.0)), focal_dist=3.0, aperture=0.0)
    if variant == 1:
        verts = (np.round(verts * F32(4.0)) / F32(4.0)).astype(F32)
    if variant in (2, 3):
        sc = F32(0.03 if variant == 2 else 1e3)
        verts = (verts * sc).astype(F32)
        cam["pos"] = (cam["pos"] * sc).astype(F32); cam["focal"] = float(F32(cam["focal"]) * sc); cam["focal_dist"] = float(F32(3.0) * sc)
    if variant == 4 and tail:
        verts = np.concatenate([verts, verts[:tail]])
        material = np.concatenate([material, [m % 4 + 1 for m in material[:tail]]]).astype(np.int32)         # never the emitter's
        is_light = np.concatenate([is_light, [False] * tail])
    tbn = _tbn_of(verts.reshape(-1, 9))
    if variant == 8 and tail:
        o, _ = open_plain_scene(30, 16)
        verts = np.concatenate([verts, o["verts"].reshape(16, 3, 3)[15 - tail:15]])
        tbn = np.concatenate([tbn, o["tbn"][15 - tail:15]])
        band = ROUGH_ONE if seed & 1 else LOBE
        if not lambert:
            mats["reflectiveness"][ROUGH_ONE] = 0.5; mats["roughness"][ROUGH_ONE] = 1.0
        material = np.concatenate([material, [MATT, band][2 - tail:]]).astype(np.int32)
        is_light = np.concatenate([is_light, [False] * tail])
    if variant == 7:
        v = verts.reshape(-1, 3, 3)
        flat_on = [(k, p) for k in range(len(v)) for p in (0, 1) if (v[k, :, p] == v[k, 0, p]).all() and abs(v[k, 0, p]) < 1.9 and (v[k, 1:] != v[k, 0]).any()]
        k, p = flat_on[int(rng.integers(0, len(flat_on)))]
        cam["pos"][p] = v[k, 0, p]
        cam["dir"] = np.array([0.0, 0.0, -1.0], F32)
    assert len(verts) == n
    lights = np.zeros(0, np.int32) if variant == 6 else np.nonzero(is_light)[0].astype(np.int32)
    arrays = dict(verts=np.ascontiguousarray(verts.reshape(n, 9)), normals=np.ascontiguousarray(np.tile(tbn[:, 0:3], (1, 3))),
                  uvs=rng.uniform(-1.5, 2.5, (n, 6)).astype(F32), tbn=np.ascontiguousarray(tbn), smoothing=np.zeros(n, np.uint8),
                  material=material, materials=mats, textures=np.zeros(0, _texture_dtype()), texels=np.zeros(0, np.uint8), lights=lights)
    return arrays, cam


def _texture_dtype():
    from pbrpathtracer_amd import ptk
    return ptk.TEXTURE_DTYPE


# ---- the family --------------------------------------------------------------------------------------------------------------------
# (seed, n, variant, lambert, W, H, D, spp).  n cycles through 1, 2, 3, 5, 8, 11, 12, 13, 14, 15, 16, 16; D through 1..8; spp takes every
# value 3..11; six of the eight frame sizes are no multiple of the 16 x 16 tile in either direction; the variant of row k is 7 k mod 9,
# but for the two scenes of the light alone that a camera in the light's plane would show black (they swapped with rows of 15 records);
# two rows in five are Lambert.  Seeds are 1000 + the row's number
# unless that scene missed a condition of tests/test_plain_random_cpu.py (the lit share, a prefix length nothing else has, the band
# triangle's material): then the next seed in steps of 101 that meets it.  The last three rows are the directed compositions.
FAMILY = (
    (1000, 1, 0, False, 33, 17, 1, 3),
    (1001, 2, 0, True, 47, 29, 2, 7),
    (1002, 3, 5, False, 48, 32, 3, 11),
    (1003, 5, 3, True, 64, 48, 4, 6),
    (2014, 8, 1, False, 40, 33, 5, 10),
    (1005, 11, 8, False, 35, 47, 6, 5),
    (1006, 12, 6, True, 56, 40, 7, 9),
    (3431, 13, 4, False, 61, 23, 8, 4),
    (1008, 14, 2, True, 33, 17, 1, 8),
    (1009, 15, 7, False, 47, 29, 2, 3),
    (1010, 16, 7, False, 48, 32, 3, 7),
    (1011, 16, 5, True, 64, 48, 4, 11),
    (1012, 1, 3, False, 40, 33, 5, 6),
    (1013, 2, 1, True, 35, 47, 6, 10),
    (1014, 3, 8, False, 56, 40, 7, 5),
    (1015, 5, 6, False, 61, 23, 8, 9),
    (1016, 8, 4, True, 33, 17, 1, 4),
    (1017, 11, 2, False, 47, 29, 2, 8),
    (1624, 12, 0, True, 48, 32, 3, 3),
    (1019, 13, 7, False, 64, 48, 4, 7),
    (1020, 14, 5, False, 40, 33, 5, 11),
    (1021, 15, 3, True, 35, 47, 6, 6),
    (1022, 16, 1, False, 56, 40, 7, 10),
    (1023, 16, 8, True, 61, 23, 8, 5),
    (1024, 1, 6, False, 33, 17, 1, 9),
    (1025, 2, 4, False, 47, 29, 2, 4),
    (1026, 3, 2, True, 48, 32, 3, 8),
    (1027, 5, 0, False, 64, 48, 4, 3),
    (1028, 8, 7, True, 40, 33, 5, 7),
    (1029, 11, 5, False, 35, 47, 6, 11),
    (1030, 12, 3, False, 56, 40, 7, 6),
    (9313, 13, 1, True, 61, 23, 8, 10),
    (1032, 14, 8, False, 33, 17, 1, 5),
    (1033, 15, 6, True, 47, 29, 2, 9),
    (1034, 16, 4, False, 48, 32, 3, 4),
    (1035, 16, 2, False, 64, 48, 4, 8),
    (1036, 1, 0, True, 40, 33, 5, 3),
    (1037, 2, 0, False, 35, 47, 6, 7),
    (1038, 3, 5, True, 56, 40, 7, 11),
    (1039, 5, 3, False, 61, 23, 8, 6),
    (1949, 8, 1, False, 33, 17, 1, 10),
    (1041, 11, 8, True, 47, 29, 2, 5),
    (1042, 12, 6, False, 48, 32, 3, 9),
    (1043, 13, 4, True, 64, 48, 4, 4),
    (1044, 14, 2, False, 40, 33, 5, 8),
    (1045, 15, 7, False, 35, 47, 6, 3),
    (1046, 16, 7, True, 56, 40, 7, 7),
    (1047, 16, 5, False, 61, 23, 8, 11),
    (2000, 14, 9, True, 47, 29, 5, 5),                      # rectangles only: a prefix of 7
    (2102, 16, 9, False, 56, 40, 6, 6),                     # ... of 8
    (2002, 13, 10, False, 40, 33, 4, 7),                    # an oblique record in front of rectangles only
)
ROW_IDS = ["%d-n%d-v%d%s" % (r[0], r[1], r[2], "-lambert" if r[3] else "") for r in FAMILY]
# the option sets every row is rendered under beside the default: (option, value it is rendered with, value it is put back to)
OPTION_SETS = (("flat_cycle", 0, 1), ("flat_rect_pairs", 0, 1), ("flat_zero_classes", 0, 1), ("lambert_kernel", 0, 1), ("plain_kernel", 0, 1),
               ("flat", 0, 1))


def row_scene(row):
    seed, n, variant, lambert = row[:4]
    return plain_scene(seed, n, variant, lambert)


def classify(arrays):
    """(zero class of every record, kinds of the pair prefix) by the host's classifiers: what the device must say after an upload"""
    from pbrpathtracer_amd import ptk
    v = np.asarray(arrays["verts"], F32).reshape(-1, 3, 3)
    return [ptk.flat_zero_class(*t) for t in v], ptk.flat_rect_prefix(arrays["verts"])


def oracle_image(OB, arrays, cam, row, rank=0, world=1):
    """(float accumulator, RGB8) of a row's frame on the CPU oracle, read-only"""
    seed, _, _, _, W, H, D, spp = row
    o = OB.Oracle(arrays)
    tot, rgb = o.render(OB.make_camera(**cam), W, H, D, 0, spp, seed, rank=rank, world=world)
    o.close()
    tot.setflags(write=False); rgb.setflags(write=False)
    return tot, rgb


# ---- geometry updates between family members -------------------------------------------------------------------------------------------
# (row A, row B) by their places in FAMILY: equal n, neither scaled; the material table and the triangles' materials stay A's.  The
# first pair lengthens A's pair prefix, the second shortens it (tests/test_plain_random_cpu.py asserts that).
UPDATE_PAIRS = ((19, 31), (49, 22), (11, 49), (6, 18), (5, 29), (48, 32))


def mixed_scene(ia, ib):
    """-> (A's arrays, A's camera, first, B's verts / normals / tbn of a random proper sub-range [first, first + count), the mixed arrays)"""
    ra, rb = FAMILY[ia], FAMILY[ib]
    assert ra[1] == rb[1] and ra[2] not in (2, 3) and rb[2] not in (2, 3)
    a, cam = row_scene(ra); b, _ = row_scene(rb)
    n = ra[1]
    rng = np.random.default_rng([ra[0], rb[0]])
    count = int(rng.integers(n // 2, n)); first = int(rng.integers(0, n - count + 1))
    k = slice(first, first + count)
    m = dict(a)
    for key in ("verts", "normals", "tbn"):
        m[key] = a[key].copy(); m[key][k] = b[key][k]
    return a, cam, first, b["verts"][k].copy(), b["normals"][k].copy(), b["tbn"][k].copy(), m
