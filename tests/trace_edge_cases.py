"""Helper of tests/test_trace_arms_cpu.py and tests/test_gpu_trace_arms.py - no tests of its own: small scenes that drive the arms
of Trace (oracle/pt_oracle.c shade, tex2d, test_triangle, sample_about) which the golden, random and plain-frame scenes never take.

    rr_cap                 materials brighter than the Russian-roulette cap of 0.95 (pathtracer.cpp:590-594)
    tex_edges              one triangle per special texture coordinate, each reading one texel; both clamps of tex2d
    sampler_band           normals with 1 - EPS <= |n.x| < 1 - FLT_EPSILON, where the two sampler forms choose different helpers
    exact_texture_values   roughness / metalness texels of 0, 1, 254 and 255 (255 is exactly 1.0f)
    render_ties            coincident triangles of different emission, in both index orders

Every panel scene is looked at along -x: the panels stand in the plane x = 0 (normals about (+-1, 0, 0), the sampler's pole),
a light triangle behind the camera, one big diffuse triangle behind the panels.  scenes() lists everything with its frame."""
import numpy as np

from conftest import load_golden, scene_from_golden

F32 = np.float32
EPS = F32(0.00001)                                  # PTK_EPS / ORC_EPS (mesh.h:12)
FLT_EPS = F32(1.1920928955078125e-7)
W, H, SPP, SEED = 48, 32, 6, 77
CAM = dict(pos=np.array([3.0, 0.0, 0.0], F32), dir=np.array([-1.0, 0.0, 0.0], F32), up=np.array([0.0, 1.0, 0.0], F32),
           focal=0.05, fovy=40.0, focal_dist=3.0, aperture=0.0)
SLOTS = ("diffuse", "normal", "emissive", "roughness", "metallic", "opacity")      # materials[].tex[k]


def _materials(n):
    from pbrpathtracer_amd import ptk
    m = np.zeros(n, ptk.MATERIAL_DTYPE)
    m["diffuse"] = 0.7; m["specular"] = 1.0; m["emissive_intensity"] = 1.0; m["roughness"] = 1.0; m["translucency"] = 1.0
    m["ior"] = 1.5; m["tex"] = -1
    return m


def pack_textures(images):
    """[H, W, 4] uint8 images -> (textures, texels) of the boundary's atlas"""
    from pbrpathtracer_amd import ptk
    tex = np.zeros(len(images), ptk.TEXTURE_DTYPE); off = 0; chunks = []
    for k, im in enumerate(images):
        h, w = im.shape[:2]
        tex[k] = (w, h, off); chunks.append(np.ascontiguousarray(im, np.uint8).reshape(-1)); off += w * h * 4
    return tex, (np.concatenate(chunks) if chunks else np.zeros(0, np.uint8))


def _unit(v):
    v = np.asarray(v, np.float64)
    return v / np.linalg.norm(v)


def plane_tri(nrm, centre, size):
    """a triangle in the plane through `centre` with the stored normal `nrm` (z = 0), as test_gpu_plain_frames.open_plain_scene
    builds its special triangles: (verts [3, 3], tbn [9]); the winding's normal is nrm's direction"""
    nrm = np.asarray(nrm, np.float64)
    t1 = _unit([-nrm[1], nrm[0], 0.0]); t2 = np.array([0.0, 0.0, 1.0])
    c = np.asarray(centre, np.float64)
    v = np.array([c - size * t1 - size * t2, c + size * t1 - size * t2, c + size * t2]).astype(F32)
    return v, np.concatenate([np.asarray(nrm, F32), t1.astype(F32), t2.astype(F32)])


def panel_scene(panels, materials, images=(), light=True, wall=True, pad=0):
    """panels: dicts with material (index), and optionally uv (one (u, v) for all three vertices), nrm (the stored normal, default
    (1, 0, 0)), cell (panels of one cell coincide; default: its own), vnormals [9] + smoothing, tbn_tail (tangent, bitangent).
    Appends the light's and the wall's materials.  pad: tiny triangles behind the wall, out of every ray's way, that only
    raise the triangle count (over 16: the BVH kernel)."""
    cells = [p.get("cell", k) for k, p in enumerate(panels)]
    ncell = max(cells) + 1
    cols = int(np.ceil(np.sqrt(ncell * 1.5))); rows = int(np.ceil(ncell / cols))
    cw, ch = 3.0 / cols, 2.0 / rows
    size = 0.46 * min(cw, ch)
    verts, tbn, uvs, normals, smoothing, material = [], [], [], [], [], []
    for p, cell in zip(panels, cells):
        cz = -1.5 + cw * (cell % cols + 0.5); cy = -1.0 + ch * (cell // cols + 0.5)
        v, t = plane_tri(p.get("nrm", (1.0, 0.0, 0.0)), (0.0, cy, cz), size)
        if "tbn_tail" in p:
            t[3:9] = np.asarray(p["tbn_tail"], F32)
        verts.append(v.reshape(9)); tbn.append(t)
        uvs.append(np.tile(np.asarray(p.get("uv", (0.25, 0.25)), F32), 3))
        normals.append(np.asarray(p["vnormals"], F32) if "vnormals" in p else np.tile(t[0:3], 3))
        smoothing.append(1 if "vnormals" in p else 0); material.append(p["material"])
    mats = [materials]
    nm = len(materials)

    def extra(v, m):
        v = np.asarray(v, F32)
        e1, e2 = v[1] - v[0], v[2] - v[0]
        n = _unit(np.cross(e1, e2)).astype(F32)
        verts.append(v.reshape(9)); tbn.append(np.concatenate([n, _unit(e1).astype(F32), _unit(np.cross(n, e1)).astype(F32)]))
        uvs.append(np.array([0, 0, 1, 0, 0, 1], F32)); normals.append(np.tile(n, 3)); smoothing.append(0); material.append(m)

    if light:
        lm = _materials(1); lm["emissive"] = (1.0, 0.9, 0.8); lm["emissive_intensity"] = 6.0
        mats.append(lm); extra([[4.0, -6.0, -6.0], [4.0, 0.0, 8.0], [4.0, 6.0, -6.0]], nm); nm += 1
    if wall:
        wm = _materials(1); wm["diffuse"] = (0.5, 0.6, 0.7)
        mats.append(wm); extra([[-1.0, -5.0, -5.0], [-1.0, 5.0, -5.0], [-1.0, 0.0, 7.0]], nm); nm += 1
    for k in range(pad):
        c = np.array([-6.0 - 0.1 * k, -2.0 + 0.3 * (k % 13), -2.0 + 0.37 * (k % 11)])
        extra([c, c + [0.0, 0.05, 0.0], c + [0.0, 0.0, 0.05]], len(materials) - 1 if not wall else nm - 1)
    mats = np.concatenate(mats)
    material = np.array(material, np.int32)
    tex, texels = pack_textures(list(images))
    em = (mats["emissive"][material] ** 2).sum(axis=1) >= float(EPS) ** 2            # pathtracer.cpp:267-273
    return dict(verts=np.array(verts, F32), normals=np.array(normals, F32), uvs=np.array(uvs, F32), tbn=np.array(tbn, F32),
                smoothing=np.array(smoothing, np.uint8), material=material, materials=mats, textures=tex, texels=texels,
                lights=np.nonzero(em)[0].astype(np.int32))


# ---- rr_cap -------------------------------------------------------------------------------------------------------------------
def _golden_cam(z):
    cam, proj = z["cam"], z["proj"]
    return dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]), focal_dist=float(z["focal_dist"]),
                aperture=0.0)


BRIGHT = (((1.0, 1.0, 1.0)), (F32(0.95),) * 3, (np.nextafter(F32(0.95), F32(1)),) * 3, (0.2, 0.96, 0.1), (4.0, 4.0, 4.0))


def rr_cap(kind):
    """The tier-S Cornell box with walls brighter than Russian roulette's cap: `prob = min(0.95f, max(diffuse))` of the UNTEXTURED
    diffuse.  kind: "plain" (untextured, opaque: the PLAIN kernel's), "textured" (plus a wall whose brightness comes only from its
    texture, the material's own diffuse at 0.1, and the reverse), "padded" (textured, 12 triangles outside the box added: a tree),
    "glass" (textured, the walls of type 1).  -> (arrays, camera)"""
    z = load_golden("tier_s_cornell.npz")
    a = {k: np.array(v) for k, v in scene_from_golden(z).items()}
    m = a["materials"]
    for k, d in enumerate(BRIGHT):
        m["diffuse"][k] = d
    if kind != "plain":
        extra = _materials(2)
        extra["diffuse"][0] = 0.1; extra["tex"][0, 0] = 0            # bright by its texture only: prob = 0.1
        extra["diffuse"][1] = 1.0; extra["tex"][1, 0] = 1            # dark by its texture, prob = 0.95 by its own diffuse
        a["materials"] = m = np.concatenate([m, extra])
        a["material"][4] = 6; a["material"][6] = 7
        a["textures"], a["texels"] = pack_textures([np.full((2, 2, 4), 255, np.uint8), np.full((2, 3, 4), 25, np.uint8)])
    if kind == "glass":
        m["type"][:5] = 1; m["type"][6:] = 1; m["translucency"] = 0.5; m["roughness"] = 0.5; m["reflectiveness"] = 0.25
    if kind == "padded":
        n = 12
        c = np.array([3.0, -1.0, 0.0]) + np.arange(n)[:, None] * np.array([0.07, 0.15, 0.0])
        v = np.stack([c, c + [0.0, 0.05, 0.0], c + [0.0, 0.0, 0.05]], axis=1).astype(F32).reshape(n, 9)
        tb = np.tile(np.array([1, 0, 0, 0, 1, 0, 0, 0, 1], F32), (n, 1))
        a["verts"] = np.concatenate([a["verts"], v]); a["tbn"] = np.concatenate([a["tbn"], tb])
        a["normals"] = np.concatenate([a["normals"], np.tile(np.array([1, 0, 0], F32), (n, 3))])
        a["uvs"] = np.concatenate([a["uvs"], np.zeros((n, 6), F32)])
        a["smoothing"] = np.concatenate([a["smoothing"], np.zeros(n, np.uint8)])
        a["material"] = np.concatenate([a["material"], np.zeros(n, np.int32)])
    return a, _golden_cam(z)


# ---- tex_edges ----------------------------------------------------------------------------------------------------------------
TEX_SIZES = ((3, 2), (5, 7), (1, 1), (9, 2))                              # (width, height)
LAST = -1
# coordinate -> the texel column (row) tex2d reads along an axis of n texels: a fixed index, LAST for n - 1, or a function of n.
# Written down from image.cpp:63-86 and the oracle's documented clamps; tests/test_trace_arms_cpu.py checks it against orc_tex2d.
#   -2^-30: fmod gives -2^-30, + 1.0f rounds to 1.0f, n * 1.0f == n: the upper clamp (the reference reads one texel past the row)
#   -2^-24: + 1.0f is 1 - 2^-24 exactly; n * that rounds below n for every n here: the last texel without a clamp
#   NaN, +-inf: x - trunc(x) is NaN; (int)NaN is INT_MIN on the CPU (the lower clamp) and 0 on the GPU: texel 0 by both routes
#   1e30, -1e30, 2^24 + 1: integers as floats, the fraction is (-)0
SPECIALS = (
    ("0", F32(0.0), 0), ("-0", F32(-0.0), 0), ("1", F32(1.0), 0), ("2", F32(2.0), 0), ("-1", F32(-1.0), 0),
    ("-2^-30", F32(-2.0 ** -30), LAST), ("-2^-24", F32(-2.0 ** -24), LAST), ("1-2^-24", F32(1.0 - 2.0 ** -24), LAST),
    ("0.5", F32(0.5), lambda n: n // 2), ("1e30", F32(1e30), 0), ("-1e30", F32(-1e30), 0), ("2^24+1", F32(2.0 ** 24 + 1), 0),
    ("NaN", F32(np.nan), 0), ("+inf", F32(np.inf), 0), ("-inf", F32(-np.inf), 0))
# the coordinates whose texel survives the interpolation w * c + u * c + v * c of three equal vertex coordinates c, which rounds:
# 1, 2, -1 and 1 - 2^-24 come out a rounding error to either side of an integer, that is in the first or the last texel, and 0.5 on
# the boundary of two texels of an even-sized axis.  The others are zeros, non-finite, integers however rounded, or tiny negatives.
STABLE = ("0", "-0", "-2^-30", "-2^-24", "1e30", "-1e30", "2^24+1", "NaN", "+inf", "-inf")
PLAIN_COORD = F32(0.3)


def special_texel(name, n):
    e = {s[0]: s[2] for s in SPECIALS}[name]
    return e(n) if callable(e) else (n - 1 if e == LAST else e)


def edge_texels(w, h):
    """the texels a special coordinate can reach: first and last column, first and last row"""
    m = np.zeros((h, w), bool); m[0, :] = m[-1, :] = True; m[:, 0] = m[:, -1] = True
    return m


def edge_texture(w, h, slot):
    """[h, w, 4] uint8 with every texel distinct in every colour channel.  Per slot the edge texels carry what a wrong texel would
    change: normal - z <= 0 on the first column / row (the nt.z clamp) against z > 0 inside; roughness, metallic - exactly 0, 1, 254 and
    255 in turn; opacity - 255 in the first column (row) and 0 in the last, alternating between, so that a wrong texel flips a hit to a miss."""
    k = np.arange(w * h).reshape(h, w)
    t = np.stack([(k * 37 + 11) % 256, (k * 91 + 5) % 256, 130 + (k * 53) % 126, np.full_like(k, 255)], axis=-1).astype(np.uint8)
    edge = edge_texels(w, h)
    idx = np.cumsum(edge.reshape(-1)).reshape(h, w) - 1
    if SLOTS[slot] == "normal":
        t[0, :, 2] = (k[0, :] * 7) % 128; t[:, 0, 2] = (k[:, 0] * 7 + 3) % 128
    elif SLOTS[slot] in ("roughness", "metallic"):
        t[..., 0] = np.where(edge, np.array([0, 255, 1, 254])[idx % 4], 20 + (k * 37) % 200)
    elif SLOTS[slot] == "opacity":
        pc = np.arange(w) % 2; pc[-1] = 1 if w > 1 else 0               # the first column (row) opaque, the last one clear
        pr = np.arange(h) % 2; pr[-1] = 1 if h > 1 else 0
        t[..., 0] = np.where((pr[:, None] + pc[None, :]) % 2 == 0, 255, 0)   # texel 0, where NaN and the infinities land: opaque
    return t


def tex_edges(slot, size, axis, pad=0):
    """One panel per special coordinate along `axis` ("u", "v", or "uv": both, 30 panels), the other coordinate at 0.3, each reading
    one texel of the size[0] x size[1] texture in `slot` of the panels' material.  -> (arrays, camera, names: panel k's (axis, special))"""
    w, h = size
    mats = _materials(1)
    mats["tex"][0, slot] = 0
    mats["reflectiveness"] = 0.5; mats["roughness"] = 0.5                # the roughness / metallic texels decide the route
    panels, names = [], []
    for ax in (("u", "v") if axis == "uv" else (axis,)):
        for name, c, _ in SPECIALS:
            panels.append(dict(material=0, uv=(c, PLAIN_COORD) if ax == "u" else (PLAIN_COORD, c))); names.append((ax, name))
    a = panel_scene(panels, mats, [edge_texture(w, h, slot)], wall=axis == "uv" or pad > 0, pad=pad)
    return a, CAM, names


def tex_missing(pad=0):
    """six panels whose textures, one slot each, have no texels (an image that failed to load, image.cpp:65-66): they sample as 0"""
    mats = _materials(6)
    mats["reflectiveness"] = 0.5; mats["roughness"] = 0.5
    for s in range(6):
        mats["tex"][s, s] = 0
    a = panel_scene([dict(material=s) for s in range(6)], mats, [np.zeros((0, 0, 4), np.uint8)], pad=pad)
    return a, CAM


# ---- sampler_band ----------------------------------------------------------------------------------------------------------------
ONE = F32(1.0)
BAND_NX = (np.nextafter(ONE - EPS, F32(0)), ONE - EPS, ONE - F32(1e-6), np.nextafter(ONE - FLT_EPS, F32(0)), ONE - FLT_EPS,
           ONE - F32(2.0 ** -24), ONE)
BAND_MATERIALS = ("diffuse", "opaque_lobe", "opaque_rough_one", "mirror", "glass_lobe", "glass_rough_one", "glass_smooth")


def band_class(ax):
    ax = np.abs(F32(ax))
    return "below" if ax < ONE - EPS else ("band" if ax < ONE - FLT_EPS else "pole")


def _band_materials():
    m = _materials(len(BAND_MATERIALS))
    for k, (typ, refl, rough) in enumerate(((0, 0.0, 1.0), (0, 0.5, 0.5), (0, 0.5, 1.0), (0, 0.5, 0.0), (1, 0.3, 0.5), (1, 0.3, 1.0),
                                            (1, 0.3, 0.0))):
        m["type"][k] = typ; m["reflectiveness"][k] = refl; m["roughness"][k] = rough
    m["translucency"] = 0.5
    m["diffuse"] = (0.8, 0.7, 0.6)
    return m


def _band_normals():
    out = []
    for a in BAND_NX:
        y = F32(np.sqrt(max(0.0, 1.0 - float(a) ** 2)))
        out += [(a, y, F32(0)), (-a, y, F32(0))]
    return out


def shading_band_panels(material):
    """two panels whose GEOMETRIC normal is (1, 0, 0), the pole, and whose shading normal lands in the band: by smoothing (three equal
    vertex normals of |x| = 1 - 5e-6, which normalize() keeps within a few ulps) and by a normal map (texel (128, 128, 255) on half-length
    tangents: 0.5 * 0.0039 off the pole, 1 - cos = 3.8e-6)"""
    a = F32(1.0 - 5e-6); v = (a, F32(np.sqrt(1.0 - float(a) ** 2)), F32(0))
    return [dict(material=material, vnormals=np.tile(np.array(v, F32), 3)),
            dict(material=material + len(BAND_MATERIALS), tbn_tail=(0, 0.5, 0, 0, 0, 0.5), uv=(0.5, 0.5))]


def sampler_band(which, pad=0):
    """which: a name of BAND_MATERIALS - its 14 normals (7 values of |n.x|, both signs), for the generic FLAT kernel; "shading" - the
    shading-normal panels of every material; "all" - everything (more than 16 triangles: a tree)"""
    m = _band_materials()
    mapped = m.copy(); mapped["tex"][:, 1] = 0                           # the same materials with the flat normal map
    mats = np.concatenate([m, mapped])
    img = np.zeros((1, 1, 4), np.uint8); img[...] = (128, 128, 255, 255)
    if which in BAND_MATERIALS:                                          # the one material alone: the opaque ones make plain scenes
        k = BAND_MATERIALS.index(which)
        return panel_scene([dict(material=0, nrm=n) for n in _band_normals()], m[k:k + 1], pad=pad), CAM
    panels = []
    kinds = BAND_MATERIALS if which == "all" else []
    for kind in kinds:
        panels += [dict(material=BAND_MATERIALS.index(kind), nrm=n) for n in _band_normals()]
    if which in ("all", "shading"):
        for k in range(len(BAND_MATERIALS)):
            panels += shading_band_panels(k)
    return panel_scene(panels, mats, [img], pad=pad), CAM


# ---- exact_texture_values ---------------------------------------------------------------------------------------------------------
def exact_texture_values(kind, pad=0):
    """kind "opaque" / "glass" / "both": panels of roughness- and of metalness-mapped materials reading the bytes 0, 1, 254 and 255"""
    img = np.zeros((2, 2, 4), np.uint8)
    img[..., 0] = [[0, 1], [254, 255]]; img[..., 1:] = 99
    kinds = (0, 1) if kind == "both" else ((0,) if kind == "opaque" else (1,))
    mats = _materials(2 * len(kinds)); panels = []
    for j, typ in enumerate(kinds):
        mats["type"][2 * j:2 * j + 2] = typ
        mats["reflectiveness"][2 * j] = 0.6; mats["tex"][2 * j, 3] = 0           # roughness from the texture
        mats["roughness"][2 * j + 1] = 0.5; mats["tex"][2 * j + 1, 4] = 0        # reflectiveness from the texture
        for mm in (2 * j, 2 * j + 1):
            panels += [dict(material=mm, uv=(u, v)) for v in (0.25, 0.75) for u in (0.25, 0.75)]
    mats["translucency"] = 0.5
    return panel_scene(panels, mats, [img], pad=pad), CAM


# ---- render_ties ---------------------------------------------------------------------------------------------------------------------
def render_ties(n_pairs, pad=0, others=0, rotate=True):
    """n_pairs pairs of coincident emissive triangles, red and green; in even pairs red has the smaller index, in odd pairs green.  The
    second of a pair lists the same three vertices from the next one on: the same plane and the same t, another centroid sum, so
    that a tree sorted by centroids may meet the larger index first - and t a rounding error apart on some rays, where the nearer of
    the two wins whatever its index.  rotate=False: exact copies, every hit a tie.  others: plain diffuse panels in cells of their own."""
    mats = _materials(3)
    mats["emissive"][0] = (1.0, 0.1, 0.1); mats["emissive"][1] = (0.1, 1.0, 0.1); mats["emissive_intensity"] = 2.0
    mats["emissive_intensity"][2] = 0.0
    first = [dict(material=k % 2, cell=k) for k in range(n_pairs)] + [dict(material=2, cell=n_pairs + k) for k in range(others)]
    second = [dict(material=1 - k % 2, cell=k) for k in range(n_pairs)]
    a = panel_scene(first + second, mats, light=False, wall=True, pad=pad)
    n0 = len(first)
    for k in range(n_pairs if rotate else 0):                             # the twin: vertices rotated by one or two (same winding)
        v = a["verts"][k].reshape(3, 3)
        a["verts"][n0 + k] = np.roll(v, -(1 + k % 2), axis=0).reshape(9)
    return a, CAM


# ---- direct lighting's dead ends ---------------------------------------------------------------------------------------------------
def no_lights():
    """plain diffuse and mirror panels before the wall and nothing that emits: DirectIllumimation returns at once (pathtracer.cpp:506-507)"""
    m = _materials(2); m["reflectiveness"][1] = 0.5; m["roughness"][1] = 0.0
    return panel_scene([dict(material=k % 2) for k in range(6)], m, light=False), CAM


def lost_light():
    """the only light is a triangle of zero area (emissive, so a light: pathtracer.cpp:267-273): Moeller-Trumbore never hits it, and a
    shadow ray from a panel towards it leaves the scene - it misses everything, which counts as lit (pathtracer.cpp:522-526)"""
    m = _materials(2); m["emissive"][1] = (1.0, 0.8, 0.6); m["emissive_intensity"][1] = 5.0
    a = panel_scene([dict(material=0) for _ in range(6)] + [dict(material=1)], m, light=False, wall=False)
    a["verts"][6] = np.tile(np.array([4.0, 0.5, 0.25], F32), 3)
    assert list(a["lights"]) == [6]
    return a, CAM


# ---- the list ------------------------------------------------------------------------------------------------------------------------
def scenes():
    """(name, arrays, camera, W, H, D, spp, seed) of every edge scene: what tests/test_gpu_trace_arms.py renders"""
    out = []

    def add(name, ac, D=4, spp=SPP):
        out.append((name, ac[0], ac[1], W, H, D, spp, SEED))

    for kind in ("plain", "textured", "padded", "glass"):
        for D in (1, 2, 3):
            add(f"rr_cap_{kind}_D{D}", rr_cap(kind), D=D, spp=4)
    for slot in range(6):
        for size in TEX_SIZES:
            tag = f"{SLOTS[slot]}_{size[0]}x{size[1]}"
            add(f"tex_edges_u_{tag}", tex_edges(slot, size, "u")[:2])
            add(f"tex_edges_v_{tag}", tex_edges(slot, size, "v")[:2])
            add(f"tex_edges_uv_{tag}", tex_edges(slot, size, "uv")[:2])
    add("tex_missing", tex_missing()); add("tex_missing_padded", tex_missing(pad=12))
    for kind in BAND_MATERIALS:
        add(f"sampler_band_{kind}", sampler_band(kind))
    add("sampler_band_shading", sampler_band("shading"))
    add("sampler_band_all", sampler_band("all"), spp=8)
    for kind in ("opaque", "glass"):
        add(f"exact_texture_values_{kind}", exact_texture_values(kind))
    add("exact_texture_values_both", exact_texture_values("both", pad=4))
    add("no_lights", no_lights()); add("lost_light", lost_light())
    add("render_ties_flat", render_ties(6, others=3))
    add("render_ties_exact", render_ties(6, others=3, rotate=False))
    add("render_ties_tree", render_ties(12, pad=6, others=6))
    return out
