"""Scenes, exact expectations and statistics for the stochastic-opacity cases, shared by
tests/test_opacity_expectations_cpu.py (oracle and reference) and tests/test_gpu_opacity_expectations.py (HIP path).

Stochastic opacity (difference 4) is where the port's kernels and the oracle agree because they share one
formula, Rng::opacity.  These cases check that formula against what the reference's `Rand() < opacity` (pathtracer.cpp:469-476)
implies, computed here in float64 from the texel bytes alone:

  * a texel byte b gives alpha = unorm8(b) (float32), a draw is u = k * 2^-24 with k uniform on [0, 2^24), so a candidate is
    accepted with probability exactly ceil(alpha * 2^24) / 2^24 (the reference's Rand() differs by less than 1e-7);
  * every layer is ONE big triangle (a camera ray along a quad's diagonal could draw twice), appended after the scene's
    other triangles so their indices stay put;
  * glowing layers get their colour from a 1x1 emissive TEXTURE on a material whose `emissive` is 0, so they are not lights;
    with diffuse 0, reflectiveness 0 and no light at all a sample's radiance is exactly one layer's one-hot colour or 0, and
    per-pixel accumulator channels are integer counts.

Renders are deterministic for a fixed seed, so the statistical bounds below (|z| <= 5, chi^2 within n +- 5 sqrt(2n),
|r| <= 5 / sqrt(n)) cannot flake; every check runs at two seeds or more.
"""
from __future__ import annotations

import math
import os
import struct
from dataclasses import dataclass, field
from typing import List, Optional, Sequence, Tuple

import numpy as np

from pbrpathtracer_amd import scenes as S

Z_MAX = 5.0
SEEDS = (7, 1234567)

RED, GREEN, BLUE = (255, 0, 0), (0, 255, 0), (0, 0, 255)


# ---- exact expectations -----------------------------------------------------------------------------------------------

def unorm8(b: int) -> np.float32:
    """The texel byte as the renderers read it: (float)b / 255 in float32."""
    return np.float32(np.float32(b) / np.float32(255.0))


def p_accept(b: int) -> float:
    """Exact probability that a candidate behind texel byte b is accepted: P(k * 2^-24 < alpha), k uniform on [0, 2^24)."""
    return math.ceil(float(unorm8(b)) * 2.0 ** 24) / 2.0 ** 24


def first_accepted(ps: Sequence[float]) -> Tuple[List[float], float]:
    """For layers ordered front to back with acceptance probabilities ps: P(the nearest accepted layer is i) and P(none)."""
    out, through = [], 1.0
    for p in ps:
        out.append(through * p)
        through *= 1.0 - p
    return out, through


def through_all(ps: Sequence[float]) -> float:
    return float(np.prod([1.0 - p for p in ps]))


# ---- statistics ---------------------------------------------------------------------------------------------------------

def binom_z(k: float, n: float, p: float) -> float:
    """z-score of k successes in n Bernoulli(p) trials; exact-zero / exact-n outcomes of p in {0, 1} give 0, others inf."""
    if p <= 0.0 or p >= 1.0:
        return 0.0 if k == n * p else math.inf
    return (float(k) - n * p) / math.sqrt(n * p * (1.0 - p))


def assert_binom(k, n, p, what: str) -> float:
    z = binom_z(k, n, p)
    assert abs(z) <= Z_MAX, f"{what}: {int(k)} of {int(n)} = {k / n:.6f}, expected {p:.6f} (z = {z:.2f})"
    return z


def assert_ratio(k1, n1, k0, n0, p: float, what: str) -> float:
    """Two independent binomial samples: the rate k1 / n1 against p times the rate k0 / n0 (for renderers whose draw order
    shifts, so that samples cannot be paired)."""
    r0 = k0 / n0
    r1 = p * r0
    z = (k1 / n1 - r1) / math.sqrt(r1 * (1.0 - r1) / n1 + p * p * r0 * (1.0 - r0) / n0)
    assert abs(z) <= Z_MAX, f"{what}: {k1 / n1:.6f} against {p:.6f} x {r0:.6f} (z = {z:.2f})"
    return z


def assert_dispersion(counts: np.ndarray, spp: int, p: float, what: str) -> float:
    """chi^2 of per-pixel counts against Binomial(spp, p): over- or under-dispersed counts (draws correlated within a pixel's
    samples, or shared between pixels) move it out of n +- 5 sqrt(2n)."""
    c = np.asarray(counts, np.float64).ravel()
    n = c.size
    var = spp * p * (1.0 - p)
    chi2 = float(np.sum((c - spp * p) ** 2) / var)
    assert abs(chi2 - n) <= Z_MAX * math.sqrt(2.0 * n), f"{what}: chi^2 {chi2:.1f} for {n} pixels (spp {spp}, p {p:.4f})"
    return chi2


def corr(a: np.ndarray, b: np.ndarray) -> float:
    a = np.asarray(a, np.float64).ravel(); b = np.asarray(b, np.float64).ravel()
    a = a - a.mean(); b = b - b.mean()
    d = math.sqrt(float(np.dot(a, a)) * float(np.dot(b, b)))
    return float(np.dot(a, b)) / d if d > 0 else (1.0 if np.array_equal(a, b) else 0.0)


def assert_uncorrelated(a: np.ndarray, b: np.ndarray, what: str) -> float:
    r = corr(a, b)
    n = np.asarray(a).size
    assert abs(r) <= Z_MAX / math.sqrt(n), f"{what}: correlation {r:.4f} over {n} pairs (bound {Z_MAX / math.sqrt(n):.4f})"
    return r


def assert_no_spatial_correlation(counts: np.ndarray, what: str) -> Tuple[float, float]:
    """Lag-1 correlation of a count image along x and along y."""
    c = np.asarray(counts, np.float64)
    rx = assert_uncorrelated(c[:, :-1], c[:, 1:], what + " (lag 1 along x)")
    ry = assert_uncorrelated(c[:-1, :], c[1:, :], what + " (lag 1 along y)")
    return rx, ry


def meaningful(spp: int, p: float) -> bool:
    """Per-pixel tests (dispersion, correlation) only where a pixel's count has a spread worth the name."""
    return spp * p * (1.0 - p) >= 2.0


# ---- texture writers ----------------------------------------------------------------------------------------------------

def write_tga(path: str, rgba: np.ndarray) -> None:
    """Uncompressed 32-bit TGA (type 2, top-left origin), for textures that need an alpha channel (PPM has none)."""
    rgba = np.ascontiguousarray(rgba, dtype=np.uint8)
    h, w, c = rgba.shape
    assert c == 4
    os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
    with open(path, "wb") as f:
        f.write(struct.pack("<BBBHHBHHHHBB", 0, 0, 2, 0, 0, 0, 0, 0, w, h, 32, 0x28))
        f.write(rgba[..., [2, 1, 0, 3]].tobytes())


def texture(out_dir: str, texels) -> str:
    """A texture file holding `texels` ([h, w, 3 or 4] bytes; a flat tuple is one texel); RGB as PPM, RGBA as TGA."""
    a = np.asarray(texels, np.uint8)
    if a.ndim == 1:
        a = a.reshape(1, 1, -1)
    name = "tex_" + "_".join(str(int(x)) for x in a.shape) + "_" + a.tobytes().hex()[:48]
    if a.shape[2] == 3:
        path = os.path.join(out_dir, name + ".ppm")
        S.write_ppm(path, a)
    else:
        path = os.path.join(out_dir, name + ".tga")
        write_tga(path, a)
    return path


# ---- scenes -------------------------------------------------------------------------------------------------------------

@dataclass
class Layer:
    """One big triangle in the OBJ plane z = `z`, covering [-extent, extent]^2 of it.
    opacity: None (no opacity texture: opaque), a texel byte b (1x1 texel (b, 255 - b, 255 - b): only red may count), or
    explicit texels for texture(); glow: None or the 1x1 emissive texel; uv: per-vertex uvs (default (0,0), (1,0), (0,1))."""
    z: float
    opacity: object = None
    glow: Optional[Tuple[int, int, int]] = None
    extent: float = 30.0
    diffuse: Tuple[float, float, float] = (0.0, 0.0, 0.0)
    uvs: Optional[np.ndarray] = None


def layer_group(name: str, L: Layer) -> S.MeshGroup:
    e = L.extent
    pos = np.array([[-e, -e, L.z], [3 * e, -e, L.z], [-e, 3 * e, L.z]], np.float64)
    uvs = L.uvs if L.uvs is not None else np.array([[0.0, 0.0], [1.0, 0.0], [0.0, 1.0]])
    return S.MeshGroup(name, pos, np.array([[0, 1, 2]]), np.asarray(uvs, np.float64))


def tri_group(name: str, a, b, c) -> S.MeshGroup:
    return S.MeshGroup(name, np.array([a, b, c], np.float64), np.array([[0, 1, 2]]), np.zeros((3, 2)))


def layer_material(out_dir: str, L: Layer) -> S.MaterialDesc:
    m = S.MaterialDesc(diffuse=L.diffuse, emissive=(0.0, 0.0, 0.0), reflectiveness=0.0, roughness=1.0)
    if L.glow is not None:
        m.textures["emissive"] = texture(out_dir, L.glow)
    if L.opacity is not None:
        op = L.opacity
        if isinstance(op, (int, np.integer)):
            op = (int(op), 255 - int(op), 255 - int(op))
        m.textures["opacity"] = texture(out_dir, op)
    return m


@dataclass
class Built:
    pts: str
    scene: S.SceneDesc
    layer_tris: List[int] = field(default_factory=list)     # triangle index of each layer, in the order given

    @property
    def width(self): return self.scene.width

    @property
    def height(self): return self.scene.height

    @property
    def depth(self): return self.scene.trace_depth


def build(out_dir: str, name: str, base: Sequence[Tuple[S.MeshGroup, S.MaterialDesc]], layers: Sequence[Layer],
          width: int, height: int, depth: int, cam_pos=(0.0, 0.0, -3.5), camera_f: float = 1.0e9, pad: int = 0,
          pow2: bool = False) -> Built:
    """One OBJ object: the base groups, then `pad` off-screen padding triangles (past the FLAT kernel's 16), then the layers.
    pow2: pad (further) to a power-of-two triangle count, for the reference: its tree builder gives a triangle that ends up
    alone in a subtree two leaves (mesh.cpp:182-186), hence TWO opacity draws per ray, and only power-of-two counts never
    split down to a subtree of one (see test_reference_draws_twice_for_a_lone_triangle)."""
    if pow2:
        n = sum(len(g.faces) for g, _ in base) + pad + len(layers)
        pad += (1 << max(1, (n - 1).bit_length())) - n
    d = os.path.join(out_dir, name)
    os.makedirs(d, exist_ok=True)
    groups = [g for g, _ in base]
    mats = [m for _, m in base]
    for i in range(pad):
        x = 200.0 + 3.0 * i
        groups.append(tri_group(f"pad{i}", (x, 200.0, 200.0), (x + 1.0, 200.0, 200.0), (x, 201.0, 200.0)))
        mats.append(S.MaterialDesc(diffuse=(0.5, 0.5, 0.5)))
    ntri0 = sum(len(g.faces) for g in groups)
    for i, L in enumerate(layers):
        groups.append(layer_group(f"layer{i}", L))
        mats.append(layer_material(d, L))
    obj = os.path.join(d, "scene.obj")
    S.write_obj(obj, groups)
    sc = S.SceneDesc(trace_depth=depth, width=width, height=height, cam_pos=tuple(cam_pos), focal_dist=3.5,
                     camera_f=camera_f, pinhole=camera_f >= 1.0e8)
    sc.objects.append(S.ObjectDesc(obj, "scene", [S.ElementDesc(g.name, m) for g, m in zip(groups, mats)]))
    pts = os.path.join(d, "scene.pts")
    S.write_pts(pts, sc)
    return Built(pts, sc, [ntri0 + i for i in range(len(layers))])


# the case scenes: camera at the origin side looking down +z (OBJ x is negated on load; every layer is symmetric enough
# that it does not matter, and the uv split is measured on the STAGED vertices)

STACKS = {
    # front-to-back texel bytes, and whether the layers' triangle indices run front to back
    "a": ((77, 128, 254), True),
    "b": ((1, 128, 254), False),
}
GLOWS = (RED, GREEN, BLUE)


def stack_scene(out_dir: str, stack: str, width: int, height: int, lens: bool = False, **kw) -> Tuple[Built, List[float]]:
    """Case 1: three glowing layers (R, G, B front to back) in front of the camera on no background, trace depth 2, no lights.
    Returns the scene and the layers' acceptance probabilities, front to back."""
    texels, front_first = STACKS[stack]
    zs = (-1.0, -0.5, 0.0)
    layers = [Layer(z, b, g) for z, b, g in zip(zs, texels, GLOWS)]
    order = list(range(3)) if front_first else [2, 1, 0]
    built = build(out_dir, f"stack_{stack}_{int(lens)}_{kw.get('pad', 0)}", [], [layers[i] for i in order], width, height, 2,
                  camera_f=2.0 if lens else 1.0e9, **kw)
    return built, [p_accept(b) for b in texels]


def cornell_base(uv: bool = True) -> List[Tuple[S.MeshGroup, S.MaterialDesc]]:
    g, m = S.cornell_groups(uv)
    return list(zip(g, m))


def edge_scene(out_dir: str, name: str, opacity, width: int, height: int, with_layers: bool = True, **kw) -> Built:
    """Case 2: the Cornell box with three glowing layers across it (camera rays, shadow rays and bounces all cross them).
    opacity: what every layer's opacity slot holds (see Layer)."""
    layers = [Layer(z, opacity, g, extent=1.5) for z, g in zip((-0.5, 0.0, 0.5), GLOWS)] if with_layers else []
    return build(out_dir, name, cornell_base(), layers, width, height, 4, **kw)


def uv_split_scene(out_dir: str, width: int, height: int) -> Built:
    """Case 2, uv at the candidate: a blue-glowing wall behind one red-glowing layer whose 2x1 opacity texture is (0 | 255)
    across u; the layer's u runs along x, the texel edge down the middle of the frame."""
    wall = Layer(1.0, None, BLUE)         # (its material only)
    layer = Layer(0.0, np.array([[[0, 0, 0], [255, 255, 255]]], np.uint8), RED, extent=3.0,
                  uvs=np.array([[0.375, 0.0], [0.875, 0.0], [0.375, 1.0]]))         # u = 0.5 + x / 24: the texel edge at x = 0
    wall_mat = layer_material(os.path.join(out_dir, "uvsplit"), wall)
    # (the wall's barycentric u runs along y: a lookup at the wall's barycentrics - the best hit so far when the layer is
    # tested - would split the frame along another line than the layer's own)
    wall_g = tri_group("wall", (-30.0, -30.0, 1.0), (-30.0, 90.0, 1.0), (90.0, -30.0, 1.0))
    return build(out_dir, "uvsplit", [(wall_g, wall_mat)], [layer], width, height, 2)


def uv_of_candidate(staged: dict, tri: int, ro, dirs: np.ndarray) -> np.ndarray:
    """float64 u texture coordinate where rays (ro, dirs[...]) cross triangle `tri` of the staged scene (NaN off it)."""
    v = np.asarray(staged["verts"], np.float64).reshape(-1, 3, 3)[tri]
    uv = np.asarray(staged["uvs"], np.float64).reshape(-1, 3, 2)[tri]
    d = np.asarray(dirs, np.float64)
    o = np.asarray(ro, np.float64)
    e1, e2 = v[1] - v[0], v[2] - v[0]
    h = np.cross(d, e2)
    a = h @ e1
    s = o - v[0]
    bu = (h @ s) / a
    q = np.cross(s, e1)
    bv = (d @ q) / a
    ok = (bu >= 0) & (bv >= 0) & (bu + bv <= 1)
    u = (1.0 - bu - bv) * uv[0, 0] + bu * uv[1, 0] + bv * uv[2, 0]
    return np.where(ok, u, np.nan)


def shadow_scene(out_dir: str, name: str, layer_texels: Sequence[int], width: int, height: int,
                 light_opacity=None, wall_behind_light: bool = False, **kw) -> Built:
    """Cases 3 and 4: a white diffuse receiver at z = 0 facing the camera (z = -1.5), a small white light at z = -4 behind the
    camera, non-glowing opacity layers between them at z = -2, -2.5, -3 (behind the camera: camera rays never cross them),
    trace depth 1 (the bounce returns 0).  light_opacity: the light's own opacity texel; wall_behind_light: an opaque
    non-emissive wall at z = -5."""
    base = [(tri_group("receiver", (-30, -30, 0.0), (90, -30, 0.0), (-30, 90, 0.0)), S.MaterialDesc(diffuse=(1.0, 1.0, 1.0)))]
    lm = S.MaterialDesc(diffuse=(1.0, 1.0, 1.0), emissive=(1.0, 1.0, 1.0))
    if light_opacity is not None:
        op = light_opacity
        if isinstance(op, (int, np.integer)):
            op = (int(op), 255 - int(op), 255 - int(op))
        lm.textures["opacity"] = texture(os.path.join(out_dir, name), op)
    base.append((tri_group("light", (-0.15, -0.1, -4.0), (0.15, -0.1, -4.0), (0.0, 0.2, -4.0)), lm))
    if wall_behind_light:
        base.append((tri_group("wall", (-30, -30, -5.0), (90, -30, -5.0), (-30, 90, -5.0)), S.MaterialDesc(diffuse=(0.5, 0.5, 0.5))))
    layers = [Layer(z, b, None) for z, b in zip((-2.0, -2.5, -3.0), layer_texels)]
    return build(out_dir, name, base, layers, width, height, 1, cam_pos=(0.0, 0.0, -1.5), **kw)


def joint_scene(out_dir: str, name: str, opacity, width: int, height: int, with_layer: bool = True, **kw) -> Built:
    """Case 5, shadow ray and bounce ray of one sample through the same layer: a white diffuse receiver at z = 0 seen from
    z = -0.5, a small RED light at z = -3 (diffuse 0: Russian roulette ends any bounce that reaches it), and between them, behind
    the camera, one layer at z = -1 wide enough to catch almost every bounce, glowing GREEN (diffuse (0, 1, 0): the light adds
    nothing through it, and roulette keeps 95 % of the bounces that hit it).  Trace depth 2: no roulette at the receiver.
    Per sample, R != 0 means the shadow ray went through, G != 0 means the bounce was stopped by the layer."""
    base = [(tri_group("receiver", (-300, -300, 0.0), (900, -300, 0.0), (-300, 900, 0.0)), S.MaterialDesc(diffuse=(1.0, 1.0, 1.0))),
            (tri_group("light", (-0.15, -0.1, -3.0), (0.15, -0.1, -3.0), (0.0, 0.2, -3.0)),
             S.MaterialDesc(diffuse=(0.0, 0.0, 0.0), emissive=(1.0, 0.0, 0.0)))]
    layers = [Layer(-1.0, opacity, GREEN, extent=300.0, diffuse=(0.0, 1.0, 0.0))] if with_layer else []
    return build(out_dir, name, base, layers, width, height, 2, cam_pos=(0.0, 0.0, -0.5), **kw)


# ---- cameras ------------------------------------------------------------------------------------------------------------

def camera(built: Built) -> dict:
    """(pos, dir, up, focal, fovy, focal_dist, aperture) as Previewer::SetPathTracerCamera derives them; pinhole scenes get
    SetCameraAperture(0)."""
    from pbrpathtracer_amd.pathtracer import camera_from_scene
    cam = camera_from_scene(built.scene)
    if built.scene.pinhole:
        cam["aperture"] = 0.0
    return cam


def staged(built: Built) -> dict:
    """The scene as the host layer stages it from the .pts (host only)."""
    from pbrpathtracer_amd.pathtracer import PathTracer
    pt = PathTracer(0)
    pt.LoadSceneFile(built.pts)
    s = {k: np.array(v, copy=True) for k, v in pt.StagedScene().items()}
    pt.close()
    return s


def oracle(OB, built: Built):
    o = OB.Oracle(staged(built))
    cam = camera(built)
    return o, OB.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])


# ---- the checks, on any renderer ------------------------------------------------------------------------------------------
#
# `render(built, first_sample, spp, seed)` -> accumulator [H, W, 3] float32.

def check_stack(render, built: Built, ps: Sequence[float], spp: int, seeds=SEEDS) -> dict:
    """Case 1: per-channel counts against P_i * prod_{j<i}(1 - P_j), misses against prod(1 - P_j); per-pixel dispersion and
    lag-1 spatial correlation of each channel; the joint rate of the two front layers (adjacent triangle indices on one
    camera ray: layer 2 is seen only when layer 1 let the ray through) factors into its marginals."""
    exp, miss = first_accepted(ps)         # channels R, G, B are the layers front to back
    zs = {}
    for seed in seeds:
        acc = render(built, 0, spp, seed)
        assert np.array_equal(acc, np.round(acc)), "a sample's radiance is not one layer's one-hot colour"
        assert acc.min() >= 0 and np.all(acc.sum(axis=2) <= spp)
        n = acc.shape[0] * acc.shape[1] * spp
        for c in range(3):
            zs[(seed, "RGB"[c])] = assert_binom(acc[..., c].sum(), n, exp[c], f"seed {seed}: layer {c} nearest accepted")
            if meaningful(spp, exp[c]):
                assert_dispersion(acc[..., c], spp, exp[c], f"seed {seed}: layer {c} counts")
                assert_no_spatial_correlation(acc[..., c], f"seed {seed}: layer {c} counts")
        zs[(seed, "miss")] = assert_binom(n - acc.sum(), n, miss, f"seed {seed}: no layer accepted")
        # the joint event "layer 1 rejected AND layer 2 accepted" against (1 - P_1) * P_2, written out as its own check
        assert_binom(acc[..., 1].sum(), n, (1.0 - ps[0]) * ps[1], f"seed {seed}: joint rate of the two front layers")
    return zs


def per_sample(render, built: Built, spp: int, seed: int, first: int = 0) -> np.ndarray:
    """[spp, H, W, 3]: one render(s, 1, seed) per sample."""
    return np.stack([render(built, first + s, 1, seed) for s in range(spp)])


def check_shadow_pairs(plain: np.ndarray, layered: np.ndarray, p_through: float, what: str) -> float:
    """Cases 3 and 4 on the port: every (pixel, sample) of the layered render is bit-identical to the plain one or exactly 0
    (opacity draws do not consume the main stream), and among the samples lit without layers the lit fraction is p_through."""
    assert plain.shape == layered.shape
    same = np.all(layered == plain, axis=-1)
    zero = np.all(layered == 0, axis=-1)
    assert np.all(same | zero), f"{what}: {int(np.sum(~(same | zero)))} samples neither unchanged nor 0"
    lit0 = np.any(plain != 0, axis=-1)
    assert lit0.mean() > 0.5, f"{what}: the plain render is mostly dark ({lit0.mean():.3f})"
    lit = np.any(layered != 0, axis=-1) & lit0
    return assert_binom(lit.sum(), lit0.sum(), p_through, f"{what}: lit fraction")


def check_joint(plain: np.ndarray, opaque: np.ndarray, layered: np.ndarray, p: float, what: str) -> dict:
    """Case 5, shadow and bounce through one layer: on the samples lit without the layer (R of `plain`) whose bounce the opaque
    layer stops (G of `opaque`), R of `layered` says the shadow draw rejected, G says the bounce draw accepted; the two rates
    are 1 - P and P, and their joint rate (1 - P) P.  One draw shared by both rays makes the joint rate 0."""
    A = (plain[..., 0] != 0) & (opaque[..., 1] != 0)
    n = int(A.sum())
    assert n > 0.5 * A.size, f"{what}: only {n} of {A.size} samples usable"
    r = layered[..., 0][A]; g = layered[..., 1][A]
    assert np.all((r == 0) | (r == plain[..., 0][A])), f"{what}: shadow contribution changed other than to 0"
    assert np.all((g == 0) | (g == opaque[..., 1][A])), f"{what}: bounce contribution changed other than to 0"
    R = r != 0; G = g != 0
    return {
        "shadow": assert_binom(R.sum(), n, 1.0 - p, f"{what}: shadow ray through"),
        "bounce": assert_binom(G.sum(), n, p, f"{what}: bounce stopped"),
        "joint": assert_binom((R & G).sum(), n, (1.0 - p) * p, f"{what}: shadow through AND bounce stopped"),
    }
