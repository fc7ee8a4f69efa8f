"""Scenes and motions of tests/test_motion_cpu.py and tests/test_gpu_motion.py (include/ptk.h ptk_render_motion,
ptk_temporal_frame_moving) - a helper, no tests of its own.

A motion is a pair of vertex tables for a sub-range [first, first + n) of a scene's triangles: where they WERE (the state the
geometry snapshot is taken in) and where they ARE (the state the frame is rendered in); every other triangle keeps its uploaded
place, so every image has moved and unmoved pixels.  All arithmetic in float64, cast to float32 once."""
import functools
import math

import numpy as np

import ray_cases as RC

f32 = np.float32
SCENES = ("s_cornell", "random16", "random300", "random6000")
MOTIONS = ("rigid", "scale", "jitter", "collapse", "far")
W, H = 64, 48


def moved_range(case):
    """[first, first + n): from triangle 1 on, a quarter of the scene but at least six triangles - the low indices are the large,
    visible triangles in every scene, and triangle 0 stays put"""
    n = len(RC.scene(case)[0]["verts"])
    return 1, max(6, n // 4)


def _rotation(axis, degrees):
    a = np.asarray(axis, np.float64); a = a / np.linalg.norm(a)
    t = math.radians(degrees)
    K = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + math.sin(t) * K + (1 - math.cos(t)) * (K @ K)


@functools.lru_cache(maxsize=None)
def motion(case, name):
    """(first, was [n, 9] float32, now [n, 9] float32, rigid): rigid = (R, t) in float64 with was = R now + t before the cast, or None"""
    arrays, cam = RC.scene(case)
    first, n = moved_range(case)
    base = np.asarray(arrays["verts"], np.float64).reshape(-1, 3, 3)[first:first + n]
    centre = base.reshape(-1, 3).mean(axis=0)
    rng = np.random.default_rng(len(base) + MOTIONS.index(name))
    rigid = None
    was = base
    if name == "rigid":
        # the frame sees the sub-range turned by 4 degrees about a skew axis through its centre and shifted; it was at the uploaded place
        R = _rotation([0.3, 1.0, 0.2], 4.0); shift = np.array([0.06, -0.03, 0.02])
        now = (base - centre) @ R.T + centre + shift
        # was = R^T (now - centre - shift) + centre
        rigid = (R.T, centre - R.T @ (centre + shift))
    elif name == "scale":
        now = (base - centre) * np.array([1.07, 0.92, 1.04]) + centre
    elif name == "jitter":
        now = base + rng.uniform(-0.04, 0.04, base.shape)
    elif name == "collapse":
        # every second triangle of the sub-range WAS a point (degenerate N': a non-finite n', no history) and is the uploaded triangle
        # now; the others ARE a point now (degenerate N, seen by no pixel) and were the uploaded triangle
        was = base.copy(); now = base.copy()
        was[0::2] = was[0::2, :1]
        now[1::2] = now[1::2, :1]
    elif name == "far":
        # the sub-range came in from far behind the camera: its previous place projects to no pixel
        now = base
        was = base - 1000.0 * np.asarray(cam["dir"], np.float64) + np.array([30.0, 20.0, 0.0])
    else:
        raise KeyError(name)
    return first, np.ascontiguousarray(was.reshape(n, 9), f32), np.ascontiguousarray(now.reshape(n, 9), f32), rigid


def tables(case, name):
    """(previous, current): the scene's whole vertex tables [num_tris][9] in the two states"""
    first, was, now, _ = motion(case, name)
    base = np.ascontiguousarray(RC.scene(case)[0]["verts"], f32).reshape(-1, 9)
    prev = base.copy(); cur = base.copy()
    prev[first:first + len(was)] = was; cur[first:first + len(now)] = now
    return prev, cur


def arrays_now(case, name):
    """the scene with the current state's vertices (normals and tbn as uploaded: ptk_update_geometry with vertices only)"""
    arrays, cam = RC.scene(case)
    return dict(arrays, verts=tables(case, name)[1]), cam


def orbit(cam, degrees, centre=(0.0, 0.0, 0.0)):
    """the camera turned about the vertical axis through `centre`"""
    a = math.radians(degrees)
    R = np.array([[math.cos(a), 0.0, math.sin(a)], [0.0, 1.0, 0.0], [-math.sin(a), 0.0, math.cos(a)]])
    c = np.asarray(centre, np.float64)
    rot = lambda v: (R @ np.asarray(v, np.float64)).astype(f32)
    return dict(cam, pos=(c + R @ (np.asarray(cam["pos"], np.float64) - c)).astype(f32), dir=rot(cam["dir"]), up=rot(cam["up"]))


def previous_camera(case):
    """the camera the motion vectors are taken under: the scene's, two degrees back on its orbit"""
    return orbit(RC.scene(case)[1], -2.0)


def primed_planes(current, seed, extent=1.0):
    """(prev_position, prev_normal) for the planes entries: the current frame's position and normal planes, bit for bit on a third
    of the pixels, shifted by up to 2 % of the extent and turned a little on the rest; 3 % of the valid pixels hold a non-finite
    n' (a degenerate previous triangle) and the invalid pixels hold NaN and 1e30."""
    rng = np.random.default_rng(seed)
    ident, pos, nrm = current[2], np.array(current[3], f32), np.array(current[4], f32)
    H, W = ident.shape
    keep = rng.random((H, W)) < 1.0 / 3.0
    Xp = np.where(keep[..., None], pos, pos + rng.uniform(-0.02, 0.02, (H, W, 3)) * extent).astype(f32)
    npr = np.where(keep[..., None], nrm, nrm + rng.uniform(-0.15, 0.15, (H, W, 3))).astype(f32)
    bad = (rng.random((H, W)) < 0.03) & (ident >= 0)
    npr[bad] = rng.choice(np.array([np.nan, np.inf, -np.inf], f32), (int(bad.sum()), 3))
    inv = ident < 0
    Xp[inv] = np.nan; npr[inv] = f32(1e30)
    return Xp, npr


# ---- the scene of the quality check ---------------------------------------------------------------------------------------------------
# The Cornell box of s_cornell with a striped card in it: CARD_STRIPES quads side by side, alternating between two new diffuse
# materials, tilted about the vertical so that its own plane is not the image plane.  The card slides along x - parallel to the
# image plane of the camera below - by STEP per frame.
CARD_STRIPES = 6
CARD_TILT = 40.0                    # degrees about y
CARD_HALF = (0.45, 0.4)             # half width (along the tilted axis), half height
CARD_START = (-0.55, -0.25, -0.1)   # its centre in the first frame
FRAMES = 8
EXTENT = float(np.linalg.norm([2.0, 2.0, 2.0]))
STEP = EXTENT / 50.0                # world units per frame: about 1.4 pixels at 64 x 48
QUALITY_CAM = dict(pos=np.array([0.0, 0.0, -2.4], f32), dir=np.array([0.0, 0.0, 1.0], f32), up=np.array([0.0, 1.0, 0.0], f32), focal=0.05,
                   fovy=60.0, focal_dist=2.4, aperture=0.0)
QUALITY_SPP, QUALITY_DEPTH, QUALITY_SEED = 4, 4, 100


def card_verts(frame):
    """[2 * CARD_STRIPES][9] float32: the card in frame `frame` (0 .. FRAMES - 1)"""
    t = math.radians(CARD_TILT)
    ax = np.array([math.cos(t), 0.0, math.sin(t)]); ay = np.array([0.0, 1.0, 0.0])
    c = np.asarray(CARD_START, np.float64) + np.array([STEP * frame, 0.0, 0.0])
    out = []
    for s in range(CARD_STRIPES):
        x0 = -CARD_HALF[0] + 2 * CARD_HALF[0] * s / CARD_STRIPES; x1 = -CARD_HALF[0] + 2 * CARD_HALF[0] * (s + 1) / CARD_STRIPES
        a, b = c + ax * x0 - ay * CARD_HALF[1], c + ax * x1 - ay * CARD_HALF[1]
        d, e = c + ax * x1 + ay * CARD_HALF[1], c + ax * x0 + ay * CARD_HALF[1]
        # wound so that cross(e1, e2) faces the camera (-z)
        out += [np.concatenate([a, e, d]), np.concatenate([a, d, b])]
    return np.ascontiguousarray(out, f32)


@functools.lru_cache(maxsize=None)
def quality_scene():
    """(arrays, first card triangle, number of card triangles) with the card in frame 0; shared, not to be modified"""
    base, _ = RC.scene("s_cornell")
    card = card_verts(0)
    n = len(card)
    v = card.astype(np.float64).reshape(n, 3, 3)
    e1, e2 = v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]
    unit = lambda x: x / np.linalg.norm(x, axis=-1, keepdims=True)
    fn = unit(np.cross(e1, e2)); tg = unit(e1); bt = unit(np.cross(fn, tg))
    mats = np.concatenate([base["materials"], base["materials"][:2]])
    first_mat = len(base["materials"])
    mats["diffuse"][first_mat] = (0.15, 0.25, 0.8); mats["diffuse"][first_mat + 1] = (0.85, 0.8, 0.2)
    stripe = (np.arange(n) // 2) % 2
    arrays = dict(base)
    arrays.update(verts=np.concatenate([np.asarray(base["verts"], f32).reshape(-1, 9), card]),
                  normals=np.concatenate([np.asarray(base["normals"], f32).reshape(-1, 9), np.tile(fn, (1, 3)).astype(f32)]),
                  uvs=np.concatenate([np.asarray(base["uvs"], f32), np.zeros((n, 6), f32)]),
                  tbn=np.concatenate([np.asarray(base["tbn"], f32), np.concatenate([fn, tg, bt], axis=1).astype(f32)]),
                  smoothing=np.concatenate([base["smoothing"], np.zeros(n, np.uint8)]),
                  material=np.concatenate([base["material"], (first_mat + stripe).astype(np.int32)]), materials=mats)
    return arrays, len(base["verts"]), n
