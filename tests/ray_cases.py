"""Helper of tests/test_rays_cpu.py and tests/test_gpu_rays.py (include/ptk.h ptk_trace_rays): the scenes, seeded ray sets inside
a scene's bounds and the CPU oracle's radiance along them, summed the way the call defines it."""
import functools

import numpy as np

from conftest import load_golden, scene_from_golden

# FLAT-size scenes, glass, stochastic opacity (the golden micro scenes; s_opacity and random 16 also draw opacity), a FLAT-size random
# scene with textures, the host-built tree (300 triangles) and the device-built tree (6000)
CASES = ("s_cornell", "s_glass", "s_opacity", "random16", "random300", "random6000")
_RANDOM = {"random16": (12, 16), "random300": (14, 300), "random6000": (16, 6000)}


@functools.lru_cache(maxsize=None)
def scene(case):
    """(arrays, camera) of a case; shared, not to be modified"""
    if case in _RANDOM:
        from test_gpu_random_scenes import random_scene
        seed, n = _RANDOM[case]
        return random_scene(seed, n, True)
    z = load_golden(f"tier_{case}.npz")
    cam, proj = z["cam"], z["proj"]
    return scene_from_golden(z), dict(pos=cam[0:3], dir=cam[3:6], up=cam[6:9], focal=float(proj[0]), fovy=float(proj[1]),
                                      focal_dist=float(z["focal_dist"]), aperture=float(z["aperture"]))


def rays_in_box(arrays, n, seed):
    """n rays: origins uniform in the scene's vertex bounding box grown by 10 % of its extent per side, directions uniform on the
    sphere (normalised in float64, then cast); float32 [n, 3] each"""
    rng = np.random.default_rng(seed)
    v = np.asarray(arrays["verts"], np.float64).reshape(-1, 3)
    lo, hi = v.min(axis=0), v.max(axis=0)
    pad = 0.1 * (hi - lo)
    ro = rng.uniform(lo - pad, hi + pad, (n, 3))
    rd = rng.normal(0.0, 1.0, (n, 3))
    rd /= np.linalg.norm(rd, axis=1, keepdims=True)
    return np.ascontiguousarray(ro, np.float32), np.ascontiguousarray(rd, np.float32)


def truth(oracle, ro, rd, depth, seed, first, spp, key_base=0, base=None):
    """out[i] = ((base_i + L(i, first)) + L(i, first + 1)) + ... in float32, L = Oracle.trace_counter (iterative form) on the stream
    of (seed, RNG pixel (key_base + i) mod 2^32, sample)"""
    n = len(ro)
    out = np.zeros((n, 3), np.float32) if base is None else np.array(base, np.float32, copy=True).reshape(n, 3)
    for i in range(n):
        acc = out[i]
        for s in range(first, first + spp):
            acc = (acc + oracle.trace_counter(ro[i], rd[i], depth, seed, (key_base + i) & 0xffffffff, s, 0)).astype(np.float32)
        out[i] = acc
    return out
