"""CPU side of the ray queries (include/ptk.h ptk_trace_rays): the recipe tests/test_gpu_rays.py holds the kernel
to - seeded rays inside a scene's bounds, the oracle's orc_trace_counter summed in sample order - is fit for use (enough rays carry
light, none gives NaN: array_equal against it is then a real comparison), and rays.equirect_rays is the panorama it says."""
import numpy as np
import pytest

import ray_cases as RC


@pytest.mark.parametrize("case", RC.CASES)
def test_rays_in_box_carry_light_and_no_nan(oracle_mod, case):
    """A condition on the inputs, not a tolerance: at least a fifth of the 1000 rays have a non-zero sum over 4 samples at depth 4
    (measured 0.50, 0.51, 0.54, 0.30, 0.27, 0.25 in the order of RC.CASES) and no sum is NaN."""
    arrays, _ = RC.scene(case)
    ro, rd = RC.rays_in_box(arrays, 1000, 5)
    assert ro.dtype == np.float32 and rd.dtype == np.float32 and ro.shape == rd.shape == (1000, 3)
    assert np.abs(np.linalg.norm(rd.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    o = oracle_mod.Oracle(arrays)
    t = RC.truth(o, ro, rd, 4, 9, 0, 4)
    o.close()
    lit = float((t != 0).any(axis=1).mean())
    print(f"{case}: {lit:.2f} of the rays carry light")
    assert not np.isnan(t).any()
    assert lit >= 0.2


def test_truth_batches_and_wraps(oracle_mod):
    """truth() itself: a base continues a sum, and the RNG pixel wraps like the oracle's uint32."""
    arrays, _ = RC.scene("s_opacity")
    ro, rd = RC.rays_in_box(arrays, 40, 6)
    o = oracle_mod.Oracle(arrays)
    whole = RC.truth(o, ro, rd, 4, 9, 2, 5)
    assert np.array_equal(RC.truth(o, ro, rd, 4, 9, 4, 3, base=RC.truth(o, ro, rd, 4, 9, 2, 2)), whole)
    wrapped = RC.truth(o, ro, rd, 4, 9, 2, 5, key_base=2 ** 32 - 10)
    assert np.array_equal(wrapped[10:], RC.truth(o, ro[10:], rd[10:], 4, 9, 2, 5, key_base=0))
    assert not np.array_equal(wrapped[:10], whole[:10])
    o.close()


@pytest.mark.parametrize("w,h", [(9, 5), (16, 8), (1, 1)])
def test_equirect_rays(w, h):
    from pbrpathtracer_amd.rays import equirect_rays
    pos = np.array([0.5, -1.0, 2.0])
    d = np.array([0.2, 0.1, -1.0]); up = np.array([0.1, 1.0, 0.0])              # neither unit nor at right angles
    ro, rd = equirect_rays(pos, d, up, w, h)
    assert ro.dtype == np.float32 and rd.dtype == np.float32 and ro.shape == rd.shape == (w * h, 3)
    assert np.array_equal(ro, np.broadcast_to(pos.astype(np.float32), ro.shape))
    assert np.abs(np.linalg.norm(rd.astype(np.float64), axis=1) - 1.0).max() < 1e-6
    f = d / np.linalg.norm(d)
    r = np.cross(up / np.linalg.norm(up), f); r /= np.linalg.norm(r)
    u = np.cross(f, r)
    g = rd.astype(np.float64).reshape(h, w, 3)
    if w % 2 == 1:
        # the centre column lies in the plane of dir and up and faces forward; its middle pixel looks along dir
        assert np.abs(g[:, w // 2] @ r).max() < 1e-6 and (g[:, w // 2] @ f > 0).all()
        if h % 2 == 1:
            assert np.abs(g[h // 2, w // 2] - f).max() < 1e-6
    if h > 1:
        # rows are top-down: the top row looks half a pixel row short of up, every row below it looks lower
        assert np.allclose(g[0] @ u, np.sin(0.5 * np.pi * (1.0 - 1.0 / h)), atol=1e-6)
        assert (np.diff(g @ u, axis=0) < 0).all()
    if w > 2:
        # columns run to the right: the rightmost column of the front half looks furthest right
        assert (g[:, 3 * w // 4 - (1 if w % 4 == 0 else 0)] @ r > 0).all() and (g[:, w // 4] @ r < 0).all()
