"""CPU side of the adaptive ray query and lightmap bake (include/ptk.h ptk_trace_rays_adaptive): the recipe
tests/test_gpu_rays_adaptive.py holds the kernels to is fit for use on the oracle alone - in every scene rays stop at the first
test, run to the end and stop in between, so that array_equal against the mirror exercises every path -, and the mirror
(tests/rays_adaptive_rule.py) has the properties the header states."""
import numpy as np
import pytest

import rays_adaptive_rule as RA

# rays stopping at MIN_SPP / strictly between / running to MAX_SPP, measured on the oracle
MEASURED = {"s_cornell": (126, 55, 19), "s_glass": (123, 37, 40), "s_opacity": (126, 31, 43), "random16": (166, 14, 20),
            "random300": (165, 4, 31)}


@pytest.mark.parametrize("name", RA.CASES)
def test_recipe_exercises_every_path(oracle_mod, name):
    """Conditions on the inputs, not tolerances: no sample is NaN; at least 10 rays stop at 8, at least 10 run to 32 and (but for
    random300, where 4 do) at least 10 stop strictly between."""
    _, _, _, samples = RA.case(name)
    assert samples.shape == (RA.MAX_SPP, RA.N, 3) and not np.isnan(samples).any()
    m = RA.rays(samples, RA.THRESHOLD, RA.MIN_SPP, RA.STEP, RA.MAX_SPP)
    n = m["n"]
    at_min, at_max = int((n == RA.MIN_SPP).sum()), int((n == RA.MAX_SPP).sum())
    between = RA.N - at_min - at_max
    print(f"{name}: {at_min} / {between} / {at_max} rays at {RA.MIN_SPP} / between / at {RA.MAX_SPP}, mean {n.mean():.1f}")
    assert at_min >= 10 and at_max >= 10
    if name != "random300":
        assert between >= 10
    assert (at_min, between, at_max) == MEASURED[name]
    assert (n % RA.STEP == 0).all() and m["ray_samples"] == int(n.sum()) and m["max_count"] == int(n.max())


def test_mirror_properties(oracle_mod):
    _, _, _, samples = RA.case("s_cornell")
    never = RA.rays(samples, 0.0, RA.MIN_SPP, RA.STEP, RA.MAX_SPP)            # the comparison is strict
    assert (never["n"] == RA.MAX_SPP).all() and never["active"] == RA.N and never["rounds"] == RA.MAX_SPP // RA.STEP
    at_once = RA.rays(samples, 1e30, RA.MIN_SPP, RA.STEP, RA.MAX_SPP)
    assert (at_once["n"] == RA.MIN_SPP).all() and at_once["active"] == 0 and at_once["rounds"] == RA.MIN_SPP // RA.STEP
    m = RA.rays(samples, RA.THRESHOLD, RA.MIN_SPP, RA.STEP, RA.MAX_SPP)
    assert (m["n"] % RA.STEP == 0).all() and (m["n"] >= RA.MIN_SPP).all() and (m["n"] <= RA.MAX_SPP).all()
    # the invariant, of the mirror itself: S1, S2 are the folds of the ray's own count
    for i in (0, 17, 199):
        k = int(m["n"][i])
        s1 = np.zeros(3, np.float32); s2 = np.zeros(3, np.float32)
        for s in range(k):
            s1 = s1 + samples[s, i]; s2 = s2 + samples[s, i] * samples[s, i]
        assert np.array_equal(m["S1"][i], s1) and np.array_equal(m["S2"][i], s2)
    # NaN never converges
    bad = samples.copy(); bad[3, 5] = np.nan
    assert RA.rays(bad, 1e30, RA.MIN_SPP, RA.STEP, RA.MAX_SPP)["n"][5] == RA.MAX_SPP


def test_lightmap_neighbourhood_rule():
    """A hand-made need plane: 3x3, clipped to the map, no wrap."""
    need = np.zeros((5, 6), bool)
    need[0, 0] = True; need[3, 5] = True
    want = np.zeros((5, 6), bool)
    want[0:2, 0:2] = True; want[2:5, 4:6] = True
    assert np.array_equal(RA.dilate_in_map(need), want)
    # the loop: 4 x 3 map, texels 0..11 but 5 covered; texel 0 is noisy for ever, the others are constant.  Its neighbours 1, 4 go
    # on with it; 2, 3 (not adjacent: 3 is the end of row 0, 4 the start of row 1 - no wrap), 6, 7, ... stop at the first test.
    W, H = 4, 3
    texel = np.array([0, 1, 2, 3, 4, 6, 7, 8, 9, 10, 11])
    S = 8
    samples = np.full((S, len(texel), 3), 0.5, np.float32)
    samples[::2, 0] = 0.0; samples[1::2, 0] = 4.0
    m = RA.lightmap(samples, texel, W, H, 0.1, 4, 2, 8)
    assert m["n"].tolist() == [8, 8, 4, 4, 8, 4, 4, 4, 4, 4, 4]
    assert m["active"] == 3 and m["rounds"] == 4 and m["ray_samples"] == int(m["n"].sum())
    # without the neighbourhood term only texel 0 goes on
    assert RA.rays(samples, 0.1, 4, 2, 8)["n"].tolist() == [8] + [4] * 10
