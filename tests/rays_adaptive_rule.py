"""numpy float32 mirror of the adaptive ray query and the adaptive lightmap bake (include/ptk.h ptk_trace_rays_adaptive,
ptk_bake_lightmap_adaptive), built on adaptive_rule.done / fold.  Given every sample of every ray, it says what each ray must hold
afterwards - its count, S1 and S2 folded in sample order - and what the result struct reports.  Helper of
tests/test_rays_adaptive_cpu.py and tests/test_gpu_rays_adaptive.py."""
import functools

import numpy as np

import adaptive_rule as AR
import ray_cases as RC

f32 = np.float32

# the recipe of both test files: 200 rays_in_box rays, depth 4, threshold 0.1, rounds of 4 samples, 8 before the first test, 32 at most
N, RAY_SEED, DEPTH, SEED, THRESHOLD, STEP, MIN_SPP, MAX_SPP = 200, 5, 4, 7, 0.1, 4, 8, 32
CASES = ("s_cornell", "s_glass", "s_opacity", "random16", "random300")


def dilate_in_map(need):
    """[H][W] bool -> texels with a `need` texel in their 3x3 neighbourhood clipped to the map"""
    H, W = need.shape
    p = np.zeros((H + 2, W + 2), bool)
    p[1:-1, 1:-1] = need
    out = np.zeros((H, W), bool)
    for dy in (0, 1, 2):
        for dx in (0, 1, 2):
            out |= p[dy:dy + H, dx:dx + W]
    return out


def _loop(samples, threshold, min_spp, step, max_spp, next_active):
    S, n_rays, _ = samples.shape
    assert S >= max_spp and step >= 2 and min_spp > 0 and min_spp % step == 0 and max_spp % step == 0 and min_spp <= max_spp
    active = np.ones(n_rays, bool)
    n = np.zeros(n_rays, np.uint32)
    rounds, ray_samples = 0, 0
    for r in range(max_spp // step):
        if not active.any():
            break
        n[active] += step
        rounds += 1
        ray_samples += int(active.sum()) * step
        if (r + 1) * step >= min_spp:
            S1, S2 = AR.fold(samples[:(r + 1) * step], n)
            active = next_active(active, active & ~AR.done(S1, S2, n, threshold))
    S1, S2 = AR.fold(samples[:max_spp], n)
    return dict(n=n, S1=S1, S2=S2, rounds=rounds, max_count=int(n.max()) if n_rays else 0, ray_samples=ray_samples,
                active=int(active.sum()))


def rays(samples, threshold, min_spp, step, max_spp):
    """The round loop of the ray query.  samples: [S >= max_spp][n][3] float32, sample s of ray i.  Returns dict(n [n] uint32,
    S1, S2 [n][3] float32, rounds, max_count, ray_samples, active)."""
    return _loop(np.asarray(samples, f32), threshold, min_spp, step, max_spp, lambda active, need: need)


def lightmap(samples, texel, W, H, threshold, min_spp, step, max_spp):
    """The round loop of the lightmap bake.  samples: [S][covered][3] of the covered texels, texel: their indices y * W + x.  A
    covered texel stays active when it is active and some active, not-done, covered texel lies in its 3x3 neighbourhood clipped to
    the map.  Returns the dict of rays(), per covered texel."""
    texel = np.asarray(texel)

    def next_active(active, need):
        plane = np.zeros(W * H, bool)
        plane[texel[need]] = True
        return active & dilate_in_map(plane.reshape(H, W)).reshape(-1)[texel]

    return _loop(np.asarray(samples, f32), threshold, min_spp, step, max_spp, next_active)


def oracle_samples(o, ro, rd, depth, seed, count, key_base=0, keys=None, mode=0):
    """[count][n][3] float32: sample s of ray i from Oracle.trace_counter on the stream of (seed, RNG pixel keys[i] - default
    (key_base + i) mod 2^32 -, s); mode 1: behind the two lens draws"""
    n = len(ro)
    out = np.zeros((count, n, 3), f32)
    for i in range(n):
        k = int(keys[i]) if keys is not None else (key_base + i) & 0xffffffff
        for s in range(count):
            out[s, i] = o.trace_counter(ro[i], rd[i], depth, seed, k, s, mode)
    return out


@functools.lru_cache(maxsize=None)
def case(name):
    """(arrays, ro, rd, samples [MAX_SPP][N][3]) of a scene at the recipe; computed once, shared, not to be modified"""
    from oracle import oracle_binding as OB
    OB.build()
    arrays, _ = RC.scene(name)
    ro, rd = RC.rays_in_box(arrays, N, RAY_SEED)
    o = OB.Oracle(arrays)
    s = oracle_samples(o, ro, rd, DEPTH, SEED, MAX_SPP)
    o.close()
    return arrays, ro, rd, s
