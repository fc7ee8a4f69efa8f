"""Helper of tests/test_hits_cpu.py and tests/test_gpu_hits.py (include/ptk.h ptk_intersect_rays, ptk_occluded_rays): a numpy
restatement of the candidate rule - no tests of its own.

Keys in uint32 arithmetic as oracle/pt_oracle.c computes them (hash32, u01, pixel_key, the key of a ray's sample).  Per ray,
oracle_binding.intersect_many - the kernels' Moeller-Trumbore, bit for bit - against EVERY triangle; t > 0 (and < inf) means
accepted by it.  The candidates are taken in ascending (t, index); an opacity-mapped one passes when
    u01(hash32(k + hash32(0 + key))) < Oracle.tex2d(opacity map, uv(u, v))[0]
with w = (1 - u) - v, ux = (w * uv0 + u * uv2) + v * uv4, uy likewise, every operation rounded to float32 (get_uv).  The first
candidate to pass is the hit: the closest accepted triangle, ties to the smaller index, found without a tree."""
import numpy as np

F32 = np.float32
U32 = np.uint32
OPACITY_SLOT = 5            # materials[].tex[5]: the opacity map (pt_oracle.c test_triangle)


def _u32(x):
    return np.asarray(x, np.uint64).astype(U32) if not (isinstance(x, np.ndarray) and x.dtype == U32) else x


def pcg_out(st):
    st = _u32(st)
    with np.errstate(over="ignore"):
        w = ((st >> ((st >> U32(28)) + U32(4))) ^ st) * U32(277803737)
    return (w >> U32(22)) ^ w


def hash32(x):
    x = np.atleast_1d(_u32(x))
    with np.errstate(over="ignore"):
        return pcg_out(x * U32(747796405) + U32(2891336453))


def u01(x):
    return (np.atleast_1d(_u32(x)) >> U32(8)).astype(F32) * F32(5.9604644775390625e-8)


def pixel_key(seed, pixel):
    """pt_oracle.c pixel_key: the 64-bit seed and the RNG pixel (mod 2^32) -> uint32 [n]"""
    seed = int(seed) & 0xffffffffffffffff
    a = hash32(seed >> 32)
    with np.errstate(over="ignore"):
        b = hash32(U32(seed & 0xffffffff) + a)
        return hash32(np.atleast_1d(_u32(np.asarray(pixel, np.uint64) & np.uint64(0xffffffff))) + b)


def ray_keys(seed, key_base, n, sample):
    """key_i = hash32(sample + pixel_key(seed, (key_base + i) mod 2^32)), i < n: the Rng::key ptk_trace_rays gives sample `sample` of
    ray i"""
    pix = (np.uint64(int(key_base) & 0xffffffff) + np.arange(n, dtype=np.uint64)) & np.uint64(0xffffffff)
    with np.errstate(over="ignore"):
        return hash32(U32(int(sample) & 0xffffffff) + pixel_key(seed, pix))


PROBE_KEY = hash32(0)[0]    # the key of Oracle.hit (rng_init(0, 0)): with it the mirror is orc_hit_brute


def mirror(oracle_mod, arrays, ro, rd, keys, oracle=None, chunk=64):
    """(tri [n] int32, -1 = miss; t [n] float32, inf = miss; bary [n, 2] float32, 0 = miss; material [n] int32, -1 = miss) of the
    rays under the candidate rule with per-ray keys `keys` (uint32 [n], or one key for all)."""
    a = oracle_mod.normalise_arrays(arrays)
    ro = np.ascontiguousarray(ro, F32).reshape(-1, 3); rd = np.ascontiguousarray(rd, F32).reshape(-1, 3)
    n, nt = len(ro), len(a["verts"])
    keys = np.broadcast_to(np.atleast_1d(_u32(keys)), (n,)) if np.size(keys) == 1 else _u32(keys)
    tri = np.full(n, -1, np.int32); t = np.full(n, np.inf, F32); bary = np.zeros((n, 2), F32); mat = np.full(n, -1, np.int32)
    if nt == 0:
        return tri, t, bary, mat
    otex = a["materials"]["tex"][a["material"], OPACITY_SLOT] if len(a["materials"]) else np.full(nt, -1, np.int32)
    o = oracle
    if (otex >= 0).any() and o is None:
        o = oracle_mod.Oracle(arrays)
    for c0 in range(0, n, chunk):
        c1 = min(n, c0 + chunk); m = c1 - c0
        tuv = oracle_mod.intersect_many(np.repeat(ro[c0:c1], nt, axis=0), np.repeat(rd[c0:c1], nt, axis=0),
                                        np.tile(a["verts"], (m, 1))).reshape(m, nt, 3)
        for j in range(m):
            i = c0 + j
            tj = tuv[j, :, 0]
            cand = np.nonzero((tj > 0) & (tj < np.inf))[0]
            cand = cand[np.argsort(tj[cand], kind="stable")]            # ascending (t, index): cand is ascending in index already
            for k in cand:
                u, v = tuv[j, k, 1], tuv[j, k, 2]
                if otex[k] >= 0:
                    uv = a["uvs"][k]
                    w = F32(F32(1.0) - u) - v
                    ux = F32(F32(w * uv[0]) + F32(u * uv[2])) + F32(v * uv[4])
                    uy = F32(F32(w * uv[1]) + F32(u * uv[3])) + F32(v * uv[5])
                    op = o.tex2d(int(otex[k]), float(ux), float(uy))[0]
                    with np.errstate(over="ignore"):
                        draw = u01(hash32(U32(k) + hash32(U32(0) + keys[i])))[0]
                    if not draw < op:
                        continue
                tri[i] = k; t[i] = tj[k]; bary[i] = (u, v); mat[i] = a["material"][k]
                break
    if o is not None and oracle is None:
        o.close()
    return tri, t, bary, mat


def occluded(t_hit, tmax=None):
    """uint8 [n]: the closest accepted t lies STRICTLY below tmax (None: +inf); a NaN, zero or negative tmax gives 0"""
    t_hit = np.asarray(t_hit, F32)
    if tmax is None:
        return (t_hit < np.inf).astype(np.uint8)
    with np.errstate(invalid="ignore"):
        return (t_hit < np.asarray(tmax, F32)).astype(np.uint8)
