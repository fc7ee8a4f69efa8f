"""Helper of tests/test_surface_sample_cpu.py and tests/test_gpu_surface_sample.py (include/ptk.h ptk_sample_surface): a numpy
restatement of the surface-sampling rule - no tests of its own.

Weights in float32 operation by operation, the quantised table in Python-exact integers (uint64 throughout), the draws in uint32
arithmetic as tests/hit_rule.py states them, the high half of the 64 x 64 bit product from 32-bit limbs."""
import math

import numpy as np

import hit_rule as HR

F32 = np.float32
U32 = np.uint32
U64 = np.uint64
LCG = U32(747796405)


def areas(verts, weights=None):
    """a_i [N] float32 of the rule: 0.5 * |cross(v2 - v1, v3 - v1)|, times w_i where weights are given"""
    v = np.ascontiguousarray(verts, F32).reshape(-1, 9)
    e1 = [v[:, 3 + k] - v[:, k] for k in range(3)]
    e2 = [v[:, 6 + k] - v[:, k] for k in range(3)]
    cx = e1[1] * e2[2] - e2[1] * e1[2]
    cy = e1[2] * e2[0] - e2[2] * e1[0]
    cz = e1[0] * e2[1] - e2[0] * e1[1]
    with np.errstate(over="ignore", invalid="ignore"):
        a = F32(0.5) * np.sqrt((cx * cx + cy * cy) + cz * cz)
        if weights is not None:
            a = a * np.ascontiguousarray(weights, F32).reshape(-1)
    assert a.dtype == F32
    return a


def quantise(a):
    """(q [N] uint64, E) for weights a [N] float32: q_i = trunc(a_i * 2^(35 - E)), E = floor(log2 max a).  ValueError where nothing
    can be sampled or a weight is not finite."""
    a = np.asarray(a, F32)
    if not np.isfinite(a).all():
        raise ValueError("a weight is not finite")
    m = float(a.max()) if len(a) else 0.0
    if not m > 0.0:
        raise ValueError("nothing to sample")
    E = math.frexp(m)[1] - 1
    q = np.trunc(np.ldexp(np.abs(a).astype(np.float64), 35 - E))
    assert q.max() < 2.0 ** 36 and q.max() >= 2.0 ** 35
    return q.astype(U64), E


def table(verts, weights=None):
    """(incl [N] uint64, E, m): the inclusive sums of the quantised weights, the exponent and the largest weight"""
    a = areas(verts, weights)
    q, E = quantise(a)
    incl = np.cumsum(q, dtype=U64)
    assert int(incl[-1]) == sum(int(x) for x in q) < 1 << 63
    return incl, E, F32(np.abs(a).max())


def info(verts, weights=None):
    """(total, E, drawable, max_weight) as ptk_surface_info reports them"""
    a = areas(verts, weights)
    q, E = quantise(a)
    return sum(int(x) for x in q), E, int((q > 0).sum()), F32(np.abs(a).max())


def mulhi64(a, b):
    """floor(a * b / 2^64) for uint64 arrays, from 32-bit limbs"""
    a = np.asarray(a, U64); b = np.asarray(b, U64)
    M = U64(0xffffffff); S = U64(32)
    al, ah, bl, bh = a & M, a >> S, b & M, b >> S
    ll, lh, hl, hh = al * bl, al * bh, ah * bl, ah * bh
    mid = (ll >> S) + (lh & M) + (hl & M)
    return hh + (lh >> S) + (hl >> S) + (mid >> S)


def raw_draws(seed, key_base, n, sample, count=4):
    """[count][n] uint32: the first raw outputs of the streams (seed, RNG pixel key_base + j, sample), j < n"""
    pix = (U64(int(key_base) & 0xffffffff) + np.arange(n, dtype=U64)) & U64(0xffffffff)
    pkey = HR.pixel_key(seed, pix)
    with np.errstate(over="ignore"):
        inc = (HR.hash32(pkey ^ U32(0x9E3779B9)) << U32(1)) | U32(1)
        state = HR.hash32(U32(int(sample) & 0xffffffff) + pkey)
        out = []
        for _ in range(count):
            out.append(HR.pcg_out(state))
            state = state * LCG + inc
    return out


def pick(incl, seed, key_base, n, sample):
    """(tri [n] int32, r2, r3 [n] uint32): the triangle of every sample and the two draws left for the point"""
    r0, r1, r2, r3 = raw_draws(seed, key_base, n, sample)
    r64 = (r0.astype(U64) << U64(32)) | r1.astype(U64)
    target = mulhi64(r64, np.full(n, incl[-1], U64))
    assert (target < incl[-1]).all()
    tri = np.searchsorted(incl, target, side="right").astype(np.int32)      # the smallest i with incl[i] > target
    return tri, r2, r3


def sample(arrays_or_verts, n, seed=0, key_base=0, sample=0, weights=None, normals=None, material=None):
    """(tri [n] int32, bary [n, 2], position [n, 3], normal [n, 3] float32, material [n] int32) of the rule.  The first argument is
    a scene's arrays (verts, tbn, material are read) or a bare [N, 9] vertex array with `normals` [N, 3] and `material` [N]."""
    if isinstance(arrays_or_verts, dict):
        verts = arrays_or_verts["verts"]
        normals = np.ascontiguousarray(arrays_or_verts["tbn"], F32).reshape(-1, 9)[:, :3]
        material = np.asarray(arrays_or_verts["material"], np.int32)
    else:
        verts = arrays_or_verts
    v = np.ascontiguousarray(verts, F32).reshape(-1, 3, 3)
    incl = table(verts, weights)[0]
    tri, r2, r3 = pick(incl, seed, key_base, n, sample)
    su = np.sqrt(HR.u01(r2)); sv = HR.u01(r3)
    assert su.dtype == F32 and sv.dtype == F32
    w0 = F32(1.0) - su; w1 = su * (F32(1.0) - sv); w2 = su * sv
    t = v[tri]
    pos = (t[:, 0] * w0[:, None] + t[:, 1] * w1[:, None]) + t[:, 2] * w2[:, None]
    assert pos.dtype == F32
    nrm = np.zeros((n, 3), F32) if normals is None else np.ascontiguousarray(normals, F32).reshape(-1, 3)[tri]
    mat = np.zeros(n, np.int32) if material is None else np.asarray(material, np.int32)[tri]
    return tri, np.stack([w1, w2], axis=1), pos, nrm, mat


def edge_table_scene():
    """(verts [5, 9], factors): right triangles in the plane z = 0 whose areas are exactly 1, 2^-20, 2^-35, 2^-36, 2^-37 times the
    largest (legs 1 x 2^k): q = 2^35, 2^15, 1, 0, 0 - the factor 2^-35 is the smallest that can be drawn"""
    ks = [0, -20, -35, -36, -37]
    v = np.zeros((len(ks), 9), F32)
    for i, k in enumerate(ks):
        x = F32(2.0 * i)
        v[i] = [x, 0, 0, x + F32(1.0), 0, 0, x, F32(2.0 ** k), 0]
    return v, [2.0 ** k for k in ks]


def stretched_torus():
    """crossings_rule.mesh("torus") with x scaled by 5 and z by 0.2 in float32: 256 triangles, area ratio about 5"""
    import crossings_rule as XR
    v = XR.mesh("torus").reshape(-1, 3, 3).copy()
    v[:, :, 0] = v[:, :, 0] * F32(5.0)
    v[:, :, 2] = v[:, :, 2] * F32(0.2)
    assert v.dtype == F32
    return v.reshape(-1, 9)
