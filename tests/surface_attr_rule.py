"""Expected surface attributes (include/ptk.h ptk_surface_attributes) - a helper, no tests of its own.

A float32 numpy restatement of the rule for arrays (tri, u, v, dirs or None) over oracle_mod.normalise_arrays(arrays): one numpy
operation per C operation, every intermediate a float32 array, texels through Oracle.tex2d.  The order of the operations is that
of tests/feature_truth.py:77-122 (oracle/pt_oracle.c shade() and get_uv()); what this file adds is the query form - any (triangle,
bary) pair, misses, no direction, the texture coordinate, the position and the opacity texel as outputs - and a report of which
arm each query took."""
import numpy as np

F32 = np.float32
NAMES = ("material", "uv", "position", "normal_geom", "normal", "albedo", "emission", "gloss", "opacity")
CHANNELS = (1, 2, 3, 3, 3, 3, 3, 2, 1)
IS_INT = (True, False, False, False, False, False, False, False, False)
SLOTS = ("diffuse", "normal", "emissive", "roughness", "reflectiveness", "opacity")     # materials[].tex[0..5]
EPS = F32(0.00001)           # ORC_EPS (mesh.h:12)


def _dot(a, b):         # pt_oracle.c:29
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(a):      # pt_oracle.c:37-42
    sqr = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    inv = F32(1.0) / np.sqrt(sqr)
    return a * inv[:, None]


def restate(oracle_mod, arrays, tri, u, v, dirs=None, oracle=None):
    """(out, arms): out maps each of NAMES to its [n] or [n, c] array; arms maps 'hit', 'smooth_only', 'map_only', 'both',
    'neither', 'flip', 'no_flip' and 'bound_<slot>' / 'unbound_<slot>' for the six texture slots to [n] bool arrays - which arm of
    the rule each query took (all False for a miss)."""
    a = oracle_mod.normalise_arrays(arrays)
    o = oracle if oracle is not None else oracle_mod.Oracle(arrays)
    tri_all = np.ascontiguousarray(tri, np.int32).reshape(-1)
    n = len(tri_all)
    u_all = np.ascontiguousarray(u, F32).reshape(-1); v_all = np.ascontiguousarray(v, F32).reshape(-1)
    d_all = None if dirs is None else np.ascontiguousarray(dirs, F32).reshape(n, 3)
    out = {nm: np.zeros((n, c) if c > 1 else n, np.int32 if i else F32) for nm, c, i in zip(NAMES, CHANNELS, IS_INT)}
    out["material"][:] = -1
    arms = {k: np.zeros(n, bool) for k in ("hit", "smooth_only", "map_only", "both", "neither", "flip", "no_flip")}
    for s in SLOTS:
        arms["bound_" + s] = np.zeros(n, bool); arms["unbound_" + s] = np.zeros(n, bool)
    hit = np.nonzero((tri_all >= 0) & (tri_all < len(a["verts"])))[0]
    if len(hit):
        with np.errstate(all="ignore"):
            tri = tri_all[hit]; u = u_all[hit]; v = v_all[hit]
            matid = a["material"][tri]
            mat = a["materials"][matid]
            tex = mat["tex"]
            w = (F32(1.0) - u) - v                                           # get_uv :216
            uv = a["uvs"][tri]
            uvx = (w * uv[:, 0] + u * uv[:, 2]) + v * uv[:, 4]               # :217
            uvy = (w * uv[:, 1] + u * uv[:, 3]) + v * uv[:, 5]               # :218
            vt = a["verts"][tri]
            pos = (vt[:, 0:3] * w[:, None] + vt[:, 3:6] * u[:, None]) + vt[:, 6:9] * v[:, None]

            def texels(slot):
                """[k, 4] texels of texture slot `slot` for the queries whose material binds one, and their indices"""
                idx = np.nonzero(tex[:, slot] >= 0)[0]
                c = np.zeros((len(idx), 4), F32)
                for j, i in enumerate(idx):
                    c[j] = o.tex2d(int(tex[i, slot]), float(uvx[i]), float(uvy[i]))
                return idx, c

            tb = a["tbn"][tri]
            ng = tb[:, 0:3].copy()                                           # :511-512
            nrm = ng.copy()
            sm = np.nonzero(a["smoothing"][tri] != 0)[0]                     # :513
            if len(sm):
                nn = a["normals"][tri[sm]]
                ws = (F32(1.0) - u[sm]) - v[sm]                              # :516
                sn = (nn[:, 0:3] * ws[:, None] + nn[:, 3:6] * u[sm][:, None]) + nn[:, 6:9] * v[sm][:, None]   # :517
                nrm[sm] = _normalize(sn)                                     # :518
            nm_idx, c = texels(1)                                            # :520-523
            if len(nm_idx):
                nt = c[:, 0:3] * F32(2.0) - F32(1.0)                         # :524
                nt[nt[:, 2] <= 0.0, 2] = EPS                                 # :525
                nt = _normalize(nt)                                          # :526
                tg, bt, n0 = tb[nm_idx, 3:6], tb[nm_idx, 6:9], nrm[nm_idx]   # :527
                m = (tg * nt[:, 0:1] + bt * nt[:, 1:2]) + n0 * nt[:, 2:3]    # :528-530
                nrm[nm_idx] = _normalize(m)                                  # :531
            flip = np.zeros(len(hit), bool)
            if d_all is not None:
                flip = _dot(nrm, d_all[hit]) > 0.0                           # :533 (a NaN does not flip)
                nrm[flip] = -nrm[flip]
            diffuse = mat["diffuse"].astype(F32).copy()                      # :538
            i, c = texels(0); diffuse[i] = c[:, 0:3]                         # :540
            emiss = mat["emissive"].astype(F32).copy()                       # :541
            i, c = texels(2); emiss[i] = c[:, 0:3]                           # :542
            rough = mat["roughness"].astype(F32).copy()                      # :543
            i, c = texels(3); rough[i] = c[:, 0]                             # :544
            refl = mat["reflectiveness"].astype(F32).copy()                  # :545
            i, c = texels(4); refl[i] = c[:, 0]                              # :546
            emission = emiss * mat["emissive_intensity"].astype(F32)[:, None]   # :629
            opacity = np.ones(len(hit), F32)
            i, c = texels(5); opacity[i] = c[:, 0]                           # :480-483, the value the draw is compared with
        out["material"][hit] = matid; out["uv"][hit] = np.stack([uvx, uvy], axis=1); out["position"][hit] = pos
        out["normal_geom"][hit] = ng; out["normal"][hit] = nrm; out["albedo"][hit] = diffuse; out["emission"][hit] = emission
        out["gloss"][hit] = np.stack([rough, refl], axis=1); out["opacity"][hit] = opacity
        is_sm = np.zeros(len(hit), bool); is_sm[sm] = True
        is_nm = np.zeros(len(hit), bool); is_nm[nm_idx] = True
        arms["hit"][hit] = True
        arms["smooth_only"][hit] = is_sm & ~is_nm; arms["map_only"][hit] = is_nm & ~is_sm
        arms["both"][hit] = is_sm & is_nm; arms["neither"][hit] = ~is_sm & ~is_nm
        arms["flip"][hit] = flip; arms["no_flip"][hit] = ~flip
        for k, s in enumerate(SLOTS):
            arms["bound_" + s][hit] = tex[:, k] >= 0; arms["unbound_" + s][hit] = tex[:, k] < 0
    if oracle is None:
        o.close()
    return out, arms


def equal(got, want):
    """array_equal with NaN == NaN, shapes and types equal too"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
