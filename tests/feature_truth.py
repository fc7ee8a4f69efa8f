"""Expected first-hit feature planes (include/ptk.h ptk_render_features) from the CPU oracle - a helper, no tests of its own.

Hits: the oracle's own camera-ray records (orc_render_counted with a CLOSED lens, kind ORC_RAY_CAMERA) give, per pixel and
sample, the ray and its closest accepted hit, stochastic opacity included; u, v come from the oracle's Moeller-Trumbore on that
(ray, triangle) pair.  Shading planes: a float32 numpy restatement of oracle/pt_oracle.c shade() lines 507-546 and get_uv()
(:213-219) - one numpy operation per C operation, every intermediate a float32 array, texels through Oracle.tex2d."""
import numpy as np

F32 = np.float32
NAMES = ("depth", "triangle", "material", "bary", "position", "normal_geom", "normal", "albedo", "emission", "gloss")
CHANNELS = (1, 1, 1, 2, 3, 3, 3, 3, 3, 2)
IS_INT = (False, True, True, False, False, False, False, False, False, False)
EPS = F32(0.00001)           # ORC_EPS (mesh.h:12)


def owned_mask(W, H, rank, world):
    """[H, W] top-down: the pixels of the 16x16 tiles rank `rank` of `world` owns (include/ptk.h ptk_set_tile)."""
    tiles_x, tiles_y = (W + 15) // 16, (H + 15) // 16
    m = np.zeros((H, W), bool)
    for ty in range(tiles_y):
        for tx in range(tiles_x):
            if (ty * tiles_x + (tx + 3 * ty) % tiles_x) % world == rank:
                m[ty * 16:(ty + 1) * 16, tx * 16:(tx + 1) * 16] = True
    return m


def camera_records(oracle_mod, arrays, cam, W, H, seed, sample, rank=0, world=1, oracle=None):
    """The camera ray of every owned pixel for (seed, sample) with the lens closed: dict of per-pixel arrays (top-down pixel
    index) seen [N] bool, tri [N] (-1 = miss), t [N] (+inf = miss), ro, rd [N, 3]."""
    o = oracle if oracle is not None else oracle_mod.Oracle(arrays)
    ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], 0.0)
    rays = o.render_counted(ocam, W, H, 1, sample, 1, seed, rank=rank, world=world, dump=True)["rays"]   # (trace depth: any)
    if oracle is None:
        o.close()
    r = rays[rays["kind"] == oracle_mod.RAY_CAMERA]
    n = W * H
    per_px = np.bincount(r["pixel"], minlength=n)
    own = owned_mask(W, H, rank, world).reshape(-1)
    assert np.array_equal(per_px, own.astype(per_px.dtype)), "expected exactly one camera record per owned pixel"
    assert (r["sample"] == sample).all() and (r["ray"] == 0).all()
    tri = np.full(n, -1, np.int32); t = np.full(n, np.inf, F32)
    ro = np.zeros((n, 3), F32); rd = np.zeros((n, 3), F32)
    tri[r["pixel"]] = r["tri"]; t[r["pixel"]] = r["t"]; ro[r["pixel"]] = r["ro"]; rd[r["pixel"]] = r["rd"]
    return dict(seen=own, tri=tri, t=t, ro=ro, rd=rd)


def _dot(a, b):         # pt_oracle.c:29
    return (a[:, 0] * b[:, 0] + a[:, 1] * b[:, 1]) + a[:, 2] * b[:, 2]


def _normalize(a):      # pt_oracle.c:37-42
    sqr = (a[:, 0] * a[:, 0] + a[:, 1] * a[:, 1]) + a[:, 2] * a[:, 2]
    inv = F32(1.0) / np.sqrt(sqr)
    return a * inv[:, None]


def truth(oracle_mod, arrays, cam, W, H, seed, sample, rank=0, world=1):
    """dict name -> plane ([H, W] or [H, W, c], rows BOTTOM-UP) of what ptk_render_features must give, plus 'branches': how many
    pixels took each branch of the normal code (smooth, normal_map, both, flip) and 'owned' [H, W] bottom-up."""
    a = oracle_mod.normalise_arrays(arrays)
    o = oracle_mod.Oracle(arrays)
    rec = camera_records(oracle_mod, arrays, cam, W, H, seed, sample, rank, world, oracle=o)
    n = W * H
    out = {nm: np.zeros((n, c) if c > 1 else n, np.int32 if i else F32) for nm, c, i in zip(NAMES, CHANNELS, IS_INT)}
    out["depth"][:] = np.inf; out["triangle"][:] = -1; out["material"][:] = -1
    hit = np.nonzero(rec["tri"] >= 0)[0]
    branches = dict(smooth=0, normal_map=0, both=0, flip=0)
    if len(hit):
        with np.errstate(all="ignore"):
            tri = rec["tri"][hit]; t = rec["t"][hit]; ro = rec["ro"][hit]; rd = rec["rd"][hit]
            tuv = oracle_mod.intersect_many(ro, rd, a["verts"][tri])
            assert np.array_equal(tuv[:, 0], t), "the oracle's record and its Moeller-Trumbore disagree on t"
            u, v = tuv[:, 1], tuv[:, 2]
            matid = a["material"][tri]
            mat = a["materials"][matid]
            tex = mat["tex"]
            p = ro + rd * t[:, None]                                         # :508
            uv = a["uvs"][tri]
            w = (F32(1.0) - u) - v                                           # get_uv :216
            uvx = (w * uv[:, 0] + u * uv[:, 2]) + v * uv[:, 4]               # :217
            uvy = (w * uv[:, 1] + u * uv[:, 3]) + v * uv[:, 5]               # :218

            def texels(slot):
                """[k, 4] texels of texture slot `slot` for the hits whose material binds one, and their indices"""
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
            flip = _dot(nrm, rd) > 0.0                                       # :533
            nrm[flip] = -nrm[flip]
            is_sm = np.zeros(len(hit), bool); is_sm[sm] = True
            is_nm = np.zeros(len(hit), bool); is_nm[nm_idx] = True
            branches = dict(smooth=int((is_sm & ~is_nm).sum()), normal_map=int((is_nm & ~is_sm).sum()),
                            both=int((is_sm & is_nm).sum()), flip=int(flip.sum()))
            diffuse = mat["diffuse"].astype(F32).copy()                      # :538
            i, c = texels(0); diffuse[i] = c[:, 0:3]                         # :540
            emiss = mat["emissive"].astype(F32).copy()                       # :541
            i, c = texels(2); emiss[i] = c[:, 0:3]                           # :542
            rough = mat["roughness"].astype(F32).copy()                      # :543
            i, c = texels(3); rough[i] = c[:, 0]                             # :544
            refl = mat["reflectiveness"].astype(F32).copy()                  # :545
            i, c = texels(4); refl[i] = c[:, 0]                              # :546
            emission = emiss * mat["emissive_intensity"].astype(F32)[:, None]   # :629
        out["depth"][hit] = t; out["triangle"][hit] = tri; out["material"][hit] = matid
        out["bary"][hit] = np.stack([u, v], axis=1); out["position"][hit] = p
        out["normal_geom"][hit] = ng; out["normal"][hit] = nrm; out["albedo"][hit] = diffuse
        out["emission"][hit] = emission; out["gloss"][hit] = np.stack([rough, refl], axis=1)
    o.close()
    planes = {}
    for nm, c in zip(NAMES, CHANNELS):
        planes[nm] = np.ascontiguousarray(out[nm].reshape((H, W, c) if c > 1 else (H, W))[::-1])
    planes["branches"] = branches
    planes["owned"] = np.ascontiguousarray(rec["seen"].reshape(H, W)[::-1])
    return planes


def planes_equal(got, want):
    """array_equal with NaN == NaN (a degenerate normal makes one on both sides), bit patterns otherwise equal as values"""
    return got.shape == want.shape and got.dtype == want.dtype and np.array_equal(got, want, equal_nan=got.dtype.kind == "f")
