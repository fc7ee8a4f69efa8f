"""What the family of tests/plain_random_scenes.py has to be for tests/test_gpu_plain_random.py to mean something: conditions on the
scenes and on the oracle's images of them, not measurements.  Every row is a PLAIN scene of its Lambert flag; together they take every
zero class, every pair kind and every prefix length 0..8 of csrc/ptk_flat_mt.h; their images are lit; every arm of Trace that a PLAIN
kernel can reach is met FLOOR times by the family alone; and their 16 x 16 tiles run from empty to full.  No device."""
import numpy as np
import pytest

import plain_random_scenes as P
import trace_arms as TA


class _Family:
    def __init__(self, OB):
        from pbrpathtracer_amd import ptk
        self.scenes = [P.row_scene(r) for r in P.FAMILY]
        self.classes, self.prefixes = zip(*[P.classify(a) for a, _ in self.scenes])
        self.images = [P.oracle_image(OB, a, cam, r)[0] for (a, cam), r in zip(self.scenes, P.FAMILY)]
        self.ptk = ptk


@pytest.fixture(scope="module")
def fam(oracle_mod):
    return _Family(oracle_mod)


# ---- predicates and classes -------------------------------------------------------------------------------------------------------
def test_the_family_has_the_shape_the_gpu_test_relies_on():
    rows = P.FAMILY
    assert 45 <= len(rows) <= 55 and len(set(rows)) == len(rows)
    assert [r[1] for r in rows[:48]] == [1, 2, 3, 5, 8, 11, 12, 13, 14, 15, 16, 16] * 4
    assert {r[6] for r in rows} == set(range(1, 9))
    assert {r[7] for r in rows} == set(range(3, 12))
    assert all(33 <= r[4] <= 64 and 17 <= r[5] <= 48 for r in rows)
    assert 3 * sum(1 for r in rows if r[4] % 16 and r[5] % 16) >= len(rows)
    assert {r[2] for r in rows} == set(P.VARIANTS)
    assert any(r[3] for r in rows) and any(not r[3] for r in rows)


def test_the_generator_is_a_function_of_its_arguments():
    for row in (P.FAMILY[5], P.FAMILY[22]):
        a, cam = P.row_scene(row); b, cam_b = P.row_scene(row)
        assert all(np.array_equal(a[k], b[k]) for k in a) and all(np.array_equal(cam[k], cam_b[k]) for k in cam)
    for n in range(1, 17):
        for variant in P.VARIANTS:
            a, cam = P.plain_scene(7, n, variant, bool(n & 1))
            assert len(a["verts"]) == n and a["verts"].dtype == np.float32 and np.isfinite(a["verts"]).all(), (n, variant)
            assert cam["aperture"] == 0.0 and not a["smoothing"].any() and (a["materials"]["type"] == 0).all()


def test_every_row_is_plain_and_lambert_as_flagged(fam):
    for row, (a, _) in zip(P.FAMILY, fam.scenes):
        assert fam.ptk.scene_is_plain(a), row
        assert fam.ptk.scene_is_lambert(a) == row[3], row
        assert len(a["verts"]) == row[1]
        m, used = a["materials"], set(a["material"].tolist())
        assert len(m) == 5 and (m["diffuse"].max(axis=1) > 0.95).sum() == 1
        if not row[3] and len(used - {P.LIGHT}):             # (a scene of the light alone has no other material in use)
            assert any(m["reflectiveness"][k] > 0 and 0 < m["roughness"][k] < 1 for k in used), row


def test_all_sixteen_zero_classes_and_all_six_pair_kinds(fam):
    assert {c for cl in fam.classes for c in cl} == set(range(16))
    assert {k for pf in fam.prefixes for k in pf} == set(range(1, 7))


def test_prefix_lengths_are_zero_to_eight(fam):
    assert {len(pf) for pf in fam.prefixes} == set(range(9))


def test_single_records_stand_directly_behind_a_prefix(fam):
    """a record that is no half of a pair right behind a non-empty prefix: the pass changes form in the middle of the list"""
    count = 0
    for (a, _), pf in zip(fam.scenes, fam.prefixes):
        count += bool(pf) and 2 * len(pf) < len(a["verts"])
    assert count >= 5, count
    # and the directed row: an oblique record in front, nothing but rectangles behind it
    a, _ = P.row_scene(P.FAMILY[-1])
    assert P.classify(a)[1] == [] and P.classify(a)[0][0] == 0
    assert len(fam.ptk.flat_rect_prefix(a["verts"][1:])) == 6


def test_the_stress_variants_are_what_they_say():
    F = {r[2]: r for r in P.FAMILY if r[1] >= 11}
    snapped, _ = P.row_scene(F[1])
    assert np.array_equal(snapped["verts"] * 4, np.round(snapped["verts"] * 4))
    small, cam_s = P.row_scene(F[2]); big, cam_b = P.row_scene(F[3])
    assert np.abs(small["verts"]).max() < 0.3 and np.abs(big["verts"]).max() > 3000 and abs(cam_s["pos"][2]) < 0.12 and cam_b["pos"][2] > 2500
    twins, _ = P.row_scene(F[4])
    assert np.array_equal(twins["verts"][-2:].view(np.uint32), twins["verts"][:2].view(np.uint32))
    assert (twins["material"][-2:] != twins["material"][:2]).all() and not set(twins["lights"].tolist()) & {len(twins["verts"]) - 1, len(twins["verts"]) - 2}
    zeros, _ = P.row_scene(F[5])
    v = zeros["verts"].reshape(-1, 3, 3)
    e = np.concatenate([v[:, 1] - v[:, 0], v[:, 2] - v[:, 0]], axis=1)
    assert ((e == 0) & np.signbit(e)).any() and ((e == 0) & ~np.signbit(e)).any()
    dark, _ = P.row_scene(F[6])
    assert len(dark["lights"]) == 0
    level, cam = P.row_scene(F[7])
    assert np.array_equal(cam["dir"], np.float32([0, 0, -1]))
    v = level["verts"].reshape(-1, 3, 3)
    assert any((v[k, :, p] == cam["pos"][p]).all() for k in range(len(v)) for p in (0, 1))
    band, _ = P.row_scene(F[8])
    thr = np.float32(1.0) - np.float32(0.00001)
    assert abs(band["tbn"][-2, 0]) == np.nextafter(thr, np.float32(0)) and abs(band["tbn"][-1, 0]) == thr


def test_cameras_in_a_plane_send_rays_that_lie_in_it(oracle_mod):
    """variant 7: in at least two rows a whole line of primary rays has an exact zero on the axis of a record's plane through the
    camera - Moeller-Trumbore's determinant against that record is an exact zero"""
    rows = 0
    for row in P.FAMILY:
        if row[2] != 7:
            continue
        a, cam = P.row_scene(row)
        o = oracle_mod.Oracle(a)
        d = o.primary_dirs(oracle_mod.make_camera(**cam), row[4], row[5])
        o.close()
        v = a["verts"].reshape(-1, 3, 3)
        rows += any((v[k, :, p] == cam["pos"][p]).all() and (d[..., p] == 0).sum() >= row[4] for k in range(len(v)) for p in (0, 1))
    assert rows >= 2, rows


# ---- oracle images ------------------------------------------------------------------------------------------------------------------
def test_every_image_is_finite_and_lit(fam):
    """no row is excused: a scene with its light list emptied (variant 6) still shows its emitter to the camera, at depth 1 too"""
    for row, img in zip(P.FAMILY, fam.images):
        assert np.isfinite(img).all(), row
        assert (img != 0).any(), row
        if row[1] >= 11 and row[2] not in (6, 7):
            assert (img != 0).any(axis=2).mean() >= 0.4, (row, float((img != 0).any(axis=2).mean()))


# ---- arm census -----------------------------------------------------------------------------------------------------------------------
def test_every_plain_reachable_arm_is_met_by_the_family_alone(oracle_mod, fam):
    scenes = [("row%d" % k, a, cam, r[4], r[5], r[6], r[7], r[0], ("PLAIN",)) for k, ((a, cam), r) in enumerate(zip(fam.scenes, P.FAMILY))]
    total, _ = TA.census(oracle_mod, scenes=scenes)
    names = list(total["PLAIN"])
    un = TA.unreachable("PLAIN", names)
    short = [(n, total["PLAIN"][n]) for n in names if n not in un and total["PLAIN"][n] < TA.FLOOR]
    assert not short, short
    assert all(total["PLAIN"][n] == 0 for n in un), [n for n in un if total["PLAIN"][n]]
    assert len(names) - len(un) >= 30


# ---- live-pixel spread ----------------------------------------------------------------------------------------------------------------
def test_tiles_run_from_empty_to_full(oracle_mod, fam):
    """live pixels per 16 x 16 tile = pixels whose camera ray of sample 0 hits a triangle (the primary hits of the oracle's counted
    render): what the cycle unit's deal has to spread over its lanes"""
    empty = few = full = 0
    for (a, cam), row in zip(fam.scenes, P.FAMILY):
        seed, _, _, _, W, H, _, _ = row
        o = oracle_mod.Oracle(a)
        r = o.render_counted(oracle_mod.make_camera(**cam), W, H, 1, 0, 1, seed, dump=True)["rays"]
        o.close()
        r = r[r["kind"] == oracle_mod.RAY_CAMERA]
        assert len(r) == W * H
        live = np.zeros(W * H, bool); live[r["pixel"]] = r["tri"] >= 0
        live = live.reshape(H, W)
        for ty in range(0, H, 16):
            for tx in range(0, W, 16):
                t = live[ty:ty + 16, tx:tx + 16]
                c = int(t.sum())
                empty += c == 0; few += 1 <= c <= 15; full += t.size == 256 and c == 256
    assert empty >= 10 and few >= 10 and full >= 10, (empty, few, full)


# ---- geometry updates ------------------------------------------------------------------------------------------------------------------
def test_update_pairs_change_the_prefix_both_ways(fam):
    assert len(P.UPDATE_PAIRS) == 6
    change = []
    for ia, ib in P.UPDATE_PAIRS:
        a, _, first, v, nn, tb, m = P.mixed_scene(ia, ib)
        n = len(a["verts"])
        assert 0 < len(v) < n and first + len(v) <= n and fam.ptk.scene_is_plain(m)
        assert not np.array_equal(m["verts"], a["verts"]) and np.array_equal(m["material"], a["material"])
        change.append(len(P.classify(m)[1]) - len(P.classify(a)[1]))
    assert change[0] > 0 and change[1] < 0, change


# ---- what the GPU file renders ---------------------------------------------------------------------------------------------------------
def test_the_gpu_file_leaves_out_no_row_and_no_option_set():
    import test_gpu_plain_random as G
    assert sorted(k for g in G.GROUPS for k in g) == list(range(len(P.FAMILY)))
    assert [o[0] for o in P.OPTION_SETS] == ["flat_cycle", "flat_rect_pairs", "flat_zero_classes", "lambert_kernel", "plain_kernel", "flat"]
    assert len(G.SPLIT_ROWS) * 4 >= len(P.FAMILY) and len(set(G.CONTRACT_ROWS)) == 6
    assert all(P.FAMILY[k][1] >= 11 for k in G.CONTRACT_ROWS) and {P.FAMILY[k][3] for k in G.CONTRACT_ROWS} == {True, False}
