"""The exact PLAIN pass's class switch as a branch tree (csrc/ptk_kernels_plain.hip, built with
-mllvm -structurizecfg-skip-uniform-regions=1; DESIGN 4.1 "The pass"): what a changed branch lowering could break.

The two exact PLAIN kernels (LAMBERT level and generic level) keep the uniform 16-way switch of the pass unstructured, with the
exec-masked hit updates inside it and `if (st == ST_TRAV)` around it.  A wrong exit of a body, a body entered for the wrong class
or an exec mask not given back would change samples, so every comparison is np.array_equal on the float accumulator: the kernel
against the generic FLAT kernel ("plain_kernel" 0: the full test, no switch, the common command line) and against itself with
"flat_zero_classes" 0 (every record through the switch to the general body).  The lists put every class first and last, alternate
between the two ends of the tree, have 1, 2, 15 and 16 records, and are built from the constructors of tests/flat_zero_scenes.py:
the box, its triangles with their vertices rolled (classes 4-15), turned in their plane (1-3) or skewed (0).

Frames of 64 x 48, 4 spp, depths 0, 1 and 8; the mirror variant of each list runs the generic level."""
import numpy as np
import pytest

import flat_zero_scenes as Z

pytestmark = pytest.mark.gpu

W, H, SPP, SEED = 64, 48, 4, 41
DEPTHS = (0, 1, 8)


def _cls(arrays):
    from pbrpathtracer_amd import ptk
    return [ptk.flat_zero_class(t[0], t[1], t[2]) for t in np.asarray(arrays["verts"], np.float32).reshape(-1, 3, 3)]


class _Pool:
    """the sixteen-triangle box and, per triangle, the rows that give it each class it can have"""
    def __init__(self):
        a, self.cam = Z.cornell()
        self.base = Z.sixteen(a)
        n = len(self.base["verts"])
        self.rows = [dict() for _ in range(n)]          # triangle -> class -> {key: row}
        keys = ("verts", "normals", "tbn")
        variants = [Z.rolled(self.base, j) for j in range(6)] + [Z.turned_in_plane(self.base), Z.skewed(self.base)]
        for v in variants:
            for k, c in enumerate(_cls(v)):
                self.rows[k].setdefault(c, {key: v[key][k].copy() for key in keys})
        self.lights = [int(l) for l in self.base["lights"]]

    def scene(self, order, classes):
        """the triangles `order` of the box, in that order, triangle order[i] in its variant of class classes[i]"""
        b = dict(self.base)
        for key in ("verts", "normals", "tbn"): b[key] = self.base[key].copy()
        for k, c in zip(order, classes):
            for key, row in self.rows[k][c].items(): b[key][k] = row
        s = Z.subset(b, order)
        assert _cls(s) == list(classes), (_cls(s), classes)
        assert len(s["lights"]) > 0
        return s

    def can(self, k, c): return c in self.rows[k]

    def with_first(self, c, last=False):
        """the twelve triangles of the box with a record of class c in front (or at the end); the others as they are in the box"""
        own = _cls(self.base)
        k = next(k for k in range(12) if self.can(k, c))
        rest = [j for j in range(12) if j != k]
        order = rest + [k] if last else [k] + rest
        return self.scene(order, [c if j == k else own[j] for j in order])


@pytest.fixture(scope="module")
def pool():
    return _Pool()


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    for name, v in (("flat_zero_classes", 1), ("plain_kernel", 1), ("lambert_kernel", 1), ("persistent", -1)): c.set_option(name, v)
    c.close()


def _render(ctx, spp=SPP):
    ctx.reset(); ctx.render(0, spp, SEED)
    return ctx.read_accum()


def _three_ways(ctx, arrays, cam, label, lambert, depths=DEPTHS, lit=True):
    """switch on == switch to the general body == generic FLAT kernel, per depth; returns the device's class table"""
    from pbrpathtracer_amd import ptk
    ctx.set_option("flat_zero_classes", 1); ctx.set_option("plain_kernel", 1)
    ctx.upload_scene(arrays); ctx.set_camera(**cam); ctx.set_tile(0, 1)
    classes = ctx.flat_classes()
    assert classes == _cls(arrays), label
    for D in depths:
        ctx.set_frame(W, H, D)
        on = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("flat_zero_classes", 0)
        off = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == lambert, label
        ctx.set_option("flat_zero_classes", 1)
        ctx.set_option("plain_kernel", 0)
        generic = _render(ctx)
        assert ctx.trace_variant() == ptk.TRACE_FLAT, label
        ctx.set_option("plain_kernel", 1)
        assert np.array_equal(on, generic), (label, D, "against the generic FLAT kernel", int((on != generic).sum()))
        assert np.array_equal(on, off), (label, D, "against flat_zero_classes = 0", int((on != off).sum()))
        assert not lit or D == 0 or (on != 0).any(), (label, D)
    return classes


def _both_levels(ctx, pool, arrays, label, depths=DEPTHS):
    """the list through the LAMBERT level, and with a mirror material through the generic level of the PLAIN kernel"""
    from pbrpathtracer_amd import ptk
    assert ptk.scene_is_plain(arrays) and ptk.scene_is_lambert(arrays), label
    got = _three_ways(ctx, arrays, pool.cam, (label, "lambert"), True, depths)
    m = Z.mirror(arrays)
    assert ptk.scene_is_plain(m) and not ptk.scene_is_lambert(m), label
    assert _three_ways(ctx, m, pool.cam, (label, "mirror"), False, depths) == got
    return got


def test_every_class_first_and_every_class_last(ctx, pool):
    first, last = set(), set()
    for c in range(16):
        first.add(_both_levels(ctx, pool, pool.with_first(c), ("first", c))[0])
        last.add(_both_levels(ctx, pool, pool.with_first(c, last=True), ("last", c))[-1])
    assert first == set(range(16)) and last == set(range(16))


def test_the_scenes_reach_all_sixteen_classes_on_the_host(pool):
    """no device needed for the claim itself: by flat_zero_class's rule the pool has a record of every class"""
    reach = set()
    for k in range(len(pool.rows)): reach |= set(pool.rows[k])
    assert reach == set(range(16)), sorted(set(range(16)) - reach)
    assert all(_cls(pool.with_first(c))[0] == c and _cls(pool.with_first(c, last=True))[-1] == c for c in range(16))


def test_lists_of_1_2_15_and_16_records(ctx, pool):
    a, _ = Z.cornell()
    one, two = Z.one_triangle(a), Z.subset(a, pool.lights)
    fifteen, sixteen = Z.subset(pool.base, range(15)), pool.base
    for arrays, n in ((one, 1), (two, 2), (fifteen, 15), (sixteen, 16)):
        assert len(arrays["verts"]) == n
        assert len(_both_levels(ctx, pool, arrays, ("records", n))) == n


def test_one_class_throughout_and_lists_that_alternate_between_the_ends_of_the_tree(ctx, pool):
    a, _ = Z.cornell()
    # one class: twelve general records; the four y-plane records of the box's floor and ceiling with the light, all class 8
    assert set(_both_levels(ctx, pool, Z.skewed(a), "all general")) == {0}
    ys = [k for k in range(12) if Z.plane_axis(pool.base["verts"][k]) == 1 and pool.can(k, 8)]
    assert len(ys) >= 4 and set(pool.lights) <= set(ys)
    assert set(_both_levels(ctx, pool, pool.scene(ys, [8] * len(ys)), "all class 8")) == {8}
    # 0 / 15: the four z-plane triangles (back wall, one panel) as class 15 between skewed (general) triangles, the lights in front
    zs = [k for k in range(16) if pool.can(k, 15)]
    others = [k for k in range(16) if k not in zs and k not in pool.lights]
    assert len(zs) == 4
    order, classes = list(pool.lights), [_cls(pool.base)[k] for k in pool.lights]
    for i, z in enumerate(zs):
        order += [others[i], z]; classes += [0, 15]
    order += others[len(zs):len(zs) + 2]; classes += [0, 0]
    got = _both_levels(ctx, pool, pool.scene(order, classes), "0 / 15")
    assert got[2:10] == [0, 15] * 4
    # 7 / 8: x-plane triangles as class 7 and y-plane triangles as class 8 in turn, twice over, then the rest of the box
    xs = [k for k in range(16) if pool.can(k, 7)]
    y8 = [k for k in range(16) if pool.can(k, 8)]
    assert len(xs) >= 4 and len(y8) >= 4
    order, classes = [], []
    for x, y in zip(xs[:4], y8[:4]):
        order += [x, y]; classes += [7, 8]
    rest = [k for k in range(12) if k not in order]
    order += rest; classes += [_cls(pool.base)[k] for k in rest]
    assert set(pool.lights) <= set(order)
    got = _both_levels(ctx, pool, pool.scene(order, classes), "7 / 8")
    assert got[:8] == [7, 8] * 4


def test_one_item_per_wave_and_a_three_way_tile_split(ctx, pool):
    """one item per wave ("persistent" 0): a wave's lanes run out of units at its item's end, so most lanes of its last passes are not in
    TRAV; tiles dealt to three ranks add up to the frame.  The distribution never changes a sample."""
    from pbrpathtracer_amd import ptk
    for arrays, lambert in ((pool.with_first(15), True), (Z.mirror(pool.with_first(0, last=True)), False)):
        want = None
        for persistent in (-1, 0, 1):
            ctx.set_option("persistent", persistent)
            ctx.upload_scene(arrays); ctx.set_camera(**pool.cam); ctx.set_frame(W, H, 8); ctx.set_tile(0, 1)
            for use, plain in ((1, 1), (0, 1), (1, 0)):
                ctx.set_option("flat_zero_classes", use); ctx.set_option("plain_kernel", plain)
                got = _render(ctx)
                assert ctx.trace_variant() == (ptk.TRACE_FLAT_PLAIN if plain else ptk.TRACE_FLAT) and (not plain or ctx.trace_is_lambert() == lambert)
                want = got if want is None else want
                assert np.array_equal(got, want), (lambert, persistent, use, plain, int((got != want).sum()))
            ctx.set_option("flat_zero_classes", 1); ctx.set_option("plain_kernel", 1)
        ctx.set_option("persistent", -1)
        assert (want != 0).any()
        total = np.zeros_like(want)
        for r in range(3):
            ctx.set_tile(r, 3)
            part = _render(ctx)
            assert not np.any((part != 0) & (total != 0))
            total += part
        ctx.set_tile(0, 1)
        assert np.array_equal(total, want), (lambert, "tiles")


def test_a_geometry_update_that_changes_the_class_word_between_two_renders(ctx, pool):
    """the back wall's two records go from classes 13 / 14 to 15 / 15 (vertices rolled: the same triangles) and then to general (skewed);
    each frame equals the generic FLAT kernel's and the switched-off pass's of the same geometry"""
    from pbrpathtracer_amd import ptk
    a, cam = Z.cornell()
    back = [k for k in range(12) if Z.plane_axis(a["verts"][k]) == 2]
    assert back == [0, 1]
    rolled, skew = Z.rolled(a, 3), Z.skewed(a, back)
    assert [_cls(rolled)[k] for k in back] == [15, 15] and [_cls(skew)[k] for k in back] == [0, 0] and [_cls(a)[k] for k in back] == [13, 14]
    for level_lambert in (True, False):
        ctx.set_option("lambert_kernel", 1 if level_lambert else 0)
        ctx.set_option("flat_zero_classes", 1); ctx.set_option("plain_kernel", 1)
        ctx.upload_scene(a); ctx.set_camera(**cam); ctx.set_frame(W, H, 8); ctx.set_tile(0, 1)
        frames = []
        for step, arrays in (("box", a), ("rolled", rolled), ("skewed", skew), ("box again", a)):
            if step != "box": ctx.update_geometry(0, arrays["verts"][back], arrays["normals"][back], arrays["tbn"][back])
            want = [_cls(arrays)[k] if k in back else c for k, c in enumerate(_cls(a))]         # (only the wall is updated)
            assert ctx.flat_classes() == want, step
            on = _render(ctx)
            assert ctx.trace_variant() == ptk.TRACE_FLAT_PLAIN and ctx.trace_is_lambert() == level_lambert
            ctx.set_option("plain_kernel", 0)
            generic = _render(ctx)
            ctx.set_option("plain_kernel", 1)
            ctx.set_option("flat_zero_classes", 0)
            off = _render(ctx)
            ctx.set_option("flat_zero_classes", 1)
            assert np.array_equal(on, generic) and np.array_equal(on, off), (level_lambert, step)
            frames.append(on)
        # the skewed wall gives another frame; back in place: the first frame again
        assert not np.array_equal(frames[0], frames[2]) and np.array_equal(frames[0], frames[3])
    ctx.set_option("lambert_kernel", 1)
