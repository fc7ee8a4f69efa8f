"""The BVH walk and both builders at their limits, against the oracle's brute-force closest hit (Oracle.hit(brute=True): every
triangle, the reference's IntersectTriangle and its tie rule).  Closest hits do not depend on the tree (include/ptk.h, DESIGN
§2): these tests hold the kernels to that where the suite's other trees are mild - leaves of 5 to 8 triangles (builder tuning
"bvh_leaf_max" / "bvh_trav_cost"), a traversal stack filled to its bound, the device builder's size switch, its multi-round
prefix sum and its fall-back to the host builder, adversarial geometry, and coordinates and ray distances near the accepted
maximum with direction components on both sides of the 1 / d clamp.  These tests drive probe_hits and render; the scenes, rays
and the off-box exclusion live in tests/walker_limit_cases.py, and tests/test_gpu_walker_limits.py holds every other kernel that walks
the tree (hit, occlusion, closest-point and radiance queries, feature planes, picking) to tree-free references on the same cases."""
import numpy as np
import pytest

import stats_bounds as SB
from bvh_check import check_bvh, leaf_sizes
from test_gpu_bvh_build import _scene, _soup
from test_gpu_random_scenes import random_scene
from walker_limit_cases import (SOAK_KINDS, TINY, _aimed_rays, _glow, _nest, _off_box, _onion, _soak_scene, far_case, nest_rays)   # noqa: F401

pytestmark = pytest.mark.gpu

PTK_MAX_BVH_DEPTH = 32            # include/ptk.h
STACK_REALISED = 24               # what stats_bounds.stack_lower_bound proves of the nest (host builder, leaf_max 1)


@pytest.fixture(scope="module")
def ctx():
    from pbrpathtracer_amd import ptk
    c = ptk.Context(0)
    yield c
    c.close()


@pytest.fixture
def tuning(ctx):
    """Builder tuning is process-wide (g_bvh_tuning): whatever a test sets is set back to the builders' own choices."""
    def set_(leaf_max, trav_cost=0):
        ctx.set_option("bvh_leaf_max", leaf_max)
        ctx.set_option("bvh_trav_cost", trav_cost)
    try:
        yield set_
    finally:
        set_(0, 0)
        ctx.set_option("device_build", 1)
        ctx.set_option("flat", 1)
        ctx.set_option("tri_threshold", 6)


def _brute(o, ro, rd):
    tri = np.full(len(ro), -1, np.int32)
    tuv = np.zeros((len(ro), 3), np.float32)
    for j in range(len(ro)):
        h, t, v = o.hit(ro[j], rd[j], brute=True)
        if h:
            tri[j], tuv[j] = t, v
    return tri, tuv


def _assert_hits(ctx, ro, rd, ref, what):
    tri, tuv = ctx.probe_hits(ro, rd)
    bad = np.nonzero((tri != ref[0]) | ((tri >= 0) & (tuv != ref[1]).any(axis=1)))[0]
    assert len(bad) == 0, f"{what}: {len(bad)} of {len(ro)} rays differ from brute force, first {bad[:5].tolist()}"
    return tri, tuv


def _upload(ctx, arrays, device_build, strict=True):
    ctx.set_option("device_build", device_build)
    ctx.upload_scene(arrays)
    if strict:
        assert ctx.upload_timing()["built_on_device"] == bool(device_build)
    nodes, order = ctx.download_bvh()
    return nodes, order


def _render_matches(ctx, o, oracle_mod, cam, W=40, H=28, D=4, spp=2, seed=9):
    ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
    ref_img, ref8 = o.render(ocam, W, H, D, 0, spp, seed)
    assert ref_img.max() > 0, "a black render is a poor test"
    ctx.set_option("flat", 0)
    ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1); ctx.reset()
    ctx.render(0, spp, seed)
    assert np.array_equal(ctx.read_accum(), ref_img) and np.array_equal(ctx.resolve_rgb8(), ref8)


# ---- 1. leaves of every size up to 8, both builders -----------------------------------------------------------------------

def _sweep_scenes():
    soup = _scene(_soup(20000, 0.03, 31))
    textured, cam = random_scene(41, 6000, True)
    assert any((m["tex"][5] >= 0) for m in textured["materials"]), "the textured scene needs opacity maps"
    return [("soup 20k", soup, None), ("textured 6000", textured, cam)]


@pytest.mark.parametrize("scene", [0, 1], ids=["soup 20k", "textured 6000"])
def test_leaf_size_sweep_gives_tree_independent_hits(ctx, oracle_mod, tuning, scene):
    name, arrays, cam = _sweep_scenes()[scene]
    verts = arrays["verts"]
    ro, rd = _aimed_rays(verts, 2000, 7 + scene)
    o = oracle_mod.Oracle(arrays)
    ref = _brute(o, ro, rd)
    assert (ref[0] >= 0).mean() > 0.5
    if cam is not None:
        W, H, D, spp, seed = 40, 28, 5, 3, 77
        ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
        ref_img, ref8 = o.render(ocam, W, H, D, 0, spp, seed)
        assert (ref_img != 0).any(axis=2).mean() > 0.5
    o.close()
    for L in (1, 2, 3, 5, 8):
        sizes = {0: np.zeros(9, np.int64), 1: np.zeros(9, np.int64)}
        for cost in (0, 4, 16):
            tuning(L, cost)
            hits = []
            for dev in (0, 1):
                nodes, order = _upload(ctx, arrays, dev)
                info = check_bvh(nodes, order, verts, leaf_max=L)
                assert info["stack_need"] == ctx.bvh_layout()[2]
                h = leaf_sizes(nodes)
                assert h[L + 1:].sum() == 0 and h[0] == 0
                sizes[dev] += h
                print(f"{name}: leaf_max {L} trav_cost {cost} {'device' if dev else 'host'}: leaf sizes 1..8 {h[1:].tolist()}, "
                      f"stack {info['stack_need']}, depth {info['depth']}")
                hits.append(_assert_hits(ctx, ro, rd, ref, f"{name} L{L} c{cost} dev{dev}"))
                if cam is not None and (L, cost) in ((8, 4), (1, 0)):
                    ctx.set_option("flat", 0)
                    for thr in (0, 6, 64):
                        ctx.set_option("tri_threshold", thr)
                        ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1); ctx.reset()
                        ctx.render(0, spp, seed)
                        assert np.array_equal(ctx.read_accum(), ref_img), (L, cost, dev, thr)
                        assert np.array_equal(ctx.resolve_rgb8(), ref8)
                    ctx.set_option("tri_threshold", 6)
            assert np.array_equal(hits[0][0], hits[1][0]) and np.array_equal(hits[0][1], hits[1][1])
        for dev in (0, 1):
            # what makes the sweep worth running: the walk decodes leaves of every size the tuning allows
            assert (sizes[dev][2:L + 1] > 0).all(), (name, L, dev, sizes[dev].tolist())


# ---- 2. a traversal stack filled to its bound --------------------------------------------------------------------------

def test_full_traversal_stack_is_reached_and_gives_exact_hits(ctx, oracle_mod, tuning):
    arrays = _nest()
    verts = arrays["verts"]
    ro, rd = nest_rays()
    m = len(ro)
    o = oracle_mod.Oracle(arrays)
    ref = _brute(o, ro, rd)
    assert (ref[0][:m // 2] < 0).all() and (ref[0][m // 2:] >= 0).mean() > 0.2
    W, H, D, spp, seed = 48, 32, 4, 2, 9
    cam = dict(pos=np.array([-1.0, 0.0, 0.0], np.float32), dir=np.array([1.0, 0.0, 0.0], np.float32), up=np.array([0.0, 0.0, 1.0], np.float32),
               focal=0.05, fovy=20.0, focal_dist=3.0, aperture=0.0)
    ocam = oracle_mod.make_camera(cam["pos"], cam["dir"], cam["up"], cam["focal"], cam["fovy"], cam["focal_dist"], cam["aperture"])
    ref_img, ref8 = o.render(ocam, W, H, D, 0, spp, seed)
    o.close()
    assert ref_img.max() > 0
    best = 0
    for L in (1, 8):
        for dev in (0, 1):
            tuning(L, 0)
            nodes, order = _upload(ctx, arrays, dev, strict=False)
            built = "device" if ctx.upload_timing()["built_on_device"] else "host"
            info = check_bvh(nodes, order, verts, leaf_max=L)
            assert info["stack_need"] == ctx.bvh_layout()[2] == PTK_MAX_BVH_DEPTH
            t = np.where(ref[0] >= 0, ref[1][:, 0], np.inf)
            lb = SB.stack_lower_bound(nodes, verts, ro, rd, t)
            print(f"nest leaf_max {L} device_build {dev} (built on the {built}): stack_need {info['stack_need']}, depth {info['depth']}, "
                  f"largest realised stack lower bound {lb.max()} ({(lb == lb.max()).sum()} rays)")
            best = max(best, int(lb.max()))
            _assert_hits(ctx, ro, rd, ref, f"nest L{L} dev{dev}")
            ctx.set_option("flat", 0)
            ctx.set_camera(**cam); ctx.set_frame(W, H, D); ctx.set_tile(0, 1); ctx.reset()
            ctx.render(0, spp, seed)
            assert np.array_equal(ctx.read_accum(), ref_img) and np.array_equal(ctx.resolve_rgb8(), ref8), (L, dev)
    assert best >= STACK_REALISED, best


# ---- 3. device-builder boundaries --------------------------------------------------------------------------------------

def test_builder_switch_at_4096_triangles(ctx, oracle_mod):
    ctx.set_option("device_build", 1)
    for n, dev in ((4095, False), (4096, True)):
        arrays = _scene(_soup(n, 0.03, n))
        ctx.upload_scene(arrays)
        assert ctx.upload_timing()["built_on_device"] is dev, n
        check_bvh(*ctx.download_bvh(), arrays["verts"])
        ro, rd = _aimed_rays(arrays["verts"], 300, n)
        o = oracle_mod.Oracle(arrays)
        _assert_hits(ctx, ro, rd, _brute(o, ro, rd), f"n {n}")
        o.close()


def test_device_build_past_one_scan_round(ctx, oracle_mod, tuning):
    """scan_sums_kernel carries its running sum between rounds of 1024 block sums: a binary tree of more than 1024 x 1024 nodes."""
    n = 700000
    verts = _soup(n, 0.004, 12)
    arrays = _scene(verts)
    tuning(1, 0)
    nodes, order = _upload(ctx, arrays, 1)
    leaves = int(leaf_sizes(nodes).sum())
    assert 2 * leaves - 1 > 1 << 20, leaves
    print(f"700k at leaf_max 1: {leaves} leaves, {2 * leaves - 1} binary nodes, {-(-(2 * leaves - 1) // 1024)} scan blocks")
    check_bvh(nodes, order, verts, leaf_max=1)
    ro, rd = _aimed_rays(verts, 200, 3)
    o = oracle_mod.Oracle(arrays)
    _assert_hits(ctx, ro, rd, _brute(o, ro, rd), "700k")
    o.close()


@pytest.mark.parametrize("name,leaf_max", [("onion 60k", 0), ("identical 300k", 1)])
def test_device_builder_falls_back_to_the_host_builder(ctx, oracle_mod, tuning, name, leaf_max):
    """The onion's device-built tree would defer more than the stack holds; 300 000 identical triangles at leaf_max 1 outgrow the
    device builder's node store (its parity splits may keep a pair together).  Either way the host builder takes over."""
    arrays = _onion() if name == "onion 60k" else _glow(_scene(np.tile(_soup(1, 0.3, 3), (300000, 1))), [0, 1])
    tuning(leaf_max, 0)
    ctx.set_option("device_build", 1)
    ctx.upload_scene(arrays)
    assert not ctx.upload_timing()["built_on_device"]
    print(f"fall-back to the host builder: {name} at leaf_max {leaf_max}, stack_need {ctx.bvh_layout()[2]}")
    check_bvh(*ctx.download_bvh(), arrays["verts"], leaf_max=max(leaf_max, 4))
    ro, rd = _aimed_rays(arrays["verts"], 150 if "300k" in name else 300, 4)
    o = oracle_mod.Oracle(arrays)
    _assert_hits(ctx, ro, rd, _brute(o, ro, rd), name)
    if name == "onion 60k":                 # (every ray into the identical stack walks all of it: probes only)
        cam = dict(pos=np.array([0.3, 0.2, 2.5], np.float32), dir=np.array([0.0, 0.0, -1.0], np.float32), up=np.array([0.0, 1.0, 0.0], np.float32),
                   focal=0.05, fovy=50.0, focal_dist=3.0, aperture=0.0)
        _render_matches(ctx, o, oracle_mod, cam)
    o.close()


@pytest.mark.parametrize("kind,seed", [(k, 100 + i) for i, k in enumerate(SOAK_KINDS)])
def test_adversarial_geometry_gives_brute_force_hits(ctx, oracle_mod, tuning, kind, seed):
    verts = _soak_scene(kind, seed)
    arrays = _scene(verts)
    ro, rd = _aimed_rays(verts, 400, seed)
    o = oracle_mod.Oracle(arrays)
    ref = _brute(o, ro, rd)
    o.close()
    for L in (0, 8):
        tuning(L, 4 if L else 0)
        for dev in (0, 1):
            nodes, order = _upload(ctx, arrays, dev)
            check_bvh(nodes, order, verts)
            _assert_hits(ctx, ro, rd, ref, f"{kind} L{L} dev{dev}")


# ---- 4. the far domain -------------------------------------------------------------------------------------------------

def test_largest_accepted_coordinate(ctx):
    from pbrpathtracer_amd import ptk
    top = np.float32(2.0 ** 61 - 2.0 ** 37)
    assert float(top) == 2.0 ** 61 - 2.0 ** 37 and np.nextafter(top, np.float32(np.inf)) == np.float32(2.0 ** 61)
    v = _soup(4096, 0.03, 5)
    v[0, 0] = top
    ctx.upload_scene(_scene(v))
    v[0, 0] = np.float32(2.0 ** 61)
    with pytest.raises(ptk.PtkError):
        ctx.upload_scene(_scene(v))
    v[0, 0] = -top
    ctx.upload_scene(_scene(v))


@pytest.mark.parametrize("e", [20, 40, 59])
def test_far_clusters_and_far_rays_give_brute_force_hits(ctx, oracle_mod, tuning, e):
    case = far_case(e)
    verts, ro, rd, dist = case["verts"], case["ro"], case["rd"], case["dist"]
    arrays = _scene(verts)
    m = len(ro)
    o = oracle_mod.Oracle(arrays)
    ref = _brute(o, ro, rd)
    o.close()
    assert (ref[0][m // 2:] >= 0).mean() > 0.3
    ill = _off_box(verts, ro, rd, ref)
    assert ill.sum() <= m // 100, ill.sum()
    ok = ~ill
    print(f"2^{e}: {int(ill.sum())} of {m} rays hit off their triangle's box by more than the slack (left out)")
    for L in (1, 8):
        tuning(L, 0)
        for dev in (0, 1):
            nodes, order = _upload(ctx, arrays, dev)
            check_bvh(nodes, order, verts, leaf_max=L)
            bmin, bmax, valid, link = SB.decode(nodes)
            leaf = valid & (link < 0)
            size = (bmax - bmin).max(axis=2)[leaf]
            ratio = (dist / np.median(size))[ok & (ref[0] >= 0)]
            print(f"2^{e}, leaf_max {L} {'device' if dev else 'host'}: distance / leaf box of the rays that hit {ratio.min():.2e} .. "
                  f"{ratio.max():.2e}, hits {(ref[0] >= 0).mean():.2f}")
            _assert_hits(ctx, ro[ok], rd[ok], (ref[0][ok], ref[1][ok]), f"2^{e} L{L} dev{dev}")
