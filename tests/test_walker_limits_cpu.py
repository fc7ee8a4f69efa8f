"""What tests/test_gpu_walker_limits.py rests on, held on the CPU: the closest-point walk's stack lower bound
(stats_bounds.closest_stack_lower_bound) on a hand-built tree and on the host builder's tree of the nest, and the references and
conditions of tests/walker_limit_cases.py - the far rays the closest hit is tree-independent for, the far and adversarial point sets
the closest-point rule answers, and hit_rule's mirror against the oracle's brute force on the nest."""
import os
import subprocess

import numpy as np
import pytest

import closest_rule as CR
import hit_rule as HR
import stats_bounds as SB
import walker_limit_cases as WC
from bvh_check import check_bvh
from conftest import ROOT
from oracle import oracle_binding as OB
from test_gpu_bvh_limits import PTK_MAX_BVH_DEPTH, STACK_REALISED, _brute
from test_stats_counting_cpu import _leaf, _node, _wall


def test_closest_stack_lower_bound_on_a_hand_built_tree():
    """tests/test_stats_counting_cpu.py's tree with its empty slots marked as the builders mark them.  Root: node 1 over x in [2, 8] and
    leaves over [10, 12], [20, 24], [30, 31]; node 1: node 2 over [2, 4], a leaf with the very same box, a leaf over [5, 8]; node 2:
    leaves over [2, 3] and [3.5, 4].  Boxes span y, z in [0, 4]: the points lie at y = z = 1, so only x counts."""
    g = lambda x0, x1: ((int(x0 * 8), 0, 0), (int(x1 * 8), 32, 32))
    X = SB.NODE_EXIT
    nodes = np.stack([_node([g(2, 8), g(10, 12), g(20, 24), g(30, 31)], [1, _leaf(0, 1), _leaf(1, 1), _leaf(2, 1)]),
                      _node([g(2, 4), g(2, 4), g(5, 8)], [2, _leaf(3, 1), _leaf(4, 1), X]),
                      _node([g(2, 3), g(3.5, 4)], [_leaf(5, 1), _leaf(6, 1), X, X])])
    verts = np.array([_wall(11), _wall(21), _wall(30.5), _wall(3), _wall(6), _wall(2.5), _wall(3.75)], np.float32)
    x = [2.5, 3.2, 31.5, 9.0, 8.5, 4.0, 1000.0]
    pts = np.array([(v, 1, 1) for v in x], np.float32)
    b = SB.closest_stack_lower_bound(nodes, verts, pts)
    # 2.5:  inside [2, 8] alone: 3 deferred; inside both twin boxes of node 1, the lower slot (node 2) wins: 2; inside [2, 3]: 1
    # 3.2:  as before down to node 2, where [2, 3] at 0.2 is surely nearer than [3.5, 4] at 0.3: the same 6
    # 31.5: the root's nearest child is the leaf [30, 31]: the first leaf, the 3 others deferred
    # 9:    [2, 8] and [10, 12] both at distance 1: no child is surely the nearest, the root's 3 count and the chain ends
    # 8.5:  [2, 8] at 0.5 against 1.5: 3; in node 1 the leaf [5, 8] at 0.5 against 4.5: 2, and that is the first leaf
    # 4:    on the face of [2, 8], nearest by distance: 3; on the face of both twins: inside neither for sure, 2 and the chain ends
    # 1000: far outside, 969 to [30, 31] against 976 to [20, 24]: 3
    assert b.tolist() == [6, 6, 3, 3, 5, 5, 3]
    assert b.dtype == np.int64


@pytest.fixture(scope="module")
def bvh_dump(tmp_path_factory):
    """tests/cpp/bvh_dump.cpp: the host builder stand-alone.  (verts, leaf_max) -> (nodes [N, 16], order, stack_need)"""
    d = tmp_path_factory.mktemp("bvh_dump")
    exe = str(d / "bvh_dump")
    subprocess.check_call(["g++", "-O2", "-std=c++17", "-I" + os.path.join(ROOT, "pbrpathtracer_amd", "csrc"),
                           os.path.join(ROOT, "tests", "cpp", "bvh_dump.cpp"),
                           os.path.join(ROOT, "pbrpathtracer_amd", "csrc", "bvh_build.cpp"), "-o", exe, "-pthread"])

    def build(verts, leaf_max):
        vf, nf, of = (str(d / f) for f in ("verts.f32", "nodes.f32", "order.i32"))
        np.ascontiguousarray(verts, np.float32).tofile(vf)
        out = subprocess.run([exe, vf, str(leaf_max), nf, of], capture_output=True, text=True)
        assert out.returncode == 0, out.stdout + out.stderr
        n_nodes, _, stack_need = (int(x) for x in out.stdout.split())
        nodes = np.fromfile(nf, np.float32).reshape(-1, 16)
        assert len(nodes) == n_nodes
        return nodes, np.fromfile(of, np.int32), stack_need
    return build


def test_nest_fills_the_closest_point_walks_stack(bvh_dump):
    verts = WC._nest()["verts"]
    pts = WC.nest_points()
    assert pts.dtype == np.float32 and pts.shape == (600, 3)
    best = {}
    for L in (1, 8):
        nodes, order, stack_need = bvh_dump(verts, L)
        info = check_bvh(nodes, order, verts, leaf_max=L)
        assert info["stack_need"] == stack_need == PTK_MAX_BVH_DEPTH
        lb = SB.closest_stack_lower_bound(nodes, verts, pts)
        best[L] = int(lb.max())
        print(f"nest leaf_max {L}: {len(nodes)} nodes, stack_need {stack_need}, largest realised closest-point stack lower bound "
              f"{lb.max()} ({(lb == lb.max()).mean():.0%} of the points; by group {[int(lb[k:k + 200].max()) for k in (0, 200, 400)]})")
        assert lb.max() <= stack_need
    assert best[1] >= STACK_REALISED, best


@pytest.mark.parametrize("e", WC.FAR_EXPONENTS)
def test_far_rays_and_points_have_tree_free_answers(e):
    verts, ro, rd = WC.far_cluster(e)
    arrays = WC._scene(verts)
    m = len(ro)
    assert m == 600
    o = OB.Oracle(arrays)
    ref = _brute(o, ro, rd)
    o.close()
    tri, t, bary, _ = WC.hits_reference(OB, ("far", e), arrays, ro, rd)
    hit = ref[0] >= 0
    assert np.array_equal(tri, ref[0]) and np.array_equal(t[hit], ref[1][hit, 0]) and np.array_equal(bary[hit], ref[1][hit, 1:])
    ill = WC._off_box(verts, ro, rd, ref)
    print(f"2^{e}: {int(ill.sum())} of {m} rays hit off their triangle's box by more than the slack, {hit[m // 2:].mean():.2f} of the near rays hit")
    assert ill.sum() <= m // 100, ill.sum()
    assert (ref[0][m // 2:] >= 0).mean() >= 0.3
    pts = WC.far_points(e)
    assert pts.dtype == np.float32 and pts.shape == (300, 3) and np.isfinite(pts).all()
    full = CR.mirror_full(arrays, pts)
    assert (full["tri"] >= 0).all() and np.isfinite(full["dist"]).all()


def test_duplicates_tie_on_the_winning_side():
    seed = WC.SOAK_SEEDS["duplicates"]
    verts = WC._soak_scene("duplicates", seed)
    pts = WC.soak_points("duplicates", verts, seed)
    assert pts.dtype == np.float32 and pts.shape == (800, 3)
    full = CR.mirror_full(WC._scene(verts), pts)
    assert (full["tri"] >= 0).all()
    assert (full["ties"] >= 2).sum() >= 50, int((full["ties"] >= 2).sum())


def test_hit_mirror_equals_brute_force_on_the_nest():
    arrays = WC._nest()
    ro, rd = WC.nest_rays()
    o = OB.Oracle(arrays)
    ref = _brute(o, ro, rd)
    tri, t, bary, mat = HR.mirror(OB, arrays, ro, rd, HR.PROBE_KEY, oracle=o)
    o.close()
    hit = ref[0] >= 0
    assert (ref[0][:128] < 0).all() and hit[128:].mean() > 0.2
    assert np.array_equal(tri, ref[0])
    assert np.array_equal(t[hit], ref[1][hit, 0]) and np.isposinf(t[~hit]).all()
    assert np.array_equal(bary[hit], ref[1][hit, 1:]) and (mat[hit] == arrays["material"][tri[hit]]).all()
