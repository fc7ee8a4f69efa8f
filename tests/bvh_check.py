"""Structural check of a BVH as it lies in HBM (ptk_download_bvh): 4-wide nodes with 8-bit quantised child boxes
(pbrpathtracer_amd/csrc/ptk_device.h).  Vectorised over the nodes of a level so that a 370 000-node tree checks in seconds.
The same properties tests/cpp/test_bvh.cpp asserts of the host builder's output."""
import numpy as np


def check_bvh(nodes: np.ndarray, order: np.ndarray, verts: np.ndarray, max_stack: int = 32, leaf_max: int = 8):
    """nodes [N,16] float32 (bit patterns), order [n] int32 leaf order -> scene triangle, verts [n,9] float32.
    Returns dict(depth, stack_need, children_per_node); raises AssertionError on any violation."""
    n = len(verts)
    N = len(nodes)
    raw = nodes.view(np.uint32)
    origin = nodes[:, 0:3].astype(np.float64)
    scale = nodes[:, 3:6].astype(np.float64)
    link = raw[:, 6:10].view(np.int32)
    lo = np.stack([(raw[:, 10 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1).astype(np.float64)   # [N,4,3]
    hi = np.stack([(raw[:, 13 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1).astype(np.float64)
    valid = (lo <= hi).all(axis=2)                                   # [N,4]
    assert ((lo <= hi).any(axis=2) == valid).all(), "a slot is empty on some axes only"
    assert valid.any(axis=1).all(), "node without children"
    bmin = origin[:, None, :] + lo * scale[:, None, :]
    bmax = origin[:, None, :] + hi * scale[:, None, :]
    assert sorted(order.tolist()) == list(range(n)), "leaf order is not a permutation of the triangles"
    tri_lo = verts.reshape(n, 3, 3).min(axis=1).astype(np.float64)
    tri_hi = verts.reshape(n, 3, 3).max(axis=1).astype(np.float64)
    # union box of every node's children (for the nesting check)
    big = 1e300
    umin = np.where(valid[..., None], bmin, big).min(axis=1)
    umax = np.where(valid[..., None], bmax, -big).max(axis=1)

    seen_node = np.zeros(N, np.int32)
    seen_tri = np.zeros(n, np.int32)
    level = np.array([0]); used = np.array([0])
    depth = 0; stack_need = 0; children = 0
    while len(level):
        depth += 1
        np.add.at(seen_node, level, 1)
        nc = valid[level].sum(axis=1)
        children += int(nc.sum())
        used_here = used + nc - 1
        stack_need = max(stack_need, int(used_here.max()))
        nxt, nxt_used = [], []
        for k in range(4):
            v = valid[level, k]
            idx = level[v]; lk = link[idx, k]; u = used_here[v]
            inner = lk >= 0
            ci = lk[inner]
            assert (ci < N).all() and (ci > idx[inner]).all(), "interior link out of range / not forward"
            # nesting: the child's own union box lies inside this child box up to the grid steps of both levels
            slack = scale[ci] + scale[idx[inner]]
            assert (umin[ci] >= bmin[idx[inner], k] - slack).all() and (umax[ci] <= bmax[idx[inner], k] + slack).all(), "child node outside its parent's box"
            nxt.append(ci); nxt_used.append(u[inner])
            code = ~lk[~inner]
            first, count = code >> 3, (code & 7) + 1
            assert (first >= 0).all() and (first + count <= n).all() and (count <= leaf_max).all(), "bad leaf range"
            li = idx[~inner]
            for j in range(int(count.max()) if len(count) else 0):
                m = count > j
                t = order[first[m] + j]
                np.add.at(seen_tri, t, 1)
                assert (tri_lo[t] > bmin[li[m], k]).all() and (tri_hi[t] < bmax[li[m], k]).all(), "triangle not strictly inside its leaf box"
        level = np.concatenate(nxt) if nxt else np.array([], np.int64)
        used = np.concatenate(nxt_used) if nxt_used else np.array([], np.int64)
        assert depth <= 64
    assert (seen_node == 1).all(), "node reached %s times" % np.unique(seen_node)
    assert (seen_tri == 1).all(), "triangle in %s leaves" % np.unique(seen_tri)
    assert stack_need <= max_stack, (stack_need, max_stack)
    return dict(depth=depth, stack_need=stack_need, children_per_node=children / N, nodes=N)


def leaf_sizes(nodes: np.ndarray) -> np.ndarray:
    """Histogram of leaf sizes of a downloaded BVH4: [9] int, entry c = leaves of c triangles (decoded as the walk decodes a leaf
    link: ~link = first << 3 | (count - 1))."""
    raw = np.ascontiguousarray(nodes, np.float32).view(np.uint32)
    link = raw[:, 6:10].view(np.int32)
    lo = np.stack([(raw[:, 10 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1)
    hi = np.stack([(raw[:, 13 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1)
    leaf = (lo <= hi).all(axis=2) & (link < 0)
    return np.bincount(((~link[leaf]) & 7) + 1, minlength=9)
