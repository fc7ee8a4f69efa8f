"""Per-ray bounds on what the BVH walk of the trace kernels counts (ptk_stats node_visits, tri_tests, max_walk_nodes and the
opacity share of tex_fetches), from the tree as it lies in HBM (ptk_download_bvh, decoded as tests/bvh_check.py decodes it)
and the oracle's record of every ray cast (oracle_binding.Oracle.render_counted(dump=True)).  Pure numpy.

Why bounds and not counts: the walk defers its triangle arm by a wave vote (option "tri_threshold"), so when a ray's closest hit
so far tightens - and with it which child boxes it still enters - depends on the other lanes of its wave.

Lower bound.  best.t never drops below the ray's final t (the oracle's closest hit, bit-identical), and the walk enters a child
box when max(t_near, 0) <= min(t_far, best.t * 1.0000153) on a box that contains the quantised one.  So every child box the ray
enters before its final t (on the quantised box shrunk by MARGIN) is visited, and every triangle of every such leaf is tested.
This holds for camera and bounce rays and for shadow rays that reach their light; an occluded shadow ray stops at an occluder
that may come first, so its bound is the root alone.
Upper bound.  Every child box the ray's half line enters at all, on the quantised box inflated by MARGIN, with axes the ray
(nearly) runs parallel to left unconstrained.
Shadow rays add the test of their light triangle that shade_interaction makes before the walk to both triangle bounds.

Opacity texels: a candidate reads one when Moeller-Trumbore accepts it and it is nearer than the best hit so far (or as near with
a smaller index).  Lower bound: the candidates of the lower-bound leaves nearer than the final hit, the final hit itself, and the
light pre-test.  Upper bound: every candidate of the upper-bound leaves that Moeller-Trumbore accepts, and the light pre-test.
Moeller-Trumbore is the oracle's (oracle_binding.intersect_many), bit-identical to the kernels' - no margin there.

Deferred entries (stack_lower_bound).  At an interior node walk_step writes every child box the ray enters to the LDS stack
except the one with the smallest key - the entry distance t_near with the slot in its two low bits - and goes on with that one.
The kernel's t_near lies between the entry distance of the quantised box inflated by MARGIN and that of the box shrunk by
MARGIN, so a child is surely pushed when the ray surely enters it before its final t and another child it surely enters has
a sure entry earlier than this child's earliest possible one - or has the very same quantised box in a lower slot (the same
bytes give the same t_near, bit for bit, and the slot bits break the tie).  The walk pops nothing while it goes on into interior nodes,
so along the chain of children that are surely the nearest the pushes add up: their sum is a lower bound on the entries the
ray's stack holds at once.

Deferred entries of the closest-point walk (closest_stack_lower_bound; closest_kernel, ptk_closest.hip).  Without a radius
(max_dist NULL) the prune bound thr2 is +inf until the first leaf has been tested, so at every interior node of the first descent
every non-empty child (link != NODE_EXIT) survives: the walk goes on into the one with the smallest key - the bits of the squared
box distance db2 with the two low bits replaced by the slot - and defers the other children - 1, whichever child that is.  Nothing
is popped before the first leaf.  So the sum of children - 1 over the nodes of that descent is held at once, and the nodes of the
descent are known as far as one child is surely the nearest.  The kernel's child box lies between the quantised box shrunk and
inflated by MARGIN x (max |p| + 2 extent), so a child is surely the nearest when
  - the point lies inside its shrunk box (the kernel's db2 is then exactly 0 and its key is its slot) and every other non-empty child
    sits in a higher slot or has the point outside its inflated box (a db2 of at least the square of what is left of the margin:
    a key above 3), or
  - its largest possible distance (to the shrunk box) is below every other non-empty child's smallest possible one (to the inflated
    box) by the factor 1 - 2^-20 on the distance, 2^-19 on db2: the key's two dropped bits and the few roundings of db2 are 2^-21.
Where no child is surely the nearest the node's own children - 1 still count - they are deferred whichever child wins - and the
chain ends there.
"""
import numpy as np

# relative to (max |ray origin| + scene extent): the kernel's own slack is 2^-21 of that per slab distance (Walk::begin)
MARGIN = 2.0 ** -16
PARALLEL = 1e-6          # |direction component| below which the upper bound does not let that axis cull
NODE_EXIT = -2 ** 31     # the link of an empty slot (ptk_device.h)


def decode(nodes: np.ndarray):
    """BVH4 records [N, 16] -> (bmin [N,4,3], bmax [N,4,3] float64, valid [N,4], link [N,4] int32)."""
    raw = np.ascontiguousarray(nodes, np.float32).view(np.uint32)
    origin = nodes[:, 0:3].astype(np.float64)
    scale = nodes[:, 3:6].astype(np.float64)
    link = raw[:, 6:10].view(np.int32)
    lo = np.stack([(raw[:, 10 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1).astype(np.float64)
    hi = np.stack([(raw[:, 13 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(3)], axis=-1).astype(np.float64)
    valid = (lo <= hi).all(axis=2)
    return origin[:, None, :] + lo * scale[:, None, :], origin[:, None, :] + hi * scale[:, None, :], valid, link


def _slabs(bmin, bmax, ro, rd, free):
    """t_near, t_far of boxes [M,3] for rays [M,3] in float64; axes in `free` [M,3] do not constrain."""
    with np.errstate(divide="ignore", invalid="ignore"):
        inv = 1.0 / rd
        t0 = (bmin - ro) * inv
        t1 = (bmax - ro) * inv
    tn = np.where(free, -np.inf, np.minimum(t0, t1))
    tf = np.where(free, np.inf, np.maximum(t0, t1))
    # a zero component that does constrain: the ray is inside that slab for every t or for none
    inside = (ro >= bmin) & (ro <= bmax)
    zero = (rd == 0.0) & ~free
    tn = np.where(zero, np.where(inside, -np.inf, np.inf), tn)
    tf = np.where(zero, np.where(inside, np.inf, -np.inf), tf)
    return tn.max(axis=1), tf.min(axis=1)


def _walk(tree, ro, rd, t_lim, margin, free, lower):
    """Level by level over (ray, node) pairs.  Returns per ray: nodes visited, leaf triangles, and the (ray, leaf record) pairs."""
    bmin, bmax, valid, link = tree
    n = len(ro)
    nodes = np.zeros(n, np.int64)
    tris = np.zeros(n, np.int64)
    cand_r, cand_rec = [], []
    ray = np.arange(n)
    node = np.zeros(n, np.int64)
    while len(ray):
        np.add.at(nodes, ray, 1)
        nxt_r, nxt_n = [], []
        for k in range(4):
            v = valid[node, k]
            r, nd = ray[v], node[v]
            m = margin[r][:, None]
            lo = bmin[nd, k] + (m if lower else -m)
            hi = bmax[nd, k] - (m if lower else -m)
            ok = (lo <= hi).all(axis=1)
            tn, tf = _slabs(lo, hi, ro[r], rd[r], free[r])
            ok &= (np.maximum(tn, 0.0) <= tf)
            if lower:
                ok &= tn < t_lim[r]
            r, lk = r[ok], link[nd[ok], k]
            inner = lk >= 0
            nxt_r.append(r[inner]); nxt_n.append(lk[inner])
            code = ~lk[~inner]
            first, count = code >> 3, (code & 7) + 1
            rl = r[~inner]
            np.add.at(tris, rl, count)
            for j in range(int(count.max()) if len(count) else 0):
                s = count > j
                cand_r.append(rl[s]); cand_rec.append(first[s] + j)
        ray = np.concatenate(nxt_r)
        node = np.concatenate(nxt_n)
    cr = np.concatenate(cand_r) if cand_r else np.zeros(0, np.int64)
    cc = np.concatenate(cand_rec) if cand_rec else np.zeros(0, np.int64)
    return nodes, tris, cr, cc


def ray_bounds(nodes, order, verts, rays, opacity_tris=None, intersect=None):
    """nodes [N,16] float32, order [n] leaf record -> scene triangle, verts [n,9] float32, rays: oracle ray records
    (oracle_binding.RAY_DTYPE).  opacity_tris: bool [n], triangles whose material has an opacity texture (None: no opacity
    bounds); intersect: oracle_binding.intersect_many.  Returns dict of int64 arrays per ray: node_lo, node_hi, tri_lo, tri_hi
    (and opa_lo, opa_hi)."""
    tree = decode(nodes)
    ro = rays["ro"].astype(np.float64)
    rd = rays["rd"].astype(np.float64)
    t = rays["t"].astype(np.float64)
    shadow = rays["kind"] == 2
    occluded = shadow & (rays["occluded"] != 0)
    extent = float(np.abs(verts).max()) if len(verts) else 1.0
    margin = MARGIN * (np.abs(ro).max(axis=1) + 2.0 * extent)
    t_lim = np.where(occluded, -np.inf, t)            # occluded shadow rays: nothing beyond the root is certain
    no_free = np.zeros(ro.shape, bool)
    n_lo, t_lo, lr, lrec = _walk(tree, ro, rd, t_lim, margin, no_free, lower=True)
    n_hi, t_hi, ur, urec = _walk(tree, ro, rd, None, margin, np.abs(rd) < PARALLEL, lower=False)
    out = dict(node_lo=n_lo, node_hi=n_hi, tri_lo=t_lo + shadow, tri_hi=t_hi + shadow)
    if opacity_tris is None:
        return out

    def accepted(r, tri):
        tuv = intersect(rays["ro"][r], rays["rd"][r], verts[tri])
        return (tuv[:, 0] > 0) & np.isfinite(tuv[:, 0]), tuv[:, 0]

    n = len(rays)
    light = rays["light"]
    pre = np.zeros(n, np.int64)                       # the light pre-test of a shadow ray reads its texel if it hits the light
    s = np.nonzero(shadow & (light >= 0))[0]
    s = s[opacity_tris[light[s]]]
    if len(s):
        pre[s] = accepted(s, light[s])[0]
    # lower: candidates of certain leaves nearer than the final hit (not the light: its pre-test is counted), plus the final hit
    lo = pre.copy()
    tri = order[lrec]
    keep = opacity_tris[tri] & (tri != light[lr]) & ~occluded[lr]
    r, tri = lr[keep], tri[keep]
    if len(r):
        hit, tt = accepted(r, tri)
        np.add.at(lo, r[hit & (tt < t[r])], 1)
    fin = (~shadow) & (rays["tri"] >= 0)
    fin[fin] = opacity_tris[rays["tri"][fin]]
    lo += fin
    hi = pre.copy()
    tri = order[urec]
    keep = opacity_tris[tri]
    r, tri = ur[keep], tri[keep]
    if len(r):
        hit, _ = accepted(r, tri)
        np.add.at(hi, r[hit], 1)
    out.update(opa_lo=lo, opa_hi=hi)
    return out


def stack_lower_bound(nodes, verts, ro, rd, t):
    """nodes [N,16] float32, verts [n,9] float32 (for the margin), rays ro, rd [m,3] with no direction component of magnitude in
    (0, 1e-18) (where the kernel's clamp of 1 / d would make its slab distances smaller than the exact ones), t [m] the final
    closest-hit distance (inf: a miss).  Returns int64 [m]: entries that are surely on the ray's traversal stack at once."""
    bmin, bmax, valid, link = decode(nodes)
    raw = np.ascontiguousarray(nodes, np.float32).view(np.uint32)
    quant = np.stack([(raw[:, 10 + a][:, None] >> (8 * np.arange(4))) & 255 for a in range(6)], axis=-1)      # [N, 4, 6]
    ro = np.asarray(ro, np.float64); rd = np.asarray(rd, np.float64); t = np.asarray(t, np.float64)
    m = len(ro)
    extent = float(np.abs(verts).max()) if len(verts) else 1.0
    margin = (MARGIN * (np.abs(ro).max(axis=1) + 2.0 * extent))[:, None]
    early = 1.0 - 2.0 ** -20          # keys keep all but two low bits of t_near: a sure order needs a few ulps between the two
    depth = np.zeros(m, np.int64)
    ray = np.arange(m)
    node = np.zeros(m, np.int64)
    while len(ray):
        sure = np.zeros((len(ray), 4), bool)
        t_sure = np.full((len(ray), 4), np.inf)         # latest possible entry (shrunk box)
        t_soon = np.full((len(ray), 4), np.inf)         # earliest possible entry (inflated box), inf: surely not entered
        for k in range(4):
            v = valid[node, k]
            lo_s, hi_s = bmin[node, k] + margin[ray], bmax[node, k] - margin[ray]
            tn, tf = _slabs(lo_s, hi_s, ro[ray], rd[ray], False)
            sure[:, k] = v & (lo_s <= hi_s).all(axis=1) & (np.maximum(tn, 0.0) <= tf) & (tn < t[ray])
            t_sure[:, k] = np.where(sure[:, k], tn, np.inf)
            tn, tf = _slabs(bmin[node, k] - margin[ray], bmax[node, k] + margin[ray], ro[ray], rd[ray], False)
            t_soon[:, k] = np.where(v & (np.maximum(tn, 0.0) <= tf), tn, np.inf)
        q = quant[node]                                  # [r, 4, 6] box bytes: equal rows give bit-identical t_near
        pushed = np.zeros(len(ray), np.int64)
        nearest = np.full(len(ray), -1)
        for k in range(4):
            others = [j for j in range(4) if j != k]
            # surely pushed: another child surely entered, surely earlier
            before = np.zeros(len(ray), bool)
            for j in others:
                same = (q[:, j] == q[:, k]).all(axis=1)
                before |= sure[:, j] & (((t_sure[:, j] < t_soon[:, k] * early) & (t_soon[:, k] > 0.0)) | (same & (j < k)))
            pushed += sure[:, k] & before
            # surely the nearest: entered, and every other child either surely not entered or surely entered later
            first = sure[:, k].copy()
            for j in others:
                same = (q[:, j] == q[:, k]).all(axis=1)
                first &= (t_soon[:, j] == np.inf) | ((t_sure[:, k] < t_soon[:, j] * early) & (t_soon[:, j] > 0.0)) | (same & (k < j))
            nearest = np.where(first, k, nearest)
        depth[ray] += pushed
        has = nearest >= 0
        nxt = link[node[has], nearest[has]]
        inner = nxt >= 0
        ray, node = ray[has][inner], nxt[inner].astype(np.int64)
    return depth



def closest_stack_lower_bound(nodes, verts, points):
    """nodes [N,16] float32, verts [n,9] float32 (for the margin), finite points [m,3] queried WITHOUT a radius.  Returns int64 [m]:
    entries that are surely in the point's column of closest_kernel's stack at once, on its first descent."""
    bmin, bmax, _, link = decode(nodes)
    child = link != NODE_EXIT                                                      # [N, 4]
    p = np.asarray(points, np.float64).reshape(-1, 3)
    m = len(p)
    extent = float(np.abs(verts).max()) if len(verts) else 1.0
    margin = (MARGIN * (np.abs(p).max(axis=1) + 2.0 * extent))[:, None]
    early = 1.0 - 2.0 ** -20
    depth = np.zeros(m, np.int64)
    pt = np.arange(m)
    node = np.zeros(m, np.int64)
    while len(pt):
        q, mg, c = p[pt][:, None, :], margin[pt][:, None, :], child[node]
        lo, hi = bmin[node], bmax[node]                                            # [r, 4, 3]
        inside = c & ((lo + mg <= q) & (q <= hi - mg)).all(axis=2)
        late = np.sqrt((np.maximum(np.maximum((lo + mg) - q, q - (hi - mg)), 0.0) ** 2).sum(axis=2))      # to the shrunk box
        soon = np.sqrt((np.maximum(np.maximum((lo - mg) - q, q - (hi + mg)), 0.0) ** 2).sum(axis=2))      # to the inflated box
        depth[pt] += c.sum(axis=1) - 1
        nearest = np.full(len(pt), -1)
        for k in range(4):
            by_slot = inside[:, k].copy()
            by_dist = c[:, k].copy()
            for j in range(4):
                if j != k:
                    by_slot &= ~c[:, j] | (soon[:, j] > 0.0) | (j > k)
                    by_dist &= ~c[:, j] | ((late[:, k] < soon[:, j] * early) & (soon[:, j] > 0.0))
            nearest = np.where(by_slot | by_dist, k, nearest)
        has = nearest >= 0
        nxt = link[node[has], nearest[has]]
        inner = nxt >= 0
        pt, node = pt[has][inner], nxt[inner].astype(np.int64)
    return depth
