"""numpy model of the library's face order (csrc/k_kdorder.hip upper levels, csrc/k_bvh.hip refine_order_kernel): a CHECKER of the
contract the two kernels state in their comments, and a REFERENCE order built by the same rules (tests/test_order_model.py proves
with it that the checker is not vacuous).

A node of capacity `cap` (a power of two) is the aligned range [j cap, (j + 1) cap) of positions, cut to [0, F).  From the top capacity
down to 2 * LEAF_T every node that holds more than cap / 2 faces is cut in the middle of its capacity along the longest axis of its
centroid box:
  cap > 2048 (k_kdorder.hip): the lower half holds the cap / 2 smallest keys, a key being the order-preserving uint of the float32
                              centroid coordinate (-0.0 < +0.0);
  cap <= 2048 (LDS pass):     the same with keys quantised to 2^21 steps of the node's extent.
Which of several EQUAL keys go below is decided by curve positions the model does not know: any choice passes.
With option bvh_window = W the top nodes are windows of the curve order: the upper levels only permute inside them (check_windows)."""
import numpy as np

LEAF_T = 16          # csrc/k_bvh.hip MVS_LEAF_T
LDS_WINDOW = 2048    # csrc/k_bvh.hip RW: the LDS pass; above it csrc/k_kdorder.hip
_Q = np.float32(2097151.0)
_THIRD = np.float32(1.0) / np.float32(3.0)


def centroids(verts, faces):
    """(v0 + v1 + v2) * (1.0f / 3.0f) in float32, in that order (kd_centroid_kernel, refine_order_kernel)"""
    v = np.ascontiguousarray(verts, dtype=np.float32)
    f = np.asarray(faces).astype(np.int64)
    return ((v[f[:, 0]] + v[f[:, 1]] + v[f[:, 2]]) * _THIRD).astype(np.float32)


def f2ord(x):
    """kd_f2ord: order-preserving float32 -> uint32"""
    u = np.ascontiguousarray(x, dtype=np.float32).view(np.uint32)
    return np.where(u & np.uint32(0x80000000), ~u, u | np.uint32(0x80000000)).astype(np.uint32)


def top_capacity(F, window):
    """capacity of the top nodes for option bvh_window = `window` (0: the whole mesh, 1: no upper levels) -- kd_refine_order"""
    if window == 1 or F <= LDS_WINDOW:
        return LDS_WINDOW
    cap = LDS_WINDOW
    while cap < F and (window == 0 or cap < window):
        cap *= 2
    return cap


def node_axis(c):
    """(axis, lo, extent) of a node's centroids: float32 extents, the first axis wins unless a later one is STRICTLY larger"""
    lo, hi = c.min(axis=0), c.max(axis=0)
    ext = (hi - lo).astype(np.float32)
    ax = 0
    if ext[1] > ext[ax]:
        ax = 1
    if ext[2] > ext[ax]:
        ax = 2
    return ax, lo[ax], ext[ax]


def node_keys(c, cap, axis=None):
    """the keys a node of capacity `cap` is cut by, as int64: (keys, axis)"""
    ax, lo, best = node_axis(c)
    if axis is not None:
        ax = axis
        lo = c[:, ax].min(); best = np.float32(c[:, ax].max() - lo)
    if cap > LDS_WINDOW:
        return f2ord(c[:, ax]).astype(np.int64), ax
    if not best > 0:
        return np.zeros(len(c), np.int64), ax
    with np.errstate(over="ignore", invalid="ignore"):
        q = ((c[:, ax] - lo).astype(np.float32) / best * _Q).astype(np.float32)
    return np.minimum(q.astype(np.int64), 0x1FFFFE), ax


def level_capacities(F, window):
    cap, out = top_capacity(F, window), []
    while cap >= 2 * LEAF_T:
        out.append(cap); cap //= 2
    return out


def expected_counts(F, window):
    """what check_order must count for F faces: a matter of F and the window alone"""
    r = dict(levels=0, upper_levels=0, cut=0, uncut=0, upper_cut=0, upper_uncut=0)
    for cap in level_capacities(F, window):
        n = np.minimum(cap, F - np.arange(0, F, cap))
        cut, uncut = int((n > cap // 2).sum()), int((n <= cap // 2).sum())
        r["levels"] += 1; r["cut"] += cut; r["uncut"] += uncut
        if cap > LDS_WINDOW:
            r["upper_levels"] += 1; r["upper_cut"] += cut; r["upper_uncut"] += uncut
    return r


def check_order(verts, faces, perm, window):
    """Checks perm (perm[p] = the caller's face at position p) against the contract for option bvh_window = `window`.
    Returns a dict: violations (list of strings, empty = the order is what the kernels say it is), levels / upper_levels checked,
    nodes cut / uncut (upper_cut / upper_uncut: those above the LDS window), ties / upper_ties = cut nodes whose lower maximum
    equals their upper minimum, tie_caps = the capacities such nodes have."""
    F = len(faces)
    perm = np.asarray(perm).astype(np.int64)
    rep = dict(violations=[], levels=0, upper_levels=0, cut=0, uncut=0, upper_cut=0, upper_uncut=0, ties=0, upper_ties=0, tie_caps=set())
    if len(perm) != F or not np.array_equal(np.sort(perm), np.arange(F)):
        rep["violations"].append("not a permutation of the faces")
        return rep
    c = centroids(verts, faces)[perm]
    for cap in level_capacities(F, window):
        upper = cap > LDS_WINDOW
        rep["levels"] += 1; rep["upper_levels"] += int(upper)
        half = cap // 2
        for start in range(0, F, cap):
            n = min(cap, F - start)
            if n <= half:                       # left uncut: nothing of it may sit above the middle -- true of any aligned range
                rep["uncut"] += 1; rep["upper_uncut"] += int(upper)
                continue
            rep["cut"] += 1; rep["upper_cut"] += int(upper)
            keys, ax = node_keys(c[start:start + n], cap)
            lo_max, hi_min = keys[:half].max(), keys[half:].min()
            if lo_max > hi_min:
                rep["violations"].append("node [%d, %d) of capacity %d, axis %d: %d keys of the lower half exceed the upper half's minimum"
                                         % (start, start + n, cap, ax, int((keys[:half] > hi_min).sum())))
            elif lo_max == hi_min:
                rep["ties"] += 1; rep["upper_ties"] += int(upper); rep["tie_caps"].add(cap)
    return rep


def check_windows(perm, perm_plain, F, window):
    """The upper levels only permute inside the top nodes: every aligned window of top_capacity(F, window) positions holds the same
    SET of faces as the same positions of the order without upper levels (option bvh_window = 1).  Returns the violations."""
    cap = top_capacity(F, window)
    a, b = np.asarray(perm).astype(np.int64), np.asarray(perm_plain).astype(np.int64)
    out = []
    for start in range(0, F, cap):
        if not np.array_equal(np.sort(a[start:start + cap]), np.sort(b[start:start + cap])):
            out.append("window [%d, %d): other faces than the order without upper levels has there" % (start, min(start + cap, F)))
    return out


def reference_order(verts, faces, window, start_order=None, axis_override=None, rank_shift=None):
    """The order the rules give, cut recursively from `start_order` (default: the identity; the library starts from its curve order).
    Equal keys are ranked by their position in the node.  Two deliberate faults for tests of the checker:
    axis_override = (cap, start): that node is cut along its SECOND longest axis;
    rank_shift = (cap, start): that node's elements of rank cap / 2 - 1 and cap / 2 change sides (a pivot off by one rank)."""
    F = len(faces)
    order = np.arange(F, dtype=np.int64) if start_order is None else np.asarray(start_order).astype(np.int64).copy()
    c_all = centroids(verts, faces)
    for cap in level_capacities(F, window):
        half = cap // 2
        for start in range(0, F, cap):
            n = min(cap, F - start)
            if n <= half:
                continue
            seg = order[start:start + n]
            c = c_all[seg]
            axis = None
            if axis_override == (cap, start):
                ext = (c.max(axis=0) - c.min(axis=0)).astype(np.float32)
                axis = int(np.argsort(-ext, kind="stable")[1])
            keys, _ = node_keys(c, cap, axis)
            rank = np.argsort(keys, kind="stable")
            if rank_shift == (cap, start):
                rank[[half - 1, half]] = rank[[half, half - 1]]
            if cap > LDS_WINDOW:     # which elements go below is the contract; the order inside a half is the next level's business
                below = np.zeros(n, bool); below[rank[:half]] = True
                order[start:start + n] = np.concatenate([seg[below], seg[~below]])
            else:
                order[start:start + n] = seg[rank]
    return order.astype(np.uint32)
