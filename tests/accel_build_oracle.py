"""numpy restatement of the hierarchy the DEVICE builder makes (rt_set_accel_builder; csrc/rt_accel_build.hip, DESIGN.md
section 36), top-down and recursive where the kernels work bottom-up and without a traversal:

1. the loose list and the tree list by the host's linear pass (non-finite boxes and boxes that span more than largeFraction of
   the scene's extent are loose), the tree objects' box centres and their per-axis range, in double;
2. 30-bit Morton codes of the centres on a 1024^3 grid over that range; the tree objects sorted by (code, object index);
3. leaves of leaf_size consecutive entries, inside a leaf ascending object index; a leaf's key is code << 32 | index of its
   first entry before that re-sort;
4. the binary radix tree over the leaves' keys: a node over leaves [l, r] splits at the highest bit in which K_l and K_r differ;
5. depth-first pre-order, skip = the first node behind the subtree;
6. every box the exact union of the stored boxes below.

build() answers accel_oracle's shape: nodes (layout.ACCEL_NODE_DTYPE), order, loose, info."""
import bisect
import collections

import numpy as np

from opengl_raytracing_amd import layout as L

Structure = collections.namedtuple("Structure", "nodes order loose info")
INNER = L.ACCEL_INNER


def classify(objects, large_fraction=0.5):
    """-> (lo[n,3], hi[n,3] float32 ordered stored boxes, tree, loose: ascending object indices)."""
    a, b = objects["bounds_min"].astype(np.float32).reshape(-1, 3), objects["bounds_max"].astype(np.float32).reshape(-1, 3)
    with np.errstate(invalid="ignore"):
        lo, hi = np.where(a < b, a, b), np.where(a < b, b, a)
        finite = np.isfinite(a).all(-1) & np.isfinite(b).all(-1)
    large = ~finite
    if finite.any():
        dlo, dhi = lo.astype(np.float64), hi.astype(np.float64)
        extent = dhi[finite].max(0) - dlo[finite].min(0)
        with np.errstate(invalid="ignore"):
            large = large | ((dhi - dlo) > np.float64(np.float32(large_fraction)) * extent).any(-1)
    idx = np.arange(len(objects), dtype=np.uint32)
    return lo, hi, idx[~large], idx[large]


def morton_codes(lo, hi, tree):
    """The 30-bit codes of the tree objects' box centres: bit k of x, y, z at bits 3k + 2, 3k + 1, 3k."""
    c = 0.5 * (lo[tree].astype(np.float64) + hi[tree].astype(np.float64))
    cmin, cmax = c.min(0), c.max(0)
    with np.errstate(divide="ignore"):
        scale = np.where(cmax > cmin, 1024.0 / (cmax - cmin), 0.0)
    q = np.minimum(1023, np.floor((c - cmin) * scale).astype(np.int64))
    code = np.zeros(len(tree), np.int64)
    for k in range(10):
        for a in range(3):
            code |= ((q[:, a] >> k) & 1) << (3 * k + 2 - a)
    return code


def build(objects, leaf_size=4, large_fraction=0.5):
    leaf_size, large_fraction = leaf_size or 4, large_fraction or 0.5
    n = len(objects)
    lo, hi, tree, loose = classify(objects, large_fraction)
    empty = Structure(np.zeros(0, L.ACCEL_NODE_DTYPE), np.zeros(0, np.uint32), np.arange(n, dtype=np.uint32),
                      dict(built=False, nodes=0, leaves=0, depth=0, loose=n, bytes=4 * n))
    if len(tree) == 0:
        return empty
    code = morton_codes(lo, hi, tree)
    by = np.lexsort((tree, code))                                  # (code, object index) ascending
    code, entries = code[by], tree[by]
    M = -(-len(tree) // leaf_size)
    K = [(int(code[j * leaf_size]) << 32) | int(entries[j * leaf_size]) for j in range(M)]
    assert all(x < y for x, y in zip(K, K[1:])), "the leaves' keys are strictly increasing"
    order = np.concatenate([np.sort(entries[j * leaf_size:(j + 1) * leaf_size]) for j in range(M)]).astype(np.uint32)
    nodes = np.zeros(2 * M - 1, L.ACCEL_NODE_DTYPE)
    count, depth = 0, 0

    def subtree(l, r, level):
        nonlocal count, depth
        me, count, depth = count, count + 1, max(depth, level)
        if l == r:
            first, cnt = l * leaf_size, min(leaf_size, len(tree) - l * leaf_size)
            ids = order[first:first + cnt]
            nodes["lo"][me], nodes["hi"][me] = lo[ids].min(0), hi[ids].max(0)
            nodes["leaf"][me] = (first << 4) | cnt
        else:
            b = (K[l] ^ K[r]).bit_length() - 1                     # the highest bit in which the two ends differ
            s = bisect.bisect_left(K, ((K[l] >> b) | 1) << b, l, r + 1) - 1      # the last leaf with that bit clear
            assert l <= s < r
            c1 = subtree(l, s, level + 1)
            c2 = subtree(s + 1, r, level + 1)
            nodes["lo"][me], nodes["hi"][me] = np.minimum(nodes["lo"][c1], nodes["lo"][c2]), np.maximum(nodes["hi"][c1], nodes["hi"][c2])
            nodes["leaf"][me] = INNER
        nodes["skip"][me] = count
        return me

    subtree(0, M - 1, 1)
    assert count == 2 * M - 1
    info = dict(built=True, nodes=len(nodes), leaves=M, depth=depth, loose=len(loose), bytes=32 * len(nodes) + 4 * n)
    return Structure(nodes, order, loose.astype(np.uint32), info)


def same_structure(got, want):
    """None when two structures are the same -- skip, leaf, order, loose word for word, the boxes as floats (-0 == +0) -- else
    what differs."""
    for name in ("order", "loose"):
        g, w = getattr(got, name), getattr(want, name)
        if len(g) != len(w) or not (g == w).all():
            return f"{name}[] differs"
    if len(got.nodes) != len(want.nodes):
        return f"{len(got.nodes)} nodes, not {len(want.nodes)}"
    for name in ("skip", "leaf", "lo", "hi"):
        bad = np.flatnonzero((got.nodes[name] != want.nodes[name]).reshape(len(want.nodes), -1).any(-1))
        if len(bad):
            return f"{name} differs on {len(bad)} nodes, first at {int(bad[0])}: {got.nodes[name][bad[0]]} != {want.nodes[name][bad[0]]}"
    return None
