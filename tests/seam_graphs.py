"""Graph generators for the routing tests at the u32 latency seam and past the delta-stepping
bucket range (numpy only, no engine).  Every generator returns the tuple random_graph does,
(node_ids, src, dst, lat u64, loss f32, directed), gives every node one self-loop (the diagonal
of the table) and is deterministic by its arguments.

The narrow engines keep a label as ``lat32 << 32 | loss bits`` with 2^32 - 1 as "unreached", so a
path latency of 2^32 - 2 is the last narrow one, 2^32 - 1 collides with the sentinel and 2^32
wraps; the wide (u64) engine takes over from 2^32 - 1."""
import numpy as np

from tests.graphs import random_graph

SEAM = 2**32 - 1                 # kLat32Inf: the first latency that leaves the narrow engines
TOPS = (2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1)
MS = 1_000_000
LADDER_E01, LADDER_E12, LADDER_E23 = 0, 1, 2   # positions of edges (0, 1), (1, 2), (2, 3) in a ladder's edge arrays


def _finish(n, src, dst, lat, loss, directed, loop_lat=None):
    """Append the self-loops and type the arrays."""
    src, dst, lat, loss = list(src), list(dst), list(lat), list(loss)
    for v in range(n):
        src.append(v); dst.append(v)
        lat.append(1000 + v if loop_lat is None else int(loop_lat[v])); loss.append(0.0)
    return (np.arange(n, dtype=np.uint32), np.asarray(src, np.uint32), np.asarray(dst, np.uint32),
            np.asarray(lat, np.uint64), np.asarray(loss, np.float32), bool(directed))


def ladder_top_node(top):
    assert top in TOPS
    return top - 2**32 + 6       # dist(0, j) = 2^32 - 6 + j for j >= 2


def _closure(n, s, d, l, directed):
    """All-pairs latencies of a small graph (min-plus Floyd-Warshall in float64-exact integers)."""
    D = np.full((n, n), np.iinfo(np.int64).max // 4, np.int64)
    np.fill_diagonal(D, 0)
    for a, b, w in zip(s, d, l):
        if a == b:
            continue
        D[a, b] = min(D[a, b], int(w))
        if not directed:
            D[b, a] = min(D[b, a], int(w))
    for k in range(n):
        D = np.minimum(D, D[:, k:k + 1] + D[k:k + 1, :])
    return D


def sink_ladder(top):
    """The directed ladder without its back arcs: the top node has no arc out, so nothing is ever
    added to its label.  Every narrow engine flags a build as soon as *any* sum it forms leaves
    u32, useful or not -- on the two-way ladders the top node's own arcs do that at 2^32 - 2
    already -- so this is the graph on which a narrow kernel itself writes the entry 2^32 - 2, and
    on which only the test of the sum against the sentinel (2^32 - 1) or for a wrap (2^32,
    2^32 + 1) sends the build to the u64 engine.  Only node 0 reaches every node: build row 0
    (``used`` in index order, rows = (0, 1))."""
    ids, s, d, l, p, _ = ladder(top, True)
    arcs = np.flatnonzero(s != d)
    keep = np.concatenate([arcs[:len(arcs) // 2], np.flatnonzero(s == d)])   # forward arcs, self-loops
    return ids, s[keep], d[keep], l[keep], p[keep], True


def trap_complete(n, seed):
    """Directed complete graph on which a prune site that trusts a wrapped u32 detour sum drops
    arcs the table needs, while no sum over a kept arc leaves u32 (so no wide rerun repairs it).
    Node c = n - 1 is reached by one long arc from every node: 2^32 - 53 .. 2^32 - 50 from every
    fifth node (their direct arc is their shortest path to c), 2^32 - 40 .. 2^32 - 32 from the
    others, and 2^32 - 2 from the eight traps n - 9 .. n - 2.  Arcs into a trap are 2 ns (the
    traps are everyone's nearest detours), all others 3 to 6 ns.  Detour u -> trap -> c sums to
    2^32 exactly: it wraps to 0, 'shorter' than every arc.  The traps' own arcs to c are pruned
    for good reason (any two-arc route is shorter), so the SSSP never adds to them."""
    rng = np.random.default_rng(seed)
    c = n - 1
    a, b = np.nonzero(~np.eye(n, dtype=bool))
    trap_b = (b >= n - 9) & (b < c)
    trap_a = (a >= n - 9) & (a < c)
    lat = np.where(trap_b, 2, rng.integers(3, 7, size=len(a))).astype(np.uint64)
    to_c = b == c
    far = 2**32 - 40 + rng.integers(0, 9, size=len(a))
    best = 2**32 - 53 + rng.integers(0, 4, size=len(a))
    lat = np.where(to_c, np.where(trap_a, 2**32 - 2, np.where(a % 5 == 0, best, far)), lat).astype(np.uint64)
    loss = rng.uniform(0, 0.3, size=len(a)).astype(np.float32)
    o = rng.permutation(len(a))
    return _finish(n, a[o], b[o], lat[o], loss[o], True)


def ladder(top, directed, embed_seed=None):
    """Eight ladder nodes 0..7.  Edge (0, 1) = 2^31, edge (1, 2) = 2^31 - 4, then 1 ns rungs up to
    the top node t = ladder_top_node(top), so dist(0, j) = 2^32 - 6 + j for 2 <= j <= t and the
    largest distance of the graph, dist(0, t), is exactly ``top``.  The nodes past t are not cut
    off (the table needs every pair reachable): they hang off node 1 by 1 ns edges, nearer to
    everything than node 0 is.  A chord (t - 2, t) of 2 ns is the second route to the top node: the
    same latency as the two rungs, another loss (the chord wins for even t, the rungs for odd t).
    directed: every edge is two arcs of one latency with their own losses.
    embed_seed: node 0 is also node 0 of a random_graph of 120 nodes (the ladder's other nodes
    become 120..126) and edge (0, 1) is shortened by that graph's eccentricity of node 0 (directed:
    arc 0 -> 1 by the largest distance towards node 0, its back arc by the largest away from it),
    so the largest distance of the whole graph is still exactly ``top``, between the top node and
    the node farthest from node 0."""
    t = ladder_top_node(top)
    e = [(0, 1, 2**31, 0.011), (1, 2, 2**31 - 4, 0.023)]
    e += [(j, j + 1, 1, 0.03 + 0.01 * j) for j in range(2, t)]
    e += [(t - 2, t, 2, 0.02 if t % 2 == 0 else 0.2)]
    e += [(1, j, 1, 0.005 * j) for j in range(t + 1, 8)]
    src = [a for a, _, _, _ in e]; dst = [b for _, b, _, _ in e]
    lat = [w for _, _, w, _ in e]; loss = [p for _, _, _, p in e]
    if directed:   # the back arcs: same latency, their own (distinct) losses
        src, dst = src + dst, dst + src[:len(e)]
        lat = lat + lat
        loss = loss + [p + 0.004 for p in loss]
    if embed_seed is None:
        return _finish(8, src, dst, lat, loss, directed)
    rng = np.random.default_rng(embed_seed)
    n0 = 120
    _, s0, d0, l0, p0, _ = random_graph(rng, n0, 0.2, directed, max_ms=6, self_loops=False)
    D = _closure(n0, s0, d0, l0, directed)
    ecc_in, ecc_out = int(D[:, 0].max()), int(D[0].max())   # towards node 0, and away from it
    m = lambda v: 0 if v == 0 else n0 - 1 + v   # noqa: E731  ladder node -> graph node
    # (arc 0 -> 1 carries the paths into the ladder, its back arc the paths out of it)
    lat = [w if w != 2**31 else w - (ecc_in if a == 0 else ecc_out) for a, w in zip(src, lat)] + [int(w) for w in l0]
    src = [m(v) for v in src] + [int(v) for v in s0]
    dst = [m(v) for v in dst] + [int(v) for v in d0]
    loss = loss + [float(p) for p in p0]
    return _finish(n0 + 7, src, dst, lat, loss, directed)


GUARD_ARC = 2**31 + 5


def guard_ladder(top, seed):
    """A dense graph (arcs x 8 >= V^2: the build prunes it and runs the padded-list kernels) on
    which their per-node guard, lat_guard = 2^32 - 2 - largest arc, decides exactly at the seam:
    a directed random_graph of 40 nodes with an arc for every second ordered pair, an arc A from
    its node 0 to node 40, the graph's largest arc B = GUARD_ARC from node 40 to node 41, and a
    1 ms arc from node 40 back to node 0 (so no source reaches node 40 but through A), with A
    chosen so that the source farthest from node 0 reaches node 41 at exactly ``top``.  Its label
    of node 40 is top - B: lat_guard for top = 2^32 - 2, one more for 2^32 - 1 (whose sum is the
    sentinel's own value), and from 2^32 on the unchecked sum wraps to a label of 0 or 1.
    Node 41 is a sink: its label, above the guard at every ``top``, is never added to, so a
    kernel that compares only the nodes whose arcs it relaxes (sssp_lds_shadow on 32-slot lists) keeps the build
    narrow at 2^32 - 2.  No row starts there: build rows (0, 41) of ``used`` in index order."""
    rng = np.random.default_rng(seed)
    n0 = 40
    _, s0, d0, l0, p0, _ = random_graph(rng, n0, 0.5, True, max_ms=6, self_loops=False)
    ecc = int(_closure(n0, s0, d0, l0, True)[:, 0].max())
    src = [0, n0, n0] + [int(v) for v in s0]
    dst = [n0, n0 + 1, 0] + [int(v) for v in d0]
    lat = [top - GUARD_ARC - ecc, GUARD_ARC, MS] + [int(w) for w in l0]
    loss = [0.05, 0.15, 0.02] + [float(p) for p in p0]
    return _finish(n0 + 2, src, dst, lat, loss, True)


def _complete_pairs(n):
    a, b = np.triu_indices(n, 1)
    return a.astype(np.uint32), b.astype(np.uint32)


def huge_complete(n, max_arc, seed):
    """Complete undirected graph, arcs uniform in [2^31, max_arc] with one arc forced to max_arc:
    every two-arc sum is >= 2^32 (it wraps u32 to less than any arc), so the table is the direct
    arcs.  max_arc = 2^32 - 2 switches the padded kernels' guard off; 2^32 - 3 makes it 1."""
    rng = np.random.default_rng(seed)
    a, b = _complete_pairs(n)
    lat = rng.integers(2**31, max_arc + 1, size=len(a), dtype=np.uint64)
    lat[int(rng.integers(len(a)))] = max_arc
    loss = rng.uniform(0, 0.3, size=len(a)).astype(np.float32)
    o = rng.permutation(len(a))
    return _finish(n, a[o], b[o], lat[o], loss[o], False)


def mixed_complete(n, small_share, seed):
    """Complete undirected graph whose arcs are 1..8 ns (a ``small_share`` of them) or
    2^32 - 2 - k with k < 8: a big and a small arc sum to 2^32 - 1 exactly (small = k + 1) or wrap
    to a single digit (small > k + 1), two big ones wrap to just under 2^32 - 4.  The small arcs
    join most nodes at a few ns; the last max(1, n // 40) nodes have big arcs only, so their rows
    and columns stay within 8 ns of the seam, some by a big + small detour that just fits."""
    rng = np.random.default_rng(seed)
    a, b = _complete_pairs(n)
    m = len(a)
    small = (rng.random(m) < small_share) & (b < n - max(1, n // 40))   # (a < b)
    lat = np.where(small, rng.integers(1, 9, size=m, dtype=np.uint64),
                   np.uint64(2**32 - 2) - rng.integers(0, 8, size=m, dtype=np.uint64))
    loss = rng.uniform(0, 0.3, size=m).astype(np.float32)
    o = rng.permutation(m)
    return _finish(n, a[o], b[o], lat[o].astype(np.uint64), loss[o], False)


def mixed_small_share(n):
    """About four small arcs per node at any n (0.03 at n = 130): the small arcs then join most
    nodes, and the few they leave out keep rows of entries just under the seam."""
    return 3.9 / (n - 1)


def _ms_edges(rng, src, dst):
    m = len(src)
    lat = rng.integers(1, 4, size=m).astype(np.uint64) * np.uint64(MS)
    loss = rng.uniform(0, 0.1, size=m).astype(np.float32)
    return list(src), list(dst), [int(x) for x in lat], [float(x) for x in loss]


def long_path(n, seed):
    """Path 0 - 1 - ... - n-1, edges of 1 to 3 ms (integer ms), losses in [0, 0.1]."""
    rng = np.random.default_rng(seed)
    s, d, l, p = _ms_edges(rng, range(n - 1), range(1, n))
    return _finish(n, s, d, l, p, False)


def ring_with_chords(n, chords, seed):
    """Ring of n nodes plus ``chords`` chords that each skip 2 to 8 nodes (local ones, so the ring
    stays hundreds of hops across); 1 to 3 ms edges: a chord ties with or beats the arcs it skips."""
    rng = np.random.default_rng(seed)
    src = list(range(n)); dst = [(v + 1) % n for v in range(n)]
    at = rng.choice(n, size=chords, replace=False)
    for v in at:
        src.append(int(v)); dst.append(int((v + rng.integers(2, 9)) % n))
    s, d, l, p = _ms_edges(rng, src, dst)
    return _finish(n, s, d, l, p, False)


def grid(w, h, seed):
    """w x h grid (node y * w + x), 1 to 3 ms edges: many equal-latency routes to every node."""
    rng = np.random.default_rng(seed)
    src, dst = [], []
    for y in range(h):
        for x in range(w):
            if x + 1 < w:
                src.append(y * w + x); dst.append(y * w + x + 1)
            if y + 1 < h:
                src.append(y * w + x); dst.append((y + 1) * w + x)
    s, d, l, p = _ms_edges(rng, src, dst)
    return _finish(w * h, s, d, l, p, False)


def broom(path_len, leaves, seed):
    """Path 0 - ... - path_len-1 whose node 0 is also the centre of a star of ``leaves`` leaves
    (> kHubDeg = 32: the centre is relaxed by whole waves, the path by lane groups)."""
    rng = np.random.default_rng(seed)
    src = list(range(path_len - 1)) + [0] * leaves
    dst = list(range(1, path_len)) + list(range(path_len, path_len + leaves))
    s, d, l, p = _ms_edges(rng, src, dst)
    return _finish(path_len + leaves, s, d, l, p, False)


# The graphs of the past-the-bucket-range tests and the bucket width each saturates under: with
# labels ordered by min(255, lat / delta), every source row has labels beyond bucket 255.
LONG_DELTA = MS
LONG_CASES = {
    "long_path": (lambda: long_path(600, 1), LONG_DELTA),
    "ring": (lambda: ring_with_chords(640, 20, 2), LONG_DELTA),
    "broom": (lambda: broom(400, 100, 4), LONG_DELTA),
    # a 24 x 25 grid is at most 47 hops of 3 ms across, under 255 buckets of 1 ms from any source:
    # it runs at 1 ms for its ties, and at 50 us (>= 24 hops of >= 1 ms from every source = 480
    # buckets) for the saturation
    "grid": (lambda: grid(24, 25, 3), LONG_DELTA),
    "grid_50us": (lambda: grid(24, 25, 3), 50_000),
}
LONG_SATURATED = ("long_path", "ring", "broom", "grid_50us")
