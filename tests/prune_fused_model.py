"""Plain numpy restatement of the fused dense prune (nearest_rows + prune_fused in routing_prune.hip).

The rules, for a graph given as a dense latency matrix W (W[x, y]: the smallest latency of an arc
x -> y in ns, INF where there is none; the diagonal is INF, self-loops are no arcs here):

  NN[x]   the `table` smallest (latency, index) out-arcs of x, ascending.
  S1(u)   the arcs (u, v) that no 2-hop detour u -> x -> v over the `first` nearest x = NN[u][:first]
          beats strictly; a detour node no nearer than the arc is skipped (it cannot beat it).
  d2[y]   min(W[u, y], min over x in S1(u), (y, l) in NN[x], y != u, of W[u, x] + l).
  (u, v), v in S1(u), falls iff some y in NN[v], y != u, y != v, with an arc y -> v has
          d2[y] + W[y, v] < W[u, v], strictly.

Sums follow the kernels: a two-term sum that reaches 2^32 - 1 (the u32 +inf mark) or wraps is no
detour; the three-term sum is formed in 64 bits.  Every compared detour is a walk of real arcs with
their own latencies, so an arc whose latency equals the shortest-path latency between its ends
(a tight arc) is never dropped."""
import numpy as np

INF = np.uint64(0xFFFFFFFF)   # kLat32Inf: no arc / no walk


def dense_matrix(el):
    """EdgeList -> W (uint64 [n, n]): parallel arcs folded to the smallest latency, an undirected
    edge both ways, self-loops left out."""
    n = el.n_nodes
    s, d, lat = np.asarray(el.src, np.int64), np.asarray(el.dst, np.int64), np.asarray(el.latency_ns, np.uint64)
    arcs = s != d
    s, d, lat = s[arcs], d[arcs], lat[arcs]
    if not el.directed:
        s, d, lat = np.concatenate([s, d]), np.concatenate([d, s]), np.concatenate([lat, lat])
    assert (lat < INF).all()
    W = np.full((n, n), INF, np.uint64)
    np.minimum.at(W, (s, d), lat)
    return W


def nearest_table(W, table=32):
    """(nodes int64 [n, table], -1 where unused; latencies uint64 [n, table], INF where unused)."""
    n = W.shape[0]
    nodes = np.full((n, table), -1, np.int64)
    lats = np.full((n, table), INF, np.uint64)
    for x in range(n):
        order = np.lexsort((np.arange(n), W[x]))   # by latency, ties by index
        order = order[W[x, order] != INF][:table]
        nodes[x, :len(order)] = order
        lats[x, :len(order)] = W[x, order]
    return nodes, lats


def first_batch(W, nodes, lats, first=8):
    """Boolean [n, n]: arc (u, v) is in S1(u)."""
    n = W.shape[0]
    s1 = np.zeros((n, n), bool)
    idx = np.arange(n)
    for u in range(n):
        w = W[u]
        z = np.full(n, INF, np.uint64)
        for j in range(min(first, nodes.shape[1])):
            x, a = nodes[u, j], lats[u, j]
            if x < 0:
                break
            b = W[x]
            t = a + b   # uint64: cannot wrap
            ok = (a < w) & (idx != x) & (b != INF) & (t < INF)
            z = np.where(ok, np.minimum(z, t), z)
        s1[u] = (w != INF) & (w <= z)
    return s1


def fused_prune(W, first=8, table=32):
    """Boolean [n, n]: the arcs the fused prune keeps."""
    n = W.shape[0]
    nodes, lats = nearest_table(W, table)
    s1 = first_batch(W, nodes, lats, first)
    kept = np.zeros((n, n), bool)
    for u in range(n):
        xs = np.nonzero(s1[u])[0]
        d2 = W[u].copy()
        d2[u] = INF
        if len(xs):
            ys = nodes[xs].ravel()
            t = (W[u, xs][:, None] + lats[xs]).ravel()
            ok = (ys >= 0) & (ys != u) & (t < INF)
            np.minimum.at(d2, ys[ok], t[ok])
        for v in xs:
            ys = nodes[v]
            ys = ys[(ys >= 0) & (ys != u) & (ys != v)]
            d, lyv, w = d2[ys], W[ys, v], W[u, v]
            ok = (d != INF) & (lyv != INF)
            kept[u, v] = not (ok & (d + lyv < w)).any()   # uint64 sum of two values below 2^32
    return kept


def tight_arcs(W, table_lat):
    """Boolean [n, n]: arcs whose latency is the shortest-path latency between their ends
    (`table_lat`: the oracle's latency table over all nodes)."""
    return (W != INF) & (W == np.asarray(table_lat, np.uint64))
