"""The seam fixtures (tests/seam_graphs.py) proved on the CPU oracle: each property a GPU test of
tests/test_routing_seam_gpu.py relies on is asserted here, so a change to a generator cannot
silently empty one of them."""
import numpy as np
import pytest

from oracle import corc
from oracle.routing import fold
from tests import seam_graphs as SG


def _oracle(gr, used=None):
    ids, s, d, l, p, directed = gr
    n = len(ids)
    used = np.arange(n, dtype=np.uint32) if used is None else used
    code, lat, loss, _ = corc.routing(n, s, d, l, p, directed, used)
    assert code == "OK"
    return lat, loss


def _arc_loss(gr, a, b):
    _, s, d, _, p, directed = gr
    k = np.flatnonzero(((s == a) & (d == b)) | ((not directed) & (s == b) & (d == a)))
    assert len(k) == 1
    return p[k[0]]


@pytest.mark.parametrize("directed", [False, True])
def test_ladder_row0_distances(directed):
    gr = SG.ladder(2**32 + 1, directed)
    lat, _ = _oracle(gr)
    assert [int(x) for x in lat[0, 2:8]] == [2**32 - 4, 2**32 - 3, 2**32 - 2, 2**32 - 1, 2**32, 2**32 + 1]
    assert int(lat[0, 1]) == 2**31
    assert int(gr[3][SG.LADDER_E01]) == 2**31 and int(gr[3][SG.LADDER_E12]) == 2**31 - 4


@pytest.mark.parametrize("directed", [False, True])
@pytest.mark.parametrize("embed", [None, 5])
@pytest.mark.parametrize("top", SG.TOPS)
def test_ladder_top_is_largest_and_tie_break_at_the_seam(top, directed, embed):
    gr = SG.ladder(top, directed, embed)
    lat, loss = _oracle(gr)
    n = len(gr[0])
    t = SG.ladder_top_node(top)
    off = 0 if embed is None else 119          # ladder node j > 0 is graph node 119 + j when embedded
    T = t + off
    assert n == (8 if embed is None else 127)
    assert int(lat[~np.eye(n, dtype=bool)].max()) == top
    far = int(np.argmax(lat[:, T] * (np.arange(n) != T)))
    assert int(lat[far, T]) == top and (embed is not None or far == 0)
    assert int((lat[~np.eye(n, dtype=bool)] >= SG.SEAM).sum() > 0) == int(top >= SG.SEAM)
    # two routes of one latency from node t-2 to the top node: two 1 ns rungs, or the 2 ns chord
    assert int(lat[far, T]) == int(lat[far, T - 2]) + 2
    rungs = fold(fold(loss[far, T - 2], _arc_loss(gr, T - 2, T - 1)), _arc_loss(gr, T - 1, T))
    chord = fold(loss[far, T - 2], _arc_loss(gr, T - 2, T))
    assert rungs != chord
    assert loss[far, T].view(np.uint32) == min(rungs, chord).view(np.uint32)
    assert (chord < rungs) == (t % 2 == 0)     # both outcomes occur over the four tops


@pytest.mark.parametrize("top", SG.TOPS)
def test_ladder_used_subset_is_narrow(top):
    """Nodes 0 and 1 alone as the used set: their entries are 2^31, while the labels of the unused
    ladder nodes reach ``top``."""
    lat, _ = _oracle(SG.ladder(top, False), np.asarray([1, 0], np.uint32))
    assert int(lat[0, 1]) == int(lat[1, 0]) == 2**31


@pytest.mark.parametrize("top", SG.TOPS)
def test_sink_ladder_row0(top):
    ids, s, d, l, p, directed = SG.sink_ladder(top)
    t = SG.ladder_top_node(top)
    assert directed and not np.any((s == t) & (d != t))                 # no arc leaves the top node
    code, lat, loss, _ = corc.routing(8, s, d, l, p, True, np.arange(8, dtype=np.uint32), rows=(0, 1))
    assert code == "OK"
    assert int(lat[0, 1:].max()) == top == int(lat[0, t])
    # no other sum of a label of row 0 and an arc out of its node reaches the sentinel
    arcs = s != d
    sums = lat[0, s[arcs]] * (s[arcs] != 0) + l[arcs]
    assert int(sums.max()) == top
    chord = fold(loss[0, t - 2], _arc_loss((ids, s, d, l, p, True), t - 2, t))
    rungs = fold(fold(loss[0, t - 2], _arc_loss((ids, s, d, l, p, True), t - 2, t - 1)),
                 _arc_loss((ids, s, d, l, p, True), t - 1, t))
    assert chord != rungs and loss[0, t].view(np.uint32) == min(chord, rungs).view(np.uint32)


@pytest.mark.parametrize("n", [40, 65, 130])
def test_trap_complete_wraps_in_the_prune_only(n):
    gr = SG.trap_complete(n, n)
    _, s, d, l, _, _ = gr
    lat, _ = _oracle(gr)
    c = n - 1
    A = np.zeros((n, n), np.uint64)
    arcs = s != d
    A[s[arcs], d[arcs]] = l[arcs]
    assert int(arcs.sum()) == n * (n - 1)
    assert int(lat[~np.eye(n, dtype=bool)].max()) < 2**32 - 20
    best = np.arange(0, n - 9, 5)
    assert np.array_equal(lat[best, c], A[best, c])                     # their direct arc is the shortest path
    traps = np.arange(n - 9, c)
    for u in best:                                                      # ... and a trap detour wraps below it
        assert np.all((A[u, traps] + A[traps, c]) % np.uint64(2**32) < 16)
        assert np.all(A[u, traps] + A[traps, c] >= 2**32)
    # the arcs that stay after an exact two-hop prune (a detour strictly shorter removes an arc):
    # no label of any row plus such an arc reaches 2^32 - 1, so a narrow build is never flagged
    eye = np.eye(n, dtype=bool)
    S = A[:, :, None] + A[None, :, :]                                   # S[x, y, v] = (x -> y) + (y -> v)
    two = np.where(eye[:, :, None] | eye[None, :, :], np.uint64(2**40), S).min(axis=1)
    kept = (A <= two) & ~eye
    assert not kept[traps, c].any()
    worst = (lat * ~np.eye(n, dtype=bool)).max(axis=0)                  # the largest label each node gets
    assert int((worst[:, None] + A)[kept].max()) < SG.SEAM - 1


@pytest.mark.parametrize("top", SG.TOPS)
def test_guard_ladder_puts_the_guard_on_the_seam(top):
    gr = SG.guard_ladder(top, 9)
    _, s, d, l, _, _ = gr
    n = len(gr[0])
    code, lat, _, _ = corc.routing(n, s, d, l, gr[4], True, np.arange(n, dtype=np.uint32), rows=(0, 41))
    assert code == "OK"
    arcs = s != d
    assert n == 42 and gr[5] and int(arcs.sum()) * 8 >= n * n         # dense: AUTO prunes it
    assert int(l[arcs].max()) == SG.GUARD_ARC == int(l[1])             # the largest arc is (40, 41)
    assert int(np.sort(l[arcs])[-2]) < 2**31                           # ... and the only one to wrap with
    assert not np.any((s == 41) & (d != 41))                           # node 41 is a sink
    guard = 2**32 - 2 - SG.GUARD_ARC
    offd = ~np.eye(n, dtype=bool)[:41]
    assert int(lat[offd].max()) == top == int(lat[:40, 41].max())
    assert int((lat[offd] >= SG.SEAM).sum() > 0) == int(top >= SG.SEAM)
    far = int(np.argmax(lat[:40, 41]))
    assert int(lat[far, 40]) - guard == top - (2**32 - 2)              # at the guard, or 1, 2, 3 above it
    # labels above the guard at nodes that have arcs out (every node but the sink): none at 2^32 - 2,
    # and node 40's alone from there on -- its compare is the only one between the add and the wrap
    above = (lat[:, :41] > guard) & offd[:, :41]
    assert not above[:, :40].any()
    assert int(above[:, 40].sum()) == 0 if top == 2**32 - 2 else int(above[:, 40].sum()) >= 1


@pytest.mark.parametrize("max_arc", [2**32 - 2, 2**32 - 3])
@pytest.mark.parametrize("n", [33, 65, 130, 257])
def test_huge_complete_is_its_direct_arcs(n, max_arc):
    gr = SG.huge_complete(n, max_arc, n)
    _, s, d, l, p, _ = gr
    lat, loss = _oracle(gr)
    arcs = s != d
    assert int(l[arcs].max()) == max_arc and int(l[arcs].min()) >= 2**31
    assert np.array_equal(lat[s[arcs], d[arcs]], l[arcs]) and np.array_equal(lat[d[arcs], s[arcs]], l[arcs])
    assert np.array_equal(loss[s[arcs], d[arcs]].view(np.uint32), (np.float32(1) - (np.float32(1) - p[arcs])).view(np.uint32))   # fold(0, p)
    assert int(arcs.sum()) == n * (n - 1) // 2
    assert int(lat[~np.eye(n, dtype=bool)].max()) < SG.SEAM


@pytest.mark.parametrize("n", [33, 65, 130, 257])
def test_mixed_complete_lands_on_the_seam_and_wraps(n):
    gr = SG.mixed_complete(n, SG.mixed_small_share(n), n)
    _, s, d, l, _, _ = gr
    lat, _ = _oracle(gr)
    offd = lat[~np.eye(n, dtype=bool)]
    assert int(offd.max()) < SG.SEAM
    assert (offd >= 2**32 - 9).mean() >= 0.02
    # arcs into and out of one node whose u32 sum wraps to a small number, and a sum of exactly 2^32 - 1
    A = np.zeros((n, n), np.uint64)
    arcs = s != d
    A[s[arcs], d[arcs]] = l[arcs]
    A[d[arcs], s[arcs]] = l[arcs]
    wraps = exact = 0
    for v in range(n):
        row = np.delete(A[v], v)
        sums = row[:, None] + row[None, :]
        wraps += int(((sums >= 2**32) & (sums % 2**32 < 16)).sum())
        exact += int((sums == SG.SEAM).sum())
    assert wraps > 0 and exact > 0


def test_mixed_complete_130_at_three_percent():
    lat, _ = _oracle(SG.mixed_complete(130, 0.03, 130))
    offd = lat[~np.eye(130, dtype=bool)]
    assert int(offd.max()) < SG.SEAM and (offd >= 2**32 - 9).mean() >= 0.02


@pytest.mark.parametrize("name", SG.LONG_SATURATED)
def test_long_families_pass_bucket_255_from_every_source(name):
    make, delta = SG.LONG_CASES[name]
    gr = make()
    lat, _ = _oracle(gr)
    n = len(gr[0])
    far = (lat * (~np.eye(n, dtype=bool))).max(axis=1) // np.uint64(delta)
    assert int((far <= 255).sum()) == 0, (name, int(far.min()))


def test_long_families_shapes():
    gr = SG.LONG_CASES["broom"][0]()
    deg = np.bincount(np.concatenate([gr[1], gr[2]])[np.concatenate([gr[1] != gr[2]] * 2)])
    assert deg[0] == 101 and deg.max() == 101           # the star centre is a hub (> kHubDeg = 32)
    assert len(SG.LONG_CASES["grid"][0]()[0]) == 600 and len(SG.LONG_CASES["ring"][0]()[0]) == 640
    lat, _ = _oracle(SG.LONG_CASES["long_path"][0]())
    assert int(lat[0].max()) // SG.MS > 1000            # ~1200 buckets of 1 ms end to end
    # ties: some grid entry is reached by two routes of one latency (ms-granular edges)
    g = SG.LONG_CASES["grid"][0]()
    arcs = g[1] != g[2]
    assert np.all(g[3][arcs] % SG.MS == 0) and set(g[3][arcs] // SG.MS) == {1, 2, 3}
