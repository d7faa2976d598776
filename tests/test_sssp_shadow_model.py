"""The sweep rule of the fire-and-forget dense SSSP (tests/sssp_shadow_model.py) against the
oracle's Dijkstra on small dense graphs: exact labels (latency and loss bits) for every source,
whatever the relaxation order, and a sweep count under the cap."""
import functools

import numpy as np
import pytest

from oracle import routing as orc
from oracle.gml import Edge, NetworkGraph
from shadow_amd import synth
from tests.sssp_shadow_model import INF, shadow_sssp, sweep_cap

N = 24


def _graph(src, dst, lat, loss, directed, n):
    edges = [Edge(int(s), int(d), int(l), np.float32(p)) for s, d, l, p in zip(src, dst, lat, loss)]
    return NetworkGraph(directed, list(range(n)), edges, {i: i for i in range(n)})


def _complete(mode, seed):
    el = synth.complete_graph(N, seed)
    rng = np.random.default_rng(seed)
    arcs = el.src != el.dst
    m = int(arcs.sum())
    if mode == "const":     # every path of k arcs ties in latency: the loss decides
        el.latency_ns[arcs] = np.uint64(5 * synth.MS)
    elif mode == "ns":      # ns-granular: distances with wide gaps between them
        el.latency_ns[arcs] = rng.integers(1_000, 10_000_000, size=m).astype(np.uint64)
    elif mode == "stray":   # one 1 ns arc: amin = 1, delta = mean / 256 > amin
        el.latency_ns[np.flatnonzero(arcs)[int(rng.integers(0, m))]] = np.uint64(1)
    return _graph(el.src, el.dst, el.latency_ns, el.packet_loss, False, N)


def _directed(seed):
    """Every ordered pair an arc of its own latency, a second arc on a third of the pairs."""
    rng = np.random.default_rng(seed)
    s, d = np.nonzero(~np.eye(N, dtype=bool))
    pick = rng.random(len(s)) < 1 / 3
    s, d = np.concatenate([np.arange(N), s, s[pick]]), np.concatenate([np.arange(N), d, d[pick]])
    lat = rng.integers(1, 301, size=len(s)).astype(np.uint64) * np.uint64(synth.MS)
    loss = rng.uniform(0.0, 0.01, size=len(s)).astype(np.float32)
    return _graph(s, d, lat, loss, True, N)


@functools.lru_cache(maxsize=None)
def _case(mode, seed):
    g = _directed(seed) if mode == "directed" else _complete(mode, seed)
    adj = orc.adjacency(g)
    lats = [l for u, row in enumerate(adj) for (v, l, _) in row if v != u]
    amin = max(min(lats), 1)
    mean = sum(lats) // len(lats)
    delta = max(amin, mean // 256)   # the build's bucket width on a pruned dense graph
    ref = [orc.dijkstra(adj, s) for s in range(N)]
    return adj, amin, delta, ref


def _check(adj, ref, delta, amin, order, waves):
    worst = 0
    for s in range(N):
        lab, sweeps, capped = shadow_sssp(adj, s, delta, amin, order, waves)
        assert not capped and sweeps < sweep_cap(N), (s, sweeps)
        worst = max(worst, sweeps)
        for v in range(N):
            want = ref[s].get(v)
            if want is None:
                assert lab[v] == INF
            else:
                assert lab[v][0] == want[0], (s, v)
                assert np.float32(lab[v][1]).view(np.uint32) == np.float32(want[1]).view(np.uint32), (s, v)
    return worst


@pytest.mark.parametrize("mode", ["rand", "const", "ns", "stray", "directed"])
@pytest.mark.parametrize("seed", [1, 2])
def test_shadow_sweeps_match_dijkstra(mode, seed):
    adj, amin, delta, ref = _case(mode, seed)
    if mode == "stray":
        assert amin == 1 and delta > amin
    worst = {}
    for name, order, waves in (("fwd", "fwd", 1), ("rev", "rev", 1), ("rev x4", "rev", 4),
                               ("shuffled x4", np.random.default_rng(seed), 4)):
        worst[name] = _check(adj, ref, delta, amin, order, waves)
    print(f"{mode}/{seed}: delta {delta} amin {amin}, most sweeps per row {worst} (cap {sweep_cap(N)})")


@pytest.mark.parametrize("scale", ["3x", "third", "huge"])
def test_shadow_sweeps_other_bucket_widths(scale):
    """A forced bucket width (SHD_SSSP_DELTA): three times and a third of the default, and one
    wider than every distance (ALGO_DELTA's 1.5 x mean on a dense graph comes close): the floor
    then creeps by amin per sweep and the rule must still end, exactly."""
    adj, amin, delta, ref = _case("rand", 1)
    d = {"3x": delta * 3, "third": max(delta // 3, 1), "huge": 10**12}[scale]
    for order, waves in (("fwd", 1), ("rev", 4)):
        _check(adj, ref, d, amin, order, waves)


def test_shadow_sweeps_unreachable_node_stays_inf():
    adj, amin, delta, _ = _case("rand", 2)
    cut = [[(v, l, p) for (v, l, p) in row if v != N - 1] for row in adj[:N - 1]] + [[]]
    lab, sweeps, capped = shadow_sssp(cut, 0, delta, amin, "rev", 2)
    assert not capped and lab[N - 1] == INF and all(lab[v] != INF for v in range(N - 1))
