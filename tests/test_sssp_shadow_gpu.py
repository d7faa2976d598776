"""GPU tests of the fire-and-forget dense SSSP (sssp_lds_shadow: label atomics that return nothing,
the frontier read back from the labels).  Every case compares the whole table, latency and loss
bits, with the C restatement (corc.routing), with SHD_SSSP_SHADOW unset (the new sweeps) and 0 (the
returning atomics)."""
import functools

import numpy as np
import pytest

from oracle import corc
from tests.graphs import engine_graph_from_edges

pytestmark = pytest.mark.gpu

AUTO, DELTA = 0, 3


def _complete(n, mode, seed):
    from shadow_amd import synth
    el = synth.complete_graph(n, seed)
    rng = np.random.default_rng(seed)
    arcs = el.src != el.dst
    m = int(arcs.sum())
    if mode == "const":      # every path of k arcs ties in latency: the loss decides
        el.latency_ns[arcs] = np.uint64(5 * synth.MS)
    elif mode == "few":      # three latencies: heavy ties
        el.latency_ns[arcs] = rng.integers(1, 4, size=m).astype(np.uint64) * np.uint64(synth.MS)
    elif mode == "ns":       # ns-granular latencies: distances with wide gaps, many empty buckets
        el.latency_ns[arcs] = rng.integers(1_000, 10_000_000, size=m).astype(np.uint64)
    elif mode == "stray":    # one 1 ns arc: the bucket width is mean / 256, far above the smallest arc
        el.latency_ns[np.flatnonzero(arcs)[int(rng.integers(0, m))]] = np.uint64(1)
    return el


def _oracle(el, used=None, rows=None):
    used = np.arange(el.n_nodes, dtype=np.uint32) if used is None else used
    kw = {} if rows is None else {"rows": rows}
    code, lat, loss, _ = corc.routing(el.n_nodes, el.src, el.dst, el.latency_ns, el.packet_loss, el.directed,
                                      used, **kw)
    assert code == "OK"
    return used, lat, loss


@functools.lru_cache(maxsize=None)
def _complete_case(n, mode):
    el = _complete(n, mode, 23 + n)
    return (el, *_oracle(el))


def _assert_table(t, lat, loss):
    assert np.array_equal(t.lat, lat)
    assert np.array_equal(t.loss.view(np.uint32), loss.view(np.uint32))


def _default_delta(el):
    """The build's bucket width on a pruned dense graph: max(smallest arc, mean arc / 256)."""
    arcs = el.src != el.dst
    lat = el.latency_ns[arcs]
    n_arcs = len(lat) * (1 if el.directed else 2)
    return max(int(lat.min()), int(lat.sum()) // n_arcs // 256)


@pytest.mark.parametrize("n", [2, 3, 33, 64, 65, 255, 256, 257, 777])
@pytest.mark.parametrize("mode", ["rand", "const", "few", "ns"])
@pytest.mark.parametrize("shadow", [None, 0])
@pytest.mark.parametrize("algo", [AUTO, DELTA])
def test_shadow_complete_graphs(engine, knob, n, mode, shadow, algo):
    """One owned node per thread (n <= 256), exactly and just past one ownership round (256, 257),
    several nodes per thread (777).  AUTO: buckets of the smallest arc; DELTA: of 1.5 x the mean
    arc, wider than most distances, so nodes are expanded again and the floor creeps by amin."""
    knob("SSSP_SHADOW", shadow)
    el, used, lat, loss = _complete_case(n, mode)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=algo)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == (2 if algo == AUTO else 3)


@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_delta_above_smallest_arc(engine, knob, shadow):
    knob("SSSP_SHADOW", shadow)
    el, used, lat, loss = _complete_case(97, "stray")
    assert int(el.latency_ns.min()) == 1 and _default_delta(el) > 1
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


@pytest.mark.parametrize("scale", ["3x", "third"])
@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_forced_bucket_width(engine, knob, scale, shadow):
    knob("SSSP_SHADOW", shadow)
    el, used, lat, loss = _complete_case(65, "rand")
    d = _default_delta(el)
    knob("SSSP_DELTA", d * 3 if scale == "3x" else d // 3)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


def _dense_directed(n, seed):
    """Every ordered pair an arc with its own latency (lat(u, v) != lat(v, u)), a second arc on a
    third of the pairs, some shorter than the first, and self-loops."""
    from shadow_amd import synth
    rng = np.random.default_rng(seed)
    s, d = np.nonzero(~np.eye(n, dtype=bool))
    pick = rng.random(len(s)) < 1 / 3
    loops = np.arange(n)
    s = np.concatenate([loops, s, s[pick]]).astype(np.uint32)
    d = np.concatenate([loops, d, d[pick]]).astype(np.uint32)
    lat = rng.integers(1, 301, size=len(s)).astype(np.uint64) * np.uint64(synth.MS)
    loss = rng.uniform(0.0, 0.01, size=len(s)).astype(np.float32)
    return synth.EdgeList(np.arange(n, dtype=np.uint32), s, d, lat, loss, True)


@functools.lru_cache(maxsize=None)
def _directed_case(n):
    el = _dense_directed(n, 300 + n)
    return (el, *_oracle(el))


@pytest.mark.parametrize("n", [40, 97])
@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_dense_directed_asymmetric(engine, knob, n, shadow):
    knob("SSSP_SHADOW", shadow)
    knob("PRUNE_DENSE_BUILD", 1)   # parallel arcs: folded by dense_build
    el, used, lat, loss = _directed_case(n)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_row_range_and_used_subset(engine, knob, shadow):
    knob("SSSP_SHADOW", shadow)
    el = _complete_case(65, "rand")[0]
    g = engine_graph_from_edges(el)
    used, lat, loss = _oracle(el, rows=(17, 41))
    _assert_table(g.compute_shortest_paths(used, engine, algo=AUTO, rows=(17, 41)), lat, loss)
    sub = np.random.default_rng(5).permutation(65)[:40].astype(np.uint32)   # strict, shuffled
    used, lat, loss = _oracle(el, used=sub)
    _assert_table(g.compute_shortest_paths(used, engine, algo=AUTO), lat, loss)


@pytest.mark.parametrize("lo,hi", [(1_400_000_000, 1_430_000_000), (1_440_000_000, 1_500_000_000)])
@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_overflow_falls_to_u64(engine, knob, lo, hi, shadow):
    """Arc latencies near 2^32 / 3 ns on a complete graph of 33 nodes: three-arc sums land just
    below the +inf mark or pass 2^32; a row that meets a label above the guard flags the build for
    the u64 rerun, and the table is the oracle's either way."""
    from shadow_amd import synth
    knob("SSSP_SHADOW", shadow)
    el = synth.complete_graph(33, 3)
    rng = np.random.default_rng(3)
    arcs = el.src != el.dst
    el.latency_ns[arcs] = rng.integers(lo, hi + 1, size=int(arcs.sum())).astype(np.uint64)
    used, lat, loss = _oracle(el)
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    _assert_table(t, lat, loss)


def test_shadow_unreachable_pair(engine, knob):
    from shadow_amd import synth
    from shadow_amd.routing import RoutingPanic
    el = synth.complete_graph(40, 7)
    keep = (el.src == el.dst) | ((el.src != 39) & (el.dst != 39))   # node 39: its self-loop only
    el = synth.EdgeList(el.node_ids, el.src[keep], el.dst[keep], el.latency_ns[keep], el.packet_loss[keep], False)
    used = np.arange(40, dtype=np.uint32)
    g = engine_graph_from_edges(el)
    msgs = []
    for shadow in (None, 0):
        knob("SSSP_SHADOW", shadow)
        with pytest.raises(RoutingPanic) as e:
            g.compute_shortest_paths(used, engine, algo=AUTO)
        assert engine.last_info()["algo_used"] == 2
        msgs.append(str(e.value))
    assert msgs[0] == msgs[1] and "no path from node" in msgs[0]


@pytest.mark.parametrize("group", [4, 8])
@pytest.mark.parametrize("block", [256, 512])
@pytest.mark.parametrize("shadow", [None, 0])
def test_shadow_forced_shapes(engine, knob, group, block, shadow):
    knob("SSSP_SHADOW", shadow)
    knob("SSSP_G", group)
    knob("SSSP_BLOCK", block)
    el, used, lat, loss = _complete_case(257, "ns")
    t = engine_graph_from_edges(el).compute_shortest_paths(used, engine, algo=AUTO)
    _assert_table(t, lat, loss)
    assert engine.last_info()["algo_used"] == 2


def test_shadow_repeated_builds_on_c2(engine, knob):
    """The workload's size: five builds with the new sweeps give one table, the one the returning
    atomics give (the order of the relaxations differs from run to run; the fixed point does not)."""
    from shadow_amd import synth
    el = synth.complete_graph(1000, 1)
    used = np.arange(1000, dtype=np.uint32)
    g = engine_graph_from_edges(el)
    runs = []
    for _ in range(5):
        t = g.compute_shortest_paths(used, engine, algo=AUTO)
        runs.append((t.lat.copy(), t.loss.view(np.uint32).copy()))
    knob("SSSP_SHADOW", 0)
    t = g.compute_shortest_paths(used, engine, algo=AUTO)
    runs.append((t.lat.copy(), t.loss.view(np.uint32).copy()))
    for r in runs[1:]:
        assert np.array_equal(r[0], runs[0][0]) and np.array_equal(r[1], runs[0][1])


def test_shadow_next_hops(engine, knob):
    el, used, lat, loss = _complete_case(65, "rand")
    g = engine_graph_from_edges(el)
    t1, nh1 = g.compute_next_hops(used, engine, algo=AUTO)
    knob("SSSP_SHADOW", 0)
    t0, nh0 = g.compute_next_hops(used, engine, algo=AUTO)
    _assert_table(t1, lat, loss)
    _assert_table(t0, lat, loss)
    assert np.array_equal(nh1, nh0)
