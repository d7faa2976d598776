"""shd_routing_update_edges on the GPU: after every update the next build must equal, bit for bit,
a fresh shd_routing_build of the modified graph (on a second engine) and the C restatement on the
modified edge arrays -- latencies, loss bits, next hops, arcs and arcs_kept -- on every path the
build can take: the dense CSR as the matrix, dense_build, the LDS kernels on plain and on
wave-spread lists, the locality-ordered copy of the global-label kernel, the blocked engine, the
wide rerun, direct mode and the sharded run."""
import functools

import numpy as np
import pytest

from oracle import corc
from tests.graphs import random_graph

pytestmark = pytest.mark.gpu
ALGOS = [0, 1, 2, 3, 4]
MS = 1_000_000


@pytest.fixture(scope="module")
def fresh():
    """A second engine: the fresh builds of the modified graphs (the first keeps its prepared graph)."""
    from shadow_amd.routing import Engine
    eng = Engine(0)
    yield eng
    eng.close()


class Net:
    def __init__(self, ids, s, d, l, p, directed, used):
        self.ids, self.s, self.d, self.directed = ids, s, d, bool(directed)
        self.l, self.p = np.array(l, np.uint64), np.array(p, np.float32)
        self.used = np.ascontiguousarray(used, np.uint32)
        self.n = len(ids)

    def graph(self, l=None, p=None):
        from shadow_amd.routing import NetworkGraph
        return NetworkGraph(self.ids, self.s, self.d, self.l if l is None else l, self.p if p is None else p,
                            self.directed)


def complete65():
    from shadow_amd import synth
    el = synth.complete_graph(65, 11, tie_frac=0.10)
    return Net(el.node_ids, el.src, el.dst, el.latency_ns, el.packet_loss, False, np.arange(65))


def partial65(directed):
    """The complete graph without 30 % of its edges and with a few parallel ones: not the dense
    matrix any more, so the prune goes through dense_build.  Directed: an arc each way, own draws."""
    from shadow_amd import synth
    el = synth.complete_graph(65, 12, tie_frac=0.10)
    rng = np.random.default_rng(5 + directed)
    s, d, l, p = el.src[65:], el.dst[65:], el.latency_ns[65:], el.packet_loss[65:]
    if directed:
        s, d = np.concatenate([s, d]), np.concatenate([d, s])
        l = np.concatenate([l, rng.integers(1, 301, len(l)).astype(np.uint64) * np.uint64(MS)])
        p = np.concatenate([p, rng.uniform(0, 0.01, len(p)).astype(np.float32)])
    keep = rng.random(len(s)) >= 0.30
    s, d, l, p = s[keep], d[keep], l[keep], p[keep]
    n_kept = len(s)
    par = rng.choice(n_kept, 6, replace=False)   # parallel edges: same ends, own weights, at the end
    s, d = np.concatenate([el.src[:65], s, s[par]]), np.concatenate([el.dst[:65], d, d[par]])
    l = np.concatenate([el.latency_ns[:65], l, l[par] + np.uint64(MS)])
    p = np.concatenate([el.packet_loss[:65], p, p[par]])
    net = Net(el.node_ids, s.astype(np.uint32), d.astype(np.uint32), l, p, directed,
              np.random.default_rng(6).permutation(65)[:60])
    net.parallel = [(65 + int(k), 65 + n_kept + i) for i, k in enumerate(par)]   # (the edge, its later twin)
    return net


def ba(n, n_used=None, seed=2):
    from shadow_amd import synth
    el = synth.barabasi_albert(n, 3, seed)
    used = np.arange(n) if n_used is None else np.random.default_rng(3).permutation(n)[:n_used]
    return Net(el.node_ids, el.src, el.dst, el.latency_ns, el.packet_loss, False, used)


NETS = {"complete65": complete65, "partial65": lambda: partial65(False), "partial65d": lambda: partial65(True),
        "ba300": lambda: ba(300, 200)}


def steps_for(net, name):
    """The update calls of one scenario: (edge_index, latency_ns, packet_loss) each."""
    rng = np.random.default_rng(len(net.s))
    E = len(net.s)
    arcs = np.flatnonzero(net.s != net.d)
    lo, hi = int(net.l[arcs].min()), int(net.l[arcs].max())

    def rand(n):
        return (rng.integers(0, E, n), rng.integers(1, 301, n).astype(np.uint64) * np.uint64(MS),
                rng.uniform(0, 0.02, n).astype(np.float32))
    steps = [rand(0), rand(1)]
    # lowers the graph's smallest arc latency, then raises its largest (the bin shift and the guard follow)
    steps.append((arcs[[3]], [max(lo // 4, 1)], [0.001]))
    steps.append((arcs[[7, 9]], [hi * 4, hi * 3], [0.5, 0.0]))
    # an edge named three times in one call (the last entry counts), among others
    e = int(arcs[11])
    steps.append(([e, int(arcs[12]), e, int(arcs[13]), e], [5 * MS, 6 * MS, 7 * MS, 8 * MS, 2 * MS],
                  [0.1, 0.2, 0.3, 0.4, 0.05]))
    # loss -0.0, 0.0 and 1.0 on arcs of short latency (they are taken)
    steps.append((arcs[[20, 21, 22]], [MS, MS, MS], np.array([-0.0, 0.0, 1.0], np.float32)))
    # a self-loop of a used node and of an unused one (the first n edges are the self-loops)
    used_node = int(net.used[2])
    unused = sorted(set(range(net.n)) - set(net.used.tolist()))
    steps.append(([used_node] + unused[:1], [77_777] * (1 + len(unused[:1])), [0.25] * (1 + len(unused[:1]))))
    if hasattr(net, "parallel"):   # one of two parallel edges: the later one, then the earlier one
        first, second = net.parallel[0]
        steps.append(([second], [1], [0.125]))
        steps.append(([first], [1], [0.0625]))
    for n in (63, 64, 65, 257):
        steps.append(rand(n))
    idx = rng.permutation(E)   # every edge
    steps.append((idx, rng.integers(1, 301, E).astype(np.uint64) * np.uint64(MS),
                  rng.uniform(0, 0.02, E).astype(np.float32)))
    return [(np.asarray(i, np.uint32), np.asarray(l, np.uint64), np.asarray(p, np.float32)) for i, l, p in steps]


@functools.lru_cache(maxsize=None)
def scenario(name):
    """The net, its update calls and, computed once, the C restatement's table after each."""
    net = NETS[name]()
    steps = steps_for(net, name)
    l, p = net.l.copy(), net.p.copy()
    want = []
    for idx, nl, np_ in steps:
        l[idx], p[idx] = nl, np_   # numpy keeps the last of repeated indices
        code, lat, loss, _ = corc.routing(net.n, net.s, net.d, l, p, net.directed, net.used)
        assert code == "OK"
        want.append((l.copy(), p.copy(), lat, loss.view(np.uint32).copy()))
    return net, steps, want


def same_as_fresh(eng, fresh, net, pg, algo, want_lat, want_bits, rows=None, next_hops=False):
    """One build from the updated graph against a fresh shd_routing_build of the modified arrays
    on the second engine, and against the oracle's table."""
    out = pg.run(algo, rows, next_hops=next_hops)
    t = out[0] if next_hops else out
    info = eng.last_info()
    g2 = net.graph(pg.edge_latency_ns, pg.edge_packet_loss)
    t2 = g2.compute_shortest_paths(net.used, fresh, algo=algo, rows=rows)
    info2 = fresh.last_info()
    assert np.array_equal(t.lat, t2.lat) and np.array_equal(t.loss.view(np.uint32), t2.loss.view(np.uint32))
    assert np.array_equal(t.lat, want_lat) and np.array_equal(t.loss.view(np.uint32), want_bits)
    for k in ("arcs", "arcs_kept", "algo_used", "wide_latency"):
        assert info[k] == info2[k], k
    return out


@pytest.mark.parametrize("algo", ALGOS)
@pytest.mark.parametrize("name", list(NETS))
def test_updates_then_builds_equal_fresh_prepares(engine, fresh, name, algo):
    """Every update set of the scenario in turn, a build after each: n = 0, 1, 63, 64, 65, 257 and
    every edge; the smallest latency lowered and the largest raised; an edge named three times;
    loss -0.0, 0.0, 1.0; self-loops of a used and an unused node; one of two parallel edges."""
    net, steps, want = scenario(name)
    pg = net.graph().prepare(net.used, engine)
    again = engine.get_knob("UPDATE_REPREPARES")
    for (idx, l, p), (wl, wp, lat, bits) in zip(steps, want):
        pg.update_edges(idx, l, p)
        assert np.array_equal(pg.edge_latency_ns, wl) and np.array_equal(pg.edge_packet_loss.view(np.uint32),
                                                                         wp.view(np.uint32))
        same_as_fresh(engine, fresh, net, pg, algo, lat, bits)
    assert engine.get_knob("UPDATE_REPREPARES") == again   # every call patched the resident arrays
    if name == "complete65":
        assert engine.last_info()["algo_used"] == (2 if algo in (0, 2) else algo)


def test_next_hops_after_an_update(engine, fresh):
    net, steps, want = scenario("complete65")
    pg = net.graph().prepare(net.used, engine)
    for (idx, l, p), (wl, wp, lat, bits) in list(zip(steps, want))[:5]:
        pg.update_edges(idx, l, p)
    t, nh = same_as_fresh(engine, fresh, net, pg, 0, lat, bits, next_hops=True)
    ref = corc.next_hops(net.n, net.s, net.d, wl, wp, False, net.used, lat, bits.view(np.float32))
    assert np.array_equal(nh, ref)


@functools.lru_cache(maxsize=None)
def ba_rows_case(n, n_used, row_sets):
    """A larger BA graph with three update calls and the oracle's rows after the last."""
    net = ba(n, n_used)
    rng = np.random.default_rng(n)
    E = len(net.s)
    arcs = np.flatnonzero(net.s != net.d)
    steps = [(rng.integers(0, E, 257), rng.integers(100, 50_001, 257).astype(np.uint64) * np.uint64(1000),
              rng.uniform(0, 0.02, 257).astype(np.float32)),
             (arcs[[5, 6]], [50, 400 * MS], [0.0, 0.3]),   # below the smallest, above the largest
             (rng.integers(0, E, 5000), rng.integers(100, 50_001, 5000).astype(np.uint64) * np.uint64(1000),
              rng.uniform(0, 0.02, 5000).astype(np.float32))]
    steps = [(np.asarray(i, np.uint32), np.asarray(l, np.uint64), np.asarray(p, np.float32)) for i, l, p in steps]
    l, p = net.l.copy(), net.p.copy()
    for idx, nl, np_ in steps:
        l[idx], p[idx] = nl, np_
    want = {}
    for rows in row_sets:
        code, lat, loss, _ = corc.routing(net.n, net.s, net.d, l, p, False, net.used, rows=rows)
        assert code == "OK"
        want[rows] = (lat, loss.view(np.uint32).copy())
    return net, steps, want


@pytest.mark.parametrize("spread", [1, 0])
def test_wave_spread_copy_follows(engine, fresh, knob, spread):
    """6,000 nodes: the 1024-thread LDS kernel, on prepare_spread's copy or (SSSP_NO_SPREAD) on the
    main arrays; a used subset in permuted order, the first and the last 64 rows.  The copy made
    at prepare is patched whatever the knob says at update time."""
    rows = ((0, 64), (3936, 4000))
    net, steps, want = ba_rows_case(6000, 4000, rows)
    knob("SSSP_NO_SPREAD", 1 - spread)
    knob("SSSP_NO_SPREAD", 1 - spread, fresh)
    pg = net.graph().prepare(net.used, engine)
    for i, (idx, l, p) in enumerate(steps):
        if spread and i == 1:
            knob("SSSP_NO_SPREAD", 1)   # the copy exists: it must be patched all the same
        pg.update_edges(idx, l, p)
        if spread and i == 1:
            knob("SSSP_NO_SPREAD", 0)
    for r in rows:
        for algo in (0, 1):
            same_as_fresh(engine, fresh, net, pg, algo, *want[r], rows=r)
    if spread:   # and the main arrays were patched too
        knob("SSSP_NO_SPREAD", 1)
        knob("SSSP_NO_SPREAD", 1, fresh)
        same_as_fresh(engine, fresh, net, pg, 0, *want[rows[0]], rows=rows[0])


def test_copies_after_a_wide_excursion(engine, fresh):
    """6,000 nodes: an edge to 5 s and back prepares the graph twice more (wide, then packed again
    with a new wave-spread copy); the update after that must find that copy's slots too."""
    rows = ((0, 64), (3936, 4000))
    net, steps, _ = ba_rows_case(6000, 4000, rows)
    pg = net.graph().prepare(net.used, engine)
    pg.update_edges(*steps[0])
    e = int(np.flatnonzero(net.s != net.d)[9])
    pg.update_edges([e], [5_000_000_000], [0.01])
    pg.update_edges([e], [MS], [0.01])
    pg.update_edges(*steps[2])
    code, lat, loss, _ = corc.routing(net.n, net.s, net.d, pg.edge_latency_ns, pg.edge_packet_loss, False, net.used,
                                      rows=rows[0])
    assert code == "OK"
    same_as_fresh(engine, fresh, net, pg, 0, lat, loss.view(np.uint32), rows=rows[0])
    assert engine.last_info()["wide_latency"] == 0


def test_locality_ordered_copy_follows(engine, fresh, knob):
    """2,000 nodes with SSSP_REORDER=1 and SSSP_GLOBAL=1 before prepare: the global-label kernel on
    prepare_reordered's copy."""
    rows = ((0, 64), (1936, 2000))
    net, steps, want = ba_rows_case(2000, None, rows)
    for e in (engine, fresh):
        knob("SSSP_REORDER", 1, e)
        knob("SSSP_GLOBAL", 1, e)
    pg = net.graph().prepare(net.used, engine)
    for idx, l, p in steps:
        pg.update_edges(idx, l, p)
    for r in rows:
        for algo in (1, 3):
            same_as_fresh(engine, fresh, net, pg, algo, *want[r], rows=r)


@pytest.mark.parametrize("bits", [40, 31])
def test_direct_mode(engine, bits):
    """Direct mode keeps the edges' u64 latencies in d_el / d_ep: latencies up to 2^40 (nearly all of
    them past u32: the patch's high word) and below 2^31 are patched in place -- no call prepares
    the graph again, which the table could not show.  n = 1, 65 and every edge; an edge named
    twice; a self-loop (an edge like any other here); loss -0.0."""
    from shadow_amd import _native as N
    from shadow_amd import synth
    el = synth.complete_graph(64, 9)
    used = np.random.default_rng(1).permutation(64).astype(np.uint32)
    net = Net(el.node_ids, el.src, el.dst, el.latency_ns, el.packet_loss, False, used)
    pg = net.graph().prepare(used, engine, mode=N.ROUTE_DIRECT)
    again = engine.get_knob("UPDATE_REPREPARES")
    rng = np.random.default_rng(2)
    E = len(net.s)
    loop = int(np.flatnonzero(net.s == net.d)[5])
    for n in (1, 65, E):
        idx = rng.integers(0, E, n).astype(np.uint32)
        lat = rng.integers(1, 2**bits, n).astype(np.uint64)
        loss = rng.uniform(0, 1, n).astype(np.float32)
        loss[0] = np.float32(-0.0)
        if n == 65:
            idx[3], idx[40], idx[64] = idx[7], idx[7], loop
        pg.update_edges(idx, lat, loss)
        if bits == 40:
            assert int(pg.edge_latency_ns[net.s != net.d].max()) >= 2**32
        code, wl, wp, _ = corc.routing(64, net.s, net.d, pg.edge_latency_ns, pg.edge_packet_loss, False, used,
                                       shortest=False)
        assert code == "OK"
        t = pg.run()
        assert np.array_equal(t.lat, wl) and np.array_equal(t.loss.view(np.uint32), wp.view(np.uint32))
    assert engine.get_knob("UPDATE_REPREPARES") == again


def test_wide_latency_there_and_back(engine, fresh):
    """One edge to 5 s: an arc beyond u32, the u64 path; back to 1 ms: the packed arcs again.  Then
    every edge between 1 and 4 s: no arc overflows u32 but the paths do, and the build reruns wide."""
    rng = np.random.default_rng(7)
    ids, s, d, l, p, directed = random_graph(rng, 60, 0.05, False)
    net = Net(ids, s, d, l, p, directed, np.arange(60))
    pg = net.graph().prepare(net.used, engine)
    e = int(np.flatnonzero(s != d)[4])
    again = engine.get_knob("UPDATE_REPREPARES")
    for lat_e, wide in ((5_000_000_000, 1), (MS, 0)):
        pg.update_edges([e], [lat_e], [0.01])
        again += 1   # into the wide graph and out of it: prepared again both times
        assert engine.get_knob("UPDATE_REPREPARES") == again
        code, lat, loss, _ = corc.routing(60, s, d, pg.edge_latency_ns, pg.edge_packet_loss, directed, net.used)
        assert code == "OK"
        for algo in (0, 4):
            same_as_fresh(engine, fresh, net, pg, algo, lat, loss.view(np.uint32))
            assert engine.last_info()["wide_latency"] == wide
    E = len(s)
    pg.update_edges(np.arange(E), rng.integers(1000, 4001, E).astype(np.uint64) * np.uint64(MS),
                    rng.uniform(0, 0.3, E).astype(np.float32))
    assert int(pg.edge_latency_ns.max()) < 2**32 - 1
    assert engine.get_knob("UPDATE_REPREPARES") == again   # the arcs fit: patched in place
    code, lat, loss, _ = corc.routing(60, s, d, pg.edge_latency_ns, pg.edge_packet_loss, directed, net.used)
    assert code == "OK" and lat.max() > 2**32
    for algo in (0, 4):
        same_as_fresh(engine, fresh, net, pg, algo, lat, loss.view(np.uint32))
        assert engine.last_info()["wide_latency"] == 1


def test_refusals_leave_the_graph(engine):
    import ctypes as C

    from shadow_amd import _native as N
    from shadow_amd.routing import Engine
    net, steps, want = scenario("ba300")
    E = len(net.s)
    with Engine(0) as e2:   # update before prepare
        one = (np.zeros(1, np.uint32), np.ones(1, np.uint64), np.zeros(1, np.float32))
        st = e2.lib.shd_routing_update_edges(e2.ctx, 1, *(N.ptr(a) for a in one), None)
        assert N.STATUS_NAMES[st] == "STATE"
    pg = net.graph().prepare(net.used, engine)
    pg.update_edges(*steps[1])   # the map exists: a refusal must not leave a half-applied call
    pg.update_edges(*steps[2])
    before = pg.run()
    lib, ctx = engine.lib, engine.ctx

    def call(idx, lat, loss, n=None, null=None):
        a = [np.asarray(idx, np.uint32), np.asarray(lat, np.uint64), np.asarray(loss, np.float32)]
        ptrs = [N.ptr(x) for x in a]
        if null is not None:
            ptrs[null] = None
        err = N.Error()
        return N.STATUS_NAMES[lib.shd_routing_update_edges(ctx, len(a[0]) if n is None else n, *ptrs, C.byref(err))]
    good = (int(np.flatnonzero(net.s != net.d)[0]), 5, 0.5)
    for null in (0, 1, 2):
        assert call([good[0]], [5], [0.5], null=null) == "INVALID"
    bad = [([good[0], E], [5, 5], [0.5, 0.5]),                         # an index past the edges
           ([good[0], good[0] + 1], [5, 0], [0.5, 0.5]),               # latency 0
           ([good[0], good[0] + 1], [5, 5], [0.5, -0.25]),             # loss below 0
           ([good[0], good[0] + 1], [5, 5], [0.5, 1.5]),               # above 1
           ([good[0], good[0] + 1], [5, 5], [0.5, float("nan")])]      # NaN
    for idx, lat, loss in bad:
        assert call(idx, lat, loss) == "INVALID"
        after = pg.run()
        assert np.array_equal(after.lat, before.lat)
        assert np.array_equal(after.loss.view(np.uint32), before.loss.view(np.uint32))
    assert call([], [], [], n=0, null=0) == "OK"
    after = pg.run()
    assert np.array_equal(after.lat, want[2][2]) and np.array_equal(after.loss.view(np.uint32), want[2][3])


def test_sharded_run_equals_the_one_context_table(fresh):
    """Two in-process ranks, the same update on both; rows exchanged (no replication)."""
    import torch

    from shadow_amd import _native as N
    from shadow_amd import dist as D
    from shadow_amd.routing import Engine
    from tests.test_comm_gpu import _run_ranks
    net, steps, want = scenario("ba300")
    n, world = len(net.used), 2
    per = (n + world - 1) // world
    engines = [Engine(0) for _ in range(world)]
    try:
        for e in engines:
            e.set_knob("SHARD_REPLICATE_MB", 0)
        D.comm_init_local(engines)
        pgs = [net.graph().prepare(net.used, e) for e in engines]
        bufs = [(torch.empty((world * per, n), dtype=torch.int64, device="cuda"),
                 torch.empty((world * per, n), dtype=torch.float32, device="cuda")) for _ in engines]
        torch.cuda.synchronize()
        for k in (1, 2, 3, 4):
            for pg in pgs:
                pg.update_edges(*steps[k])
            _run_ranks([lambda e=e, b=b: D.routing_run_sharded(e, N.ALGO_AUTO, b[0], b[1])
                        for e, b in zip(engines, bufs)])
            torch.cuda.synchronize()
            for bl, bp in bufs:
                assert np.array_equal(bl[:n].cpu().numpy().view(np.uint64), want[k][2])
                assert np.array_equal(bp[:n].cpu().numpy().view(np.uint32), want[k][3])
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("which", ["edge01", "rung23"])
def test_ladder_edge_across_the_u32_seam(engine, fresh, which):
    """One edge of the ladder (tests/seam_graphs.py; largest distance 2^32 - 2) to 2^32 - 2, the
    last latency a packed arc holds: patched in place, and the largest arc now switches the padded
    kernels' guard off.  To 2^32 - 1, the narrow labels' sentinel: prepared again, on the u64
    arcs.  Back to 1 ns: prepared again, packed.  Edge (0, 1) carries every long path (the table
    goes past 2^33); the rung (2, 3) drops out of every shortest path, only the arc maximum moves."""
    from tests import seam_graphs as SG
    ids, s, d, l, p, directed = SG.ladder(2**32 - 2, False)
    edge, ends = {"edge01": (SG.LADDER_E01, (0, 1)), "rung23": (SG.LADDER_E23, (2, 3))}[which]
    assert (int(s[edge]), int(d[edge])) == ends
    net = Net(ids, s, d, l, p, directed, np.arange(8))
    pg = net.graph().prepare(net.used, engine)
    again = engine.get_knob("UPDATE_REPREPARES")
    for lat_e, more in ((2**32 - 2, 0), (2**32 - 1, 1), (1, 1)):
        pg.update_edges([edge], [lat_e], [0.07])
        again += more
        assert engine.get_knob("UPDATE_REPREPARES") == again, lat_e
        assert int(pg.edge_latency_ns[s != d].max()) == (lat_e if lat_e > 1 else 2**31 - 4 if edge == 0 else 2**31)
        code, lat, loss, _ = corc.routing(8, s, d, pg.edge_latency_ns, pg.edge_packet_loss, directed, net.used)
        assert code == "OK"
        for algo in (0, 4):
            same_as_fresh(engine, fresh, net, pg, algo, lat, loss.view(np.uint32))
            if int(lat[~np.eye(8, dtype=bool)].max()) >= 2**32 - 1:
                assert engine.last_info()["wide_latency"] == 1


def test_patch_keeps_the_largest_arc_at_the_last_narrow_latency(engine, fresh):
    """huge_complete(65): arcs in [2^31, 2^32 - 2] with the largest exactly 2^32 - 2 (guard off:
    the unpadded kernel on the padded lists).  Patches move that largest arc to another edge and
    rewrite a quarter of the others inside the range: lat_minmax must leave max_arc_lat at
    2^32 - 2, and every build equals a fresh prepare's."""
    from tests import seam_graphs as SG
    ids, s, d, l, p, directed = SG.huge_complete(65, 2**32 - 2, 65)
    net = Net(ids, s, d, l, p, directed, np.arange(65))
    arcs = np.flatnonzero(s != d)
    top = int(arcs[np.argmax(l[arcs])])
    other = int(arcs[0] if arcs[0] != top else arcs[1])
    rng = np.random.default_rng(65)
    some = rng.choice(arcs[(arcs != top) & (arcs != other)], len(arcs) // 4, replace=False)
    steps = [([top, other], [2**31, 2**32 - 2], [0.1, 0.2]),
             (some, rng.integers(2**31, 2**32 - 2, len(some), dtype=np.uint64), rng.uniform(0, 0.3, len(some))),
             ([other, top], [2**32 - 3, 2**32 - 2], [0.2, 0.0])]
    pg = net.graph().prepare(net.used, engine)
    again = engine.get_knob("UPDATE_REPREPARES")
    for idx, nl, np_ in steps:
        pg.update_edges(np.asarray(idx, np.uint32), np.asarray(nl, np.uint64), np.asarray(np_, np.float32))
        assert int(pg.edge_latency_ns[arcs].max()) == 2**32 - 2
        code, lat, loss, _ = corc.routing(65, s, d, pg.edge_latency_ns, pg.edge_packet_loss, directed, net.used)
        assert code == "OK"
        for algo in (0, 2, 4):
            same_as_fresh(engine, fresh, net, pg, algo, lat, loss.view(np.uint32))
    assert engine.get_knob("UPDATE_REPREPARES") == again
