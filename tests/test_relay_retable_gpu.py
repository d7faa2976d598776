"""shd_relay_retable on the GPU: the relay takes a new table and keeps its hosts' RNG streams, event
ids and path counters -- rounds before and after against the C restatement carrying the same state
across; the revival of a relay that a resident routing run stopped; the refusals; the runahead;
and the two-call window with the network switched (update + resident run + retable) half way."""
import numpy as np
import pytest

from oracle import corc
from oracle.token_bucket import SIM_START as S
from tests.test_outbound_gpu import HEADER, ChainOracle, chain_case
from tests.test_window_gpu import Parts, run_windows

pytestmark = pytest.mark.gpu
MS = 1_000_000
H, NN = 64, 60   # chain_case()'s shape: 64 hosts on 60 nodes


def tables(seed, lo_ms=60, hi_ms=70, loss=0.02):
    rng = np.random.default_rng(seed)
    return (rng.integers(lo_ms * MS, hi_ms * MS, (NN, NN)).astype(np.uint64),
            rng.uniform(0, loss, (NN, NN)).astype(np.float32))


def batch(seed, start, n=3000):
    from shadow_amd import synth
    return synth.packet_batch(H, n, start, start + 10 * MS, seed=seed)


def same_round(r, o):
    assert np.array_equal(r.status, o["status"])
    assert np.array_equal(r.ev_off, o["events"]["off"])
    for k in ("deliver", "src", "seq", "pkt"):
        assert np.array_equal(getattr(r, "ev_" + k), o["events"][k]), k
    assert (r.min_deliver, r.min_latency, r.n_sent) == (o["min_deliver"], o["min_latency"], o["n_sent"])


def counts_of(b, status, host_node):
    src = np.repeat(np.arange(H), np.diff(b.src_off.astype(np.int64)))
    sent = status == 2
    c = np.zeros((NN, NN), np.uint64)
    np.add.at(c, (host_node[src[sent]], host_node[b.dst_host[sent]]), 1)
    return c


def test_caller_tables_keep_the_hosts_state():
    """Round 1 on table A, retable to B, round 2 on B with the RNG streams and event ids the oracle
    carried over; the path counters are the sum of both rounds.  Then a B with one latency beyond
    u32 (the 64-bit pipeline) and back to A (the bins again)."""
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.routing import Engine
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(1), tables(2, 20, 45, 0.3)
    wide = (B[0].copy(), B[1])
    wide[0][7, 9] = np.uint64(2**32 + 5)
    orng, onid = rng0.copy(), np.zeros(H, np.uint64)
    with Engine(0) as eng:
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), *A, engine=eng)
        total = np.zeros((NN, NN), np.uint64)
        start = 10**9
        for k, (tab, pipe) in enumerate(((A, 7), (B, 7), (wide, 1), (A, 7))):
            if k:
                rl.retable(*tab)
            b = batch(40 + k, start)
            end = start + 10 * MS
            o = corc.relay_round(b.src_off, b.send_time, b.dst_host, b.payload, host_node, tab[0], tab[1], orng, onid,
                                 end, 10**12, 0)
            r = rl.round(b.src_off, b.send_time, b.dst_host, b.payload, end, 10**12, 0)
            same_round(r, o)
            assert rl.last_pipeline() == pipe, k
            st, nid = rl.host_state()
            assert np.array_equal(st, orng) and np.array_equal(nid, onid)
            total += counts_of(b, o["status"], host_node)
            assert np.array_equal(rl.packet_counts(), total)
            start = end
        assert total.sum() > 8000


def graph_tables():
    """A 60-node complete graph (edges of 60-70 ms, the chain's path latencies) and an update of
    every edge (40-50 ms, other losses): the two networks of the resident-table tests, with the
    oracle's table of each."""
    from shadow_amd import synth
    el = synth.complete_graph(NN, 21)
    rng = np.random.default_rng(22)
    E = len(el.src)
    el.latency_ns = rng.integers(60_000, 70_000, E).astype(np.uint64) * np.uint64(1000)
    l2 = rng.integers(40_000, 50_000, E).astype(np.uint64) * np.uint64(1000)
    p2 = rng.uniform(0, 0.05, E).astype(np.float32)
    used = np.arange(NN, dtype=np.uint32)
    tabs = []
    for l, p in ((el.latency_ns, el.packet_loss), (l2, p2)):
        code, lat, loss, _ = corc.routing(NN, el.src, el.dst, l, p, False, used)
        assert code == "OK"
        tabs.append((lat, loss))
    return el, used, (np.arange(E, dtype=np.uint32), l2, p2), tabs


def test_resident_table_revival():
    """A relay on the resident table stops at the next resident run, as before; retable() revives
    it on the rebuilt table with its state kept."""
    from shadow_amd import synth
    from shadow_amd._native import ShdError
    from shadow_amd.relay import Relay
    from shadow_amd.routing import Engine
    from tests.graphs import engine_graph_from_edges
    el, used, upd, (A, B) = graph_tables()
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    orng, onid = rng0.copy(), np.zeros(H, np.uint64)
    with Engine(0) as eng:
        pg = engine_graph_from_edges(el).prepare(used, eng)
        pg.run_resident()
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), engine=eng)
        assert rl.n_nodes == NN
        b = batch(50, 10**9)
        end = 10**9 + 10 * MS
        o = corc.relay_round(b.src_off, b.send_time, b.dst_host, b.payload, host_node, *A, orng, onid, end, 10**12, 0)
        same_round(rl.round(b.src_off, b.send_time, b.dst_host, b.payload, end, 10**12, 0), o)
        pg.update_edges(*upd)
        b2 = batch(51, end)
        # the update alone leaves the resident table and the relay on it as they were
        o = corc.relay_round(b2.src_off, b2.send_time, b2.dst_host, b2.payload, host_node, *A, orng, onid,
                             end + 10 * MS, 10**12, 0)
        same_round(rl.round(b2.src_off, b2.send_time, b2.dst_host, b2.payload, end + 10 * MS, 10**12, 0), o)
        pg.run_resident()
        with pytest.raises(ShdError, match="STATE"):
            rl.round(b2.src_off, b2.send_time, b2.dst_host, b2.payload, end + 20 * MS, 10**12, 0)
        rl.retable()
        b3 = batch(52, end + 10 * MS)
        o = corc.relay_round(b3.src_off, b3.send_time, b3.dst_host, b3.payload, host_node, *B, orng, onid,
                             end + 20 * MS, 10**12, 0)
        same_round(rl.round(b3.src_off, b3.send_time, b3.dst_host, b3.payload, end + 20 * MS, 10**12, 0), o)
        st, nid = rl.host_state()
        assert np.array_equal(st, orng) and np.array_equal(nid, onid)


def test_refusals():
    import ctypes as C

    from shadow_amd import _native as N
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.routing import Engine
    from tests.graphs import engine_graph_from_edges
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(3), tables(4)
    with Engine(0) as eng:
        lib, ctx = eng.lib, eng.ctx
        name = lambda st: N.STATUS_NAMES[st]  # noqa: E731
        assert name(lib.shd_relay_retable(ctx, NN, N.ptr(B[0]), N.ptr(B[1]))) == "STATE"   # no setup
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), *A, engine=eng)
        small = tables(5)[0][:NN - 1, :NN - 1].copy(), tables(5)[1][:NN - 1, :NN - 1].copy()
        assert name(lib.shd_relay_retable(ctx, NN - 1, N.ptr(small[0]), N.ptr(small[1]))) == "INVALID"
        assert name(lib.shd_relay_retable(ctx, NN, N.ptr(B[0]), None)) == "INVALID"
        assert name(lib.shd_relay_retable(ctx, NN, None, N.ptr(B[1]))) == "INVALID"
        assert name(lib.shd_relay_retable(ctx, NN, None, None)) == "STATE"   # no resident table at all
        # a resident table of a row range is no table for a relay
        el, used, _, _ = graph_tables()
        g = engine_graph_from_edges(el)._cgraph()
        err = N.Error()
        N.check(lib.shd_routing_build(ctx, C.byref(g), N.ptr(used), NN, N.ROUTE_SHORTEST, N.ALGO_AUTO, 0, NN // 2,
                                      None, None, C.byref(err)), "shd_routing_build", err)
        assert name(lib.shd_relay_retable(ctx, NN, None, None)) == "STATE"
        # after every refusal the relay still runs, on its old table
        b = batch(60, 10**9)
        end = 10**9 + 10 * MS
        o = corc.relay_round(b.src_off, b.send_time, b.dst_host, b.payload, host_node, *A, rng0.copy(),
                             np.zeros(H, np.uint64), end, 10**12, 0)
        same_round(rl.round(b.src_off, b.send_time, b.dst_host, b.payload, end, 10**12, 0), o)


def test_zero_latency_table_under_the_runahead():
    """With the runahead set up, a table whose smallest latency is 0 is refused (Runahead::new
    asserts a non-zero minimum): the relay goes on with its old table and the runahead stays."""
    from shadow_amd import _native as N
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead
    from shadow_amd.routing import Engine
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(10), tables(11)
    B[0][3, 4] = 0
    with Engine(0) as eng:
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), *A, engine=eng)
        rl.retable(*B)   # no runahead: as shd_relay_setup, which takes such a table
        rl.retable(*A)
        ra = Runahead(eng, True, int(A[0].min()))
        st = eng.lib.shd_relay_retable(eng.ctx, NN, N.ptr(B[0]), N.ptr(B[1]))
        assert N.STATUS_NAMES[st] == "INVALID"
        assert ra.get() == int(A[0].min())
        b = batch(61, 10**9)
        end = 10**9 + 10 * MS
        o = corc.relay_round(b.src_off, b.send_time, b.dst_host, b.payload, host_node, *A, rng0.copy(),
                             np.zeros(H, np.uint64), end, 10**12, 0)
        same_round(rl.round(b.src_off, b.send_time, b.dst_host, b.payload, end, 10**12, 0), o)


def test_a_new_communicator_needs_a_new_setup():
    """The relay's shard and exchange buffers follow the communicator: a relay set up before the
    communicator was created is not revived by retable()."""
    from shadow_amd import _native as N
    from shadow_amd import dist as D
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.routing import Engine
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(12), tables(13)
    engines = [Engine(0), Engine(0)]
    try:
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), *A, engine=engines[0])
        rl.retable(*B)
        D.comm_init_local(engines)
        st = engines[0].lib.shd_relay_retable(engines[0].ctx, NN, N.ptr(A[0]), N.ptr(A[1]))
        assert N.STATUS_NAMES[st] == "STATE"
        rels = [D.ShardedRelay(e, host_node, rng0, np.zeros(H, np.uint64), *A) for e in engines]
        for r in rels:
            r.retable(*B)
    finally:
        for e in engines:
            e.close()


def test_relay_and_runahead_setup_leave_the_prepared_graph():
    """The table reductions of shd_relay_setup / shd_runahead_setup write a word of their own: a
    build from the same prepared graph afterwards (the dense prune reads the arcs' losses) still
    gives the graph's table."""
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead
    from shadow_amd.routing import Engine
    from tests.graphs import engine_graph_from_edges
    el, used, _, (A, _) = graph_tables()
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    with Engine(0) as eng:
        pg = engine_graph_from_edges(el).prepare(used, eng)
        pg.run_resident()
        Relay(host_node, rng0, np.zeros(H, np.uint64), engine=eng)
        Runahead(eng, True, int(A[0].min()))
        t = pg.run()
        assert np.array_equal(t.lat, A[0]) and np.array_equal(t.loss.view(np.uint32), A[1].view(np.uint32))


def test_runahead_follows_the_table_and_keeps_the_pending_output():
    """A round's output is pending (no device queues: the next window counts it once).  After the
    retable the runahead is the new table's smallest latency -- the lowest latency used on the old
    network is forgotten -- and the window still starts at the pending output's earliest deliver
    time."""
    from oracle.relay import RunaheadState, next_window
    from shadow_amd import synth
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead
    from shadow_amd.rounds import next_window as eng_window
    from shadow_amd.routing import Engine
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(6), tables(7, 80, 95)
    with Engine(0) as eng:
        rl = Relay(host_node, rng0, np.zeros(H, np.uint64), *A, engine=eng)
        ra = Runahead(eng, True, int(A[0].min()))
        ora = RunaheadState(True, int(A[0].min()))
        b = batch(70, 10**9)
        end = 10**9 + 10 * MS
        r = rl.round(b.src_off, b.send_time, b.dst_host, b.payload, end, 10**12, 0)
        ora.update_lowest_used_latency(r.min_latency)
        assert r.n_sent and ra.get() == ora.get() == r.min_latency < int(B[0].min())
        rl.retable(*B)
        ora = RunaheadState(True, int(B[0].min()))   # what the manager would build from the new RoutingInfo
        assert ra.get() == ora.get() == int(B[0].min())
        want = next_window(r.min_deliver, ora.get(), 10**12)
        assert eng_window(eng, None, 10**12) == want and want[0] == r.min_deliver
        # the next round's latencies count again
        b2 = batch(71, end)
        r2 = rl.round(b2.src_off, b2.send_time, b2.dst_host, b2.payload, end + 10 * MS, 10**12, 0)
        ora.update_lowest_used_latency(r2.min_latency)
        assert ra.get() == ora.get() == r2.min_latency


def test_two_ranks_retable():
    """Two in-process ranks, each its shard of the hosts: every rank retables (no collective), and
    the next sharded round runs on the new table with each rank's streams and ids carried on."""
    from shadow_amd import dist as D
    from shadow_amd import synth
    from shadow_amd.routing import Engine
    from tests.test_comm_gpu import _check_rank, _run_ranks, _slice_batch
    host_node, rng0 = synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1)
    A, B = tables(8), tables(9, 20, 45, 0.3)
    engines = [Engine(0), Engine(0)]
    try:
        D.comm_init_local(engines)
        rels = [D.ShardedRelay(e, host_node, rng0, np.zeros(H, np.uint64), *A) for e in engines]
        orng, onid = rng0.copy(), np.zeros(H, np.uint64)
        start = 10**9
        for k, tab in enumerate((A, B)):
            if k:
                for r in rels:
                    r.retable(*tab)
            b = batch(90 + k, start)
            end = start + 10 * MS
            o = corc.relay_round(b.src_off, b.send_time, b.dst_host, b.payload, host_node, *tab, orng, onid, end,
                                 10**12, 0)
            parts = [_slice_batch(b, r.lo, r.hi) for r in rels]
            outs = _run_ranks([lambda r=r, p=p: r.round(*p[:4], (end, 10**12, 0)) for r, p in zip(rels, parts)])
            bases = np.array([p[4] for p in parts], np.int64)
            for r, out in zip(rels, outs):
                _check_rank(out, o, r.lo, r.hi, lambda src: bases[(src >= rels[1].lo).astype(np.int64)], b)
                st, nid = r.host_state()
                assert np.array_equal(st[r.lo:r.hi], orng[r.lo:r.hi])
                assert np.array_equal(nid[r.lo:r.hi], onid[r.lo:r.hi])
            start = end
    finally:
        for e in engines:
            e.close()


class SwitchOracle(ChainOracle):
    """The chain's oracle on a network that changes: the tables are the routing tables of a graph,
    and switch() puts the second network's in place -- with the runahead a manager would build
    from the new RoutingInfo."""

    def __init__(self, end_time):
        super().__init__(end_time)
        from oracle.relay import RunaheadState
        self.el, self.used, self.upd, self.tabs = graph_tables()
        self.lat, self.loss = self.tabs[0]
        self.ra = RunaheadState(True, int(self.lat.min()))

    def switch(self):
        from oracle.relay import RunaheadState
        self.lat, self.loss = self.tabs[1]
        self.ra = RunaheadState(True, int(self.lat.min()))


def switch_offers(k, ws, we, n_hosts, prio):
    """Every host offers a few packets in each of the first five windows (a tenth local)."""
    rng = np.random.default_rng(80 + k)
    per_host, pid = [], k * 100_000
    for h in range(n_hosts):
        n = int(rng.integers(1, 5)) if k < 5 else 0
        offers = []
        for i, t in enumerate(np.sort(rng.integers(ws, we, n)).tolist()):
            dst = h if rng.random() < 0.1 else int(rng.integers(0, n_hosts))
            pay = int(rng.choice([0, 1448, int(rng.integers(1, 1449))]))
            offers.append((t, prio[h] + i, pay + HEADER, pay, dst, pid + i))
        prio[h] += n
        pid += n
        per_host.append(offers)
    return per_host


def test_window_with_the_network_switched_half_way():
    """Six windows through open and close; after the third close the network changes: on the
    engine every edge is updated, the table rebuilt into the resident table and adopted by the
    relay, between that close and the next open.  Everything test_chain_through_open_and_close
    compares, in every window."""
    from shadow_amd.routing import Engine
    from tests.graphs import engine_graph_from_edges
    from tests.test_inbound_gpu import _same_state as _same_in_state
    from tests.test_outbound_gpu import _same_state
    o = SwitchOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    prio = [0] * o.H
    with Engine(0) as eng:
        pg = engine_graph_from_edges(o.el).prepare(o.used, eng)
        p = Parts(eng, o, rng0, out_b, in_b)

        def offers(k, ws, we):
            if k == 3:
                o.switch()
                pg.update_edges(*o.upd)
                pg.run_resident()
                p.relay.retable()
                assert p.runahead.get() == o.ra.get() == int(o.tabs[1][0].min())
            return switch_offers(k, ws, we, o.H, prio)
        run_windows(p, o, offers, 6, (S + 10**9, S + 10**9 + o.ra.get()))
        assert len(o.batches) >= 5 and sum(len(b[1]) for b in o.batches) > 150
        for h in range(o.H):
            _same_state(p.ostage.state(h), o.om.hosts[h])
            _same_in_state(p.istage.state(h), o.im.hosts[h])
