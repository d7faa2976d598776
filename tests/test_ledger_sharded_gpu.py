"""GPU tests of the sharded ledger record (shd_ledger_record_sharded, csrc/ledger.hip): after a
sharded relay round every rank sends each sent packet's (size, id) to the rank that owns its
destination, records what it received as a batch of its own and rewrites its events' ev_pkt, so
that the queues' popped tags index entries the rank holds.  In-process ranks on one GPU (one host
thread per rank, shd_comm_init_local), against the C restatement's relay into persistent queues:
the oracle's tag names the global packet, whose (size, id) every popped event must carry.
Assertions run only after every thread has joined: a failing rank never strands a peer."""
import threading

import numpy as np
import pytest

from oracle import corc

pytestmark = pytest.mark.gpu

ID_XOR = 0x5A5A0F0F
FAR = 2**62
LOW32 = np.uint64(0xFFFFFFFF)


def _run_ranks(fns):
    res, errs = [None] * len(fns), []

    def wrap(i):
        try:
            res[i] = fns[i]()
        except BaseException as e:   # noqa: BLE001 -- reported below
            errs.append(e)
    ts = [threading.Thread(target=wrap, args=(i,)) for i in range(len(fns))]
    for t in ts:
        t.start()
    for t in ts:
        t.join(timeout=300)
    assert not any(t.is_alive() for t in ts), "a rank hung"
    if errs:
        raise errs[0]
    return res


def _dev(a, dt):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()


def _sizes_ids(n, seed):
    rng = np.random.default_rng(seed)
    return (rng.integers(53, 1501, n).astype(np.uint32),
            (np.arange(n, dtype=np.uint32) ^ np.uint32(ID_XOR)).astype(np.uint32))


class Case:
    """Tables, the rounds' global batches with their sizes and ids, and the oracle's answer: the
    statuses per round and everything its queues pop below FAR after the last round."""

    def __init__(self, host_node, lat, loss, rng0, batches, round_ends):
        self.host_node, self.lat, self.loss, self.rng0 = host_node, lat, loss, rng0
        self.H = len(host_node)
        self.batches, self.round_ends = batches, round_ends
        self.sizes, self.ids = zip(*[_sizes_ids(b.n, 700 + k) for k, b in enumerate(batches)])
        oq = corc.EventQueues(self.H)
        orng, onid = rng0.copy(), np.zeros(self.H, np.uint64)
        self.status = []
        for k, (b, we) in enumerate(zip(batches, round_ends)):
            o = corc.relay_round_eq(b.src_off, b.send_time, b.dst_host, b.payload, host_node, lat, loss, orng, onid,
                                    we, FAR, 0, queues=oq, batch_no=k)
            self.status.append(o["status"])
        self.pop = oq.pop(FAR)
        oq.close()


class Rank:
    def __init__(self, eng, case):
        from shadow_amd import dist as D
        from shadow_amd.equeue import EventQueues
        from shadow_amd.ledger import PacketLedger
        self.eng = eng
        self.relay = D.ShardedRelay(eng, case.host_node, case.rng0, np.zeros(case.H, np.uint64), case.lat, case.loss)
        self.lo, self.hi = self.relay.lo, self.relay.hi
        self.queues = EventQueues(eng, case.H) if self.hi > self.lo else None   # a rank without hosts has none
        self.ledger = PacketLedger(eng)
        self.numbers = []   # the batch number each round was recorded under (None: nothing received)

    def arrays(self, case, k):
        """This rank's slice of round k's batch on the device: off, time, dst, payload, size, id, status."""
        import torch
        b = case.batches[k]
        a, e = int(b.src_off[self.lo]), int(b.src_off[self.hi])
        d = [_dev((b.src_off[self.lo:self.hi + 1] - b.src_off[self.lo]).astype(np.uint32), np.int32),
             _dev(b.send_time[a:e], np.int64), _dev(b.dst_host[a:e], np.int32), _dev(b.payload[a:e], np.int32),
             _dev(case.sizes[k][a:e], np.int32), _dev(case.ids[k][a:e], np.int32),
             torch.empty(max(e - a, 1), dtype=torch.uint8, device="cuda")]
        torch.cuda.synchronize()
        return d, e - a

    def round(self, case, k, d, n, local=0, number=None, spoil=None):
        """Sharded round -> record_sharded -> the batch into the queues (nothing pops yet)."""
        we = case.round_ends[k]
        out = self.relay.round_device(d[0], d[1], d[2], d[3], (we, FAR, 0), d[6])
        if spoil is not None:
            spoil(self, out)
        if number is None:
            number = self.ledger.next_batch() if self.queues else 0
        self.ledger.record_sharded(number, d[4] if n else None, d[5] if n else None, d[2] if n else None,
                                   d[6] if n else None, n, out, local)
        self.numbers.append(number if out.n_events else None)
        if self.queues and out.n_events:
            self.queues.advance_device(out, 0)
        return out.n_events

    def pop_all(self):
        """Everything pending: (Popped, sizes, ids) through the ledger's gather."""
        from shadow_amd import dist as D
        if not self.queues:
            return None
        eq = self.queues.advance_device(None, FAR)
        p = self.queues.popped(eq)
        ds, dp = self.ledger.gather_device(eq.tag, eq.n_popped)
        return p, D.d2h(self.eng, ds, eq.n_popped, np.uint32), D.d2h(self.eng, dp, eq.n_popped, np.uint32)


def _engines(world):
    from shadow_amd import dist as D
    from shadow_amd.routing import Engine
    engines = [Engine(0) for _ in range(world)]
    D.comm_init_local(engines)
    return engines


def _check_pops(case, ranks, pops):
    """Every rank's popped events are the oracle's for its hosts, and each carries the (size, id)
    of the global packet the oracle's tag names."""
    op = case.pop
    total = 0
    for r, got in zip(ranks, pops):
        if got is None:
            assert r.hi == r.lo
            continue
        p, size, pkt = got
        a, z = int(op["off"][r.lo]), int(op["off"][r.hi])
        total += z - a
        assert np.array_equal(p.off.astype(np.int64), op["off"][r.lo:r.hi + 1].astype(np.int64) - a)
        assert np.array_equal(p.deliver, op["deliver"][a:z])
        assert np.array_equal(p.src, op["src"][a:z])
        assert np.array_equal(p.seq, op["seq"][a:z])
        rnd = (op["tag"][a:z] >> np.uint64(32)).astype(np.int64)
        glob = (op["tag"][a:z] & LOW32).astype(np.int64)
        want_size, want_id = np.zeros(z - a, np.uint32), np.zeros(z - a, np.uint32)
        for k in range(len(case.batches)):
            m = rnd == k
            want_size[m], want_id[m] = case.sizes[k][glob[m]], case.ids[k][glob[m]]
            # the engine's batch number is the rank's own: the one round k was recorded under
            if m.any():
                assert r.numbers[k] is not None
                assert np.array_equal((p.tag[m] >> np.uint64(32)).astype(np.int64), np.full(m.sum(), r.numbers[k]))
        assert np.array_equal(size, want_size) and np.array_equal(pkt, want_id)
        assert p.n_pending == 0
        st = r.ledger.stats()
        assert (st.live_batches, st.live_events, st.entries_held) == (0, 0, 0)
    assert total == len(op["tag"])


def _run_case(case, world, search=False):
    engines = _engines(world)
    try:
        for e in engines:
            e.set_knob("LEDGER_REMAP_SEARCH", 1 if search else 0)
        ranks = [Rank(e, case) for e in engines]
        received = []
        for k in range(len(case.batches)):
            parts = [r.arrays(case, k) for r in ranks]
            received.append(_run_ranks([lambda r=r, p=p: r.round(case, k, *p) for r, p in zip(ranks, parts)]))
            for r, (d, n) in zip(ranks, parts):
                a = int(case.batches[k].src_off[r.lo])
                assert np.array_equal(d[6].cpu().numpy()[:n], case.status[k][a:a + n])
        stats = [r.ledger.stats() for r in ranks]
        pops = _run_ranks([r.pop_all for r in ranks])
        _check_pops(case, ranks, pops)
        for r in ranks:
            r.next = r.ledger.next_batch() if r.queues else 0
        return ranks, received, stats
    finally:
        for e in engines:
            e.close()


@pytest.fixture(scope="module")
def big_case():
    """4000 hosts on 40 nodes, two rounds of 200,000 sends: the pack spans ~65 workgroups per rank
    and the remap searches slices of about 10^5 entries."""
    from shadow_amd import synth
    H, NN, P = 4000, 40, 200_000
    el = synth.complete_graph(NN, 11)
    used = np.arange(NN, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(NN, el.src, el.dst, el.latency_ns, el.packet_loss, False, used)
    assert code == "OK"
    ws, ra = 10**9, 10**6
    batches = [synth.packet_batch(H, P, ws + k * ra, ws + (k + 1) * ra, seed=820 + k) for k in range(2)]
    return Case(synth.c5_host_nodes(H, NN), lat, loss, synth.host_rng_states(H, 1), batches, [ws + ra, ws + 2 * ra])


@pytest.mark.parametrize("world,search", [(2, False), (3, False), (2, True), (3, True)])
def test_round_trip_against_the_oracle(big_case, world, search):
    """Two rounds recorded before anything pops (two batches live on every rank), then every event
    popped and gathered: (size, id) of the global packet, worlds 2 and 3 (shards 1334 / 1334 / 1332);
    the remap through its inverse table and through the binary search (LEDGER_REMAP_SEARCH)."""
    ranks, received, stats = _run_case(big_case, world, search)
    if world == 3:
        assert [(r.lo, r.hi) for r in ranks] == [(0, 1334), (1334, 2668), (2668, 4000)]
    for k in range(2):
        assert sum(received[k]) == int((big_case.status[k] == 2).sum())
    for r, st, n0, n1 in zip(ranks, stats, *received):
        assert (st.live_batches, st.live_events, st.entries_held, st.oldest_batch) == (2, n0 + n1, n0 + n1, 0)
        assert min(n0, n1) > 50_000


def _edge_case():
    """130 hosts, three ranks (shards of 44, 44, 42), a node per rank.  Rank 0 sends nothing; every
    packet of rank 1 is dropped (its node's loss row is 1.0); rank 2 sends only to the other two
    shards -- it receives nothing -- and its first host's first 65 entries alternate between the
    two destination ranks, across a wave boundary of the ballot count."""
    from shadow_amd import synth
    H = 130
    host_node = np.minimum(np.arange(H) // 44, 2).astype(np.uint32)
    lat = np.full((3, 3), 5 * 10**6, np.uint64) + np.arange(9, dtype=np.uint64).reshape(3, 3) * np.uint64(1000)
    loss = np.array([[0, 0, 0], [1, 1, 1], [0.25, 0.25, 0.25]], np.float32)
    rng = np.random.default_rng(77)
    ws, we = 10**9, 10**9 + 10**6
    per_host = [[] for _ in range(H)]
    for h in range(44, 88):                        # rank 1: anywhere, all dropped
        per_host[h] = [(int(t), int(rng.integers(0, H))) for t in np.sort(rng.integers(ws, we, 7))]
    per_host[88] = [(ws + i, 0 if i % 2 == 0 else 44 + i % 44) for i in range(65)]
    for h in range(89, H):                         # rank 2: to ranks 0 and 1 only
        per_host[h] = [(int(t), int(rng.integers(0, 88))) for t in np.sort(rng.integers(ws, we, 9))]
    off = np.zeros(H + 1, np.uint32)
    off[1:] = np.cumsum([len(x) for x in per_host])
    flat = [x for e in per_host for x in e]
    b = synth.PacketBatch(off, np.array([x[0] for x in flat], np.uint64), np.array([x[1] for x in flat], np.uint32),
                          rng.integers(1, 1449, len(flat)).astype(np.uint32))   # (a packet without payload is never dropped)
    return Case(host_node, lat, loss, synth.host_rng_states(H, 5), [b], [we])


def test_edge_shapes_three_ranks():
    case = _edge_case()
    st = case.status[0]
    b = case.batches[0]
    assert int(b.src_off[44]) == 0                                             # rank 0 sends nothing
    assert (st[:int(b.src_off[88])] == 1).all() and int(b.src_off[88]) > 0    # rank 1: every packet dropped
    assert (b.dst_host[int(b.src_off[88]):] < 88).all()                        # rank 2 receives nothing
    first = np.minimum(b.dst_host[int(b.src_off[88]):][:65] // 44, 2)
    assert first.tolist() == [i % 2 for i in range(65)] and (st[int(b.src_off[88]):][:65] == 2).sum() > 40
    ranks, received, stats = _run_case(case, 3)
    assert received[0][2] == 0 and received[0][0] > 0 and received[0][1] > 0
    assert stats[2].live_batches == 0 and ranks[2].numbers == [None]
    assert ranks[2].next == 0   # it passed no batch to its queues


def test_nine_ranks_the_last_without_hosts():
    """64 hosts on nine ranks: shards of 8, the ninth rank owns no host; two rounds."""
    from shadow_amd import synth
    H, NN = 64, 8
    el = synth.complete_graph(NN, 3)
    code, lat, loss, _ = corc.routing(NN, el.src, el.dst, el.latency_ns, el.packet_loss, False,
                                      np.arange(NN, dtype=np.uint32))
    assert code == "OK"
    ws, ra = 10**9, 10**6
    batches = [synth.packet_batch(H, 3000, ws + k * ra, ws + (k + 1) * ra, seed=40 + k) for k in range(2)]
    case = Case(synth.c5_host_nodes(H, NN), lat, loss, synth.host_rng_states(H, 2), batches, [ws + ra, ws + 2 * ra])
    ranks, received, stats = _run_case(case, 9)
    assert (ranks[8].lo, ranks[8].hi) == (64, 64) and received[0][8] == received[1][8] == 0


def _small_case(n_rounds):
    from shadow_amd import synth
    H, NN = 130, 5
    el = synth.complete_graph(NN, 9)
    code, lat, loss, _ = corc.routing(NN, el.src, el.dst, el.latency_ns, el.packet_loss, False,
                                      np.arange(NN, dtype=np.uint32))
    assert code == "OK"
    ws, ra = 10**9, 10**6
    batches = [synth.packet_batch(H, 5000, ws + k * ra, ws + (k + 1) * ra, seed=60 + k) for k in range(n_rounds)]
    return Case(synth.c5_host_nodes(H, NN), lat, loss, synth.host_rng_states(H, 4), batches,
                [ws + (k + 1) * ra for k in range(n_rounds)])


def _status_of(fn):
    """The call's outcome as a status name (None: it returned)."""
    from shadow_amd._native import ShdError
    try:
        fn()
        return None
    except ShdError as e:
        return e.code


def _tuple(s):
    return (s.live_batches, s.live_events, s.entries_held, s.oldest_batch)


@pytest.mark.parametrize("what", ["local", "batch_number"])
def test_failure_is_global(what):
    """One rank fails -- its caller's own status (SHD_ERR_HIP carried in), or a batch number not
    above the last one it recorded: both ranks return that status, both ledgers are as they were,
    and the next record works.  The failed record's round had committed, so its events are gone
    with it: the oracle's pops are compared for the other two rounds only."""
    case = _small_case(3)
    engines = _engines(2)
    try:
        ranks = [Rank(e, case) for e in engines]
        parts = [r.arrays(case, 0) for r in ranks]
        _run_ranks([lambda r=r, p=p: r.round(case, 0, *p) for r, p in zip(ranks, parts)])
        before = [_tuple(r.ledger.stats()) for r in ranks]
        assert all(b[0] == 1 for b in before)
        parts = [r.arrays(case, 1) for r in ranks]
        kw = [dict(), dict(local=6)   # SHD_ERR_HIP
              if what == "local" else dict(number=0)]
        got = _run_ranks([lambda r=r, p=p, k=k: _status_of(lambda: r.round(case, 1, *p, **k))
                          for r, p, k in zip(ranks, parts, kw)])
        want = "HIP" if what == "local" else "INVALID"
        assert got == [want, want]
        assert [_tuple(r.ledger.stats()) for r in ranks] == before
        parts = [r.arrays(case, 2) for r in ranks]
        n2 = _run_ranks([lambda r=r, p=p: r.round(case, 2, *p) for r, p in zip(ranks, parts)])
        after = [_tuple(r.ledger.stats()) for r in ranks]
        for b, a, n in zip(before, after, n2):
            assert n > 0 and a == (2, b[1] + n, b[2] + n, 0)
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("search", [False, True])
def test_corrupted_index_kills_that_rank_alone(search):
    """Rank 1's ev_pkt[0] overwritten with an index its sender never sent: that rank's record is
    SHD_ERR_INVALID, the event's ev_pkt UINT32_MAX, its ledger SHD_ERR_STATE until the next setup;
    rank 0's record succeeded and its pops carry the right sizes and ids."""
    import torch
    from shadow_amd import dist as D
    case = _small_case(1)
    engines = _engines(2)
    try:
        for e in engines:
            e.set_knob("LEDGER_REMAP_SEARCH", 1 if search else 0)
        ranks = [Rank(e, case) for e in engines]
        parts = [r.arrays(case, 0) for r in ranks]
        seen = {}

        def spoil(r, out):
            # the round's ev_pkt copied into an array of the test's own, entry 0 past every batch
            pk = D.d2h(r.eng, out.ev_pkt, out.n_events, np.uint32)
            pk[0] = 0x7FFFFFF0
            seen["pkt"] = _dev(pk, np.int32)
            torch.cuda.synchronize()
            out.ev_pkt = seen["pkt"].data_ptr()
        got = _run_ranks([lambda: _status_of(lambda: ranks[0].round(case, 0, *parts[0])),
                          lambda: _status_of(lambda: ranks[1].round(case, 0, *parts[1], spoil=spoil))])
        assert got == [None, "INVALID"]
        torch.cuda.synchronize()
        left = seen["pkt"].cpu().numpy().view(np.uint32)
        assert left[0] == 2**32 - 1 and (left[1:] < len(left)).all()
        st = _status_of(ranks[1].ledger.stats)
        assert st == "STATE"
        p, size, pkt = ranks[0].pop_all()
        op = case.pop
        z = int(op["off"][ranks[0].hi])
        glob = (op["tag"][:z] & LOW32).astype(np.int64)
        assert np.array_equal(p.seq, op["seq"][:z])
        assert np.array_equal(size, case.sizes[0][glob]) and np.array_equal(pkt, case.ids[0][glob])
    finally:
        for e in engines:
            e.close()
