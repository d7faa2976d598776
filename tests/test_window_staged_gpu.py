"""GPU parity of shd_window_close_staged and the two fetch calls (shadow_amd/csrc/window.cpp) against
their twin: the same offers over the same windows through shd_window_close_sockets with
numpy-grouped device arrays -- the path tests/test_window_gpu.py and tests/test_outbound*_gpu.py
hold against the composed oracle.  Every output of every open and close is compared exactly, on
one context under each of the four disciplines and under in-process ranks."""
import ctypes as C

import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S
from tests.test_outbound import MS, bucket

pytestmark = pytest.mark.gpu

RA = 10 * MS
END = S + 10**12
FIRST = S + 10**9
HEADER = 52
WINDOWS = 6


class Net:
    """H hosts, one node each, path latencies of one to four and a half windows, 2 % loss; outbound
    buckets of 125 kB/s (12 ms a full packet, longer than a window: packets stay queued across
    windows) on three hosts of four, inbound buckets on every second host."""

    def __init__(self, H, seed=3):
        from shadow_amd import synth
        rng = np.random.default_rng(seed)
        self.H = H
        self.lat = rng.integers(RA, 45 * MS, (H, H)).astype(np.uint64)
        self.lat[0, min(1, H - 1)] = RA
        self.loss = np.full((H, H), 0.02, np.float32)
        self.host_node = np.arange(H, dtype=np.uint32)
        self.rng0 = synth.host_rng_states(H, 3)
        self.out_b = [None if h % 4 == 3 else bucket(125_000) for h in range(H)]
        self.in_b = [bucket(1_250_000) if h % 2 else None for h in range(H)]


def _rows(bs):
    return [np.array([(0, 0, 0, S)[i] if b is None else b[i] for b in bs], np.uint64) for i in range(4)]


class Parts:
    def __init__(self, eng, net, qdisc):
        from shadow_amd.equeue import EventQueues
        from shadow_amd.inbound import InboundStage
        from shadow_amd.ledger import PacketLedger
        from shadow_amd.outbound import OutboundStage
        from shadow_amd.relay import Relay
        from shadow_amd.rounds import Runahead
        from shadow_amd.window import Window
        H = net.H
        self.eng, self.lo, self.hi = eng, 0, H
        self.relay = Relay(net.host_node, net.rng0, np.zeros(H, np.uint64), net.lat, net.loss, engine=eng)
        self.queues = EventQueues(eng, H)
        self.runahead = Runahead(eng, True, int(net.lat.min()))
        self.ostage = OutboundStage(eng, *_rows(net.out_b), ring_capacity=64, qdisc=qdisc, max_sockets=8)
        self.istage = InboundStage(eng, *_rows(net.in_b), ring_capacity=512)
        self.ledger = PacketLedger(eng)
        self.win = Window(eng, H)


def offers_of(net, qdisc, n_windows=WINDOWS, seed=17):
    """Per window the grouped offers of every host: (off, time, prio, size, payload, dst, pkt, sock).
    Up to five offers per host and window in time order, a tenth local; window 4 has none.  FIFO:
    the host's priority counter; round-robin: the key is the socket; the socket disciplines: the
    counter or 0 (a control packet), and one of three sockets."""
    rng = np.random.default_rng(seed)
    H, counter, out = net.H, np.ones(net.H, np.int64), []
    for k in range(n_windows):
        ws = FIRST + k * RA
        cnt = rng.integers(0, 6, H) * (k != 4)
        off = np.zeros(H + 1, np.uint32)
        off[1:] = np.cumsum(cnt)
        n = int(off[-1])
        host = np.repeat(np.arange(H), cnt)
        t = rng.integers(ws, ws + RA, n)
        t = t[np.lexsort((t, host))].astype(np.uint64)
        first = np.repeat(off[:-1].astype(np.int64), cnt)
        number = counter[host] + (np.arange(n) - first)
        counter += cnt
        sock = rng.choice([11, 22, 2**40 + 33], n).astype(np.uint64)
        if qdisc == "fifo":
            prio = number.astype(np.uint64)
        elif qdisc == "round-robin":
            prio = sock
        else:
            prio = np.where(rng.random(n) < 0.3, 0, number).astype(np.uint64)
        pay = rng.choice([0, 1448, 700], n).astype(np.uint32)
        dst = np.where(rng.random(n) < 0.1, host, rng.integers(0, H, n)).astype(np.uint32)
        pkt = (k * 100_000 + np.arange(n)).astype(np.uint32)
        out.append((off, t, prio, pay + np.uint32(HEADER), pay, dst, pkt, sock))
    return out


def shard(cols, lo, hi):
    """The offers of hosts [lo, hi), offsets from 0."""
    off = cols[0].astype(np.int64)
    a, z = int(off[lo]), int(off[hi])
    return ((off[lo:hi + 1] - a).astype(np.uint32),) + tuple(c[a:z] for c in cols[1:])


def _dev(arr):
    import torch
    d = [torch.from_numpy(np.ascontiguousarray(a).view(a.dtype.str.replace("u", "i"))).cuda() for a in arr]
    torch.cuda.synchronize()
    return d


def staged(cols, k, lo, qdisc, n_threads=3, dup=False):
    """Window k's offers of one context in n_threads shuffled stages; the time base is the window's
    start.  dup: the first stage's first host gets a second run (of count 0) in the last stage."""
    from shadow_amd.outbound import OfferStages
    sockets = qdisc.endswith("sockets")
    st = OfferStages.from_grouped(*cols[:7], time_base=FIRST + k * RA, n_threads=n_threads, first_host=lo,
                                  sock=cols[7] if sockets else None, seed=100 + k)
    if dup:
        src = next(h for h in st.run_host if len(h))
        st = OfferStages(st.run_host[:-1] + [np.r_[st.run_host[-1], src[:1]]],
                         st.run_count[:-1] + [np.r_[st.run_count[-1], np.uint32(0)]], st.offers, st.words)
    return st


def window(p, mode, cols, k, qdisc, end=END, fetch=False, hook=None):
    """One window on one context (or rank): open, close by `mode`, every output as a dict."""
    we = FIRST + (k + 1) * RA
    op = p.win.open(we)
    rec = p.win.records(op)
    if hook:
        hook(p, we, cols)
    if fetch:
        same(vars(p.win.records_host(op)), vars(rec))
    if p.hi == p.lo:   # a rank without hosts: no arrays, no stage
        from shadow_amd.outbound import OfferStages
        cl = p.win.close(*(None,) * 7, 0, we, end) if mode == "arrays" else \
            p.win.close_staged(OfferStages([], [], [], 8), FIRST + k * RA, we, end)
    elif mode == "arrays":
        d = _dev(cols)
        cl = p.win.close(*d[:7], len(cols[1]), we, end, d_sock=d[7] if qdisc.endswith("sockets") else None)
    else:
        st = staged(cols, k, p.lo, qdisc)
        held = st.pinned(p.eng.lib) if k % 2 == 0 else st   # pinned and pageable stages in turn
        try:
            cl = p.win.close_staged(held, FIRST + k * RA, we, end)
        finally:
            held.free()
    ch = p.win.closed(cl)
    if fetch:
        same(vars(p.win.closed_host(cl)), vars(ch))
    st = p.ledger.stats()
    return dict(rec=vars(rec), ch=vars(ch), n_popped=op.n_popped, n_pending=op.n_pending, qnext=op.queue_next_time,
                n_out=op.records.n_out, in_stored=op.records.n_stored, in_next=op.records.next_task_time,
                n_batch=cl.n_batch, n_events=cl.n_events, n_local=cl.n_local, n_stored=cl.n_stored,
                out_next=cl.next_task_time, min_deliver=cl.min_deliver,
                ledger=(st.live_batches, st.live_events, st.entries_held, st.oldest_batch))


def same(a, b, where=""):
    assert a.keys() == b.keys()
    for key in a:
        x, y = a[key], b[key]
        if isinstance(x, dict):
            same(x, y, f"{where}{key}.")
        elif isinstance(x, np.ndarray):
            assert x.dtype == y.dtype and np.array_equal(x, y), where + key
        else:
            assert x == y, (where + key, x, y)


def end_state(p, qdisc):
    hosts = range(p.hi - p.lo)
    return dict(state=[p.ostage.state(h) for h in hosts],
                sockets=[p.ostage.sockets(h) for h in hosts] if qdisc != "fifo" else None)


def _code(fn):
    from shadow_amd._native import ShdError
    try:
        fn()
        return "OK"
    except ShdError as e:
        return e.code


def run_one_context(net, qdisc, mode, all_offers, hooks=None):
    """Every window of all_offers on a fresh engine; hooks: {window: hook(p, we, cols)} run between
    that window's open and its close."""
    from shadow_amd.routing import Engine
    with Engine(0) as eng:
        p = Parts(eng, net, qdisc)
        out = [window(p, mode, cols, k, qdisc, fetch=mode == "staged", hook=(hooks or {}).get(k))
               for k, cols in enumerate(all_offers)]
        return out, end_state(p, qdisc)


@pytest.mark.parametrize("qdisc", ["fifo", "round-robin", "fifo-sockets", "round-robin-sockets"])
def test_twin_runs_one_context(qdisc):
    """40 hosts, six windows, buckets that block: device arrays against three shuffled stages."""
    net = Net(40)
    offers = offers_of(net, qdisc)
    want, want_end = run_one_context(net, qdisc, "arrays", offers)
    assert sum(w["n_batch"] for w in want) > 100 and sum(w["n_out"] for w in want) > 50
    assert max(w["n_stored"] for w in want[1:]) > 20, "no packets queued across windows"
    got, got_end = run_one_context(net, qdisc, "staged", offers)
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"window {k}: ")
    assert got_end == want_end


def test_fetch_calls():
    """records_host / closed_host equal records() / closed() (every twin run above checks that
    too); a short capacity is SHD_ERR_INVALID with the counts and nothing written; before any open
    both are SHD_ERR_STATE."""
    from shadow_amd import _native as N
    from shadow_amd.routing import Engine
    net = Net(40)
    offers = offers_of(net, "fifo", 3)
    with Engine(0) as eng:
        p = Parts(eng, net, "fifo")
        lib, n1, n2 = eng.lib, C.c_uint64(77), C.c_uint64(78)
        assert lib.shd_window_records_host(eng.ctx, None, None, None, None, 0, C.byref(n1)) == 9   # SHD_ERR_STATE
        assert lib.shd_window_sent_host(eng.ctx, None, None, 0, None, None, None, 0, C.byref(n1), C.byref(n2)) == 9
        assert (n1.value, n2.value) == (77, 78)
        for k in range(2):
            window(p, "arrays", offers[k], k, "fifo")
        we = FIRST + 3 * RA   # the third window: records from the first two, a batch and local deliveries
        op = p.win.open(we)
        rec = p.win.records(op)
        n = op.records.n_out
        assert n > 1
        off, pkt = np.full(net.H + 1, 0xAB, np.uint32), np.full(n, 0xAB, np.uint32)
        time, kind = np.full(n, 0xAB, np.uint64), np.full(n, 0xAB, np.uint8)
        st = lib.shd_window_records_host(eng.ctx, N.ptr(off), N.ptr(pkt), N.ptr(time), N.ptr(kind), n - 1, C.byref(n1))
        assert (st, n1.value) == (5, n)   # SHD_ERR_INVALID, the count returned
        assert (off == 0xAB).all() and (pkt == 0xAB).all() and (time == 0xAB).all() and (kind == 0xAB).all()
        assert lib.shd_window_records_host(eng.ctx, None, None, None, None, 0, C.byref(n1)) == 0 and n1.value == n
        same(vars(p.win.records_host(op)), vars(rec))
        d = _dev(offers[2])
        cl = p.win.close(*d[:7], len(offers[2][1]), we, END)
        ch = p.win.closed(cl)
        assert cl.n_batch > 1 and cl.n_local > 1
        sp, ss = np.full(cl.n_batch, 0xAB, np.uint32), np.full(cl.n_batch, 0xAB, np.uint8)
        lo, lp, lt = np.full(net.H + 1, 0xAB, np.uint32), np.full(cl.n_local, 0xAB, np.uint32), np.full(cl.n_local, 0xAB, np.uint64)
        for cap_b, cap_l in ((cl.n_batch - 1, cl.n_local), (cl.n_batch, cl.n_local - 1)):
            st = lib.shd_window_sent_host(eng.ctx, N.ptr(sp), N.ptr(ss), cap_b, N.ptr(lo), N.ptr(lp), N.ptr(lt), cap_l,
                                          C.byref(n1), C.byref(n2))
            assert (st, n1.value, n2.value) == (5, cl.n_batch, cl.n_local)
            assert all((a == 0xAB).all() for a in (sp, ss, lo, lp, lt))
        # a short capacity does not matter for a buffer that is not asked for
        assert lib.shd_window_sent_host(eng.ctx, None, None, 0, N.ptr(lo), N.ptr(lp), N.ptr(lt), cl.n_local, None, None) == 0
        assert np.array_equal(lo, ch.loc_off) and np.array_equal(lp, ch.loc_pkt) and np.array_equal(lt, ch.loc_time)
        assert (sp == 0xAB).all()
        same(vars(p.win.closed_host(cl)), vars(ch))


def test_refused_staging_keeps_the_window_open():
    """Window 2's first close stages a host twice: SHD_ERR_INVALID, the outbound stage as it was;
    a second open is SHD_ERR_STATE, so the window is still open; the corrected close and every
    window after it are the twin's."""
    qdisc = "fifo-sockets"
    net = Net(40)
    offers = offers_of(net, qdisc)
    want, want_end = run_one_context(net, qdisc, "arrays", offers)
    seen = []

    def hook(p, we, cols):
        before = end_state(p, qdisc)
        seen.append(_code(lambda: p.win.close_staged(staged(cols, 2, 0, qdisc, dup=True), FIRST + 2 * RA, we, END)))
        seen.append(_code(lambda: p.win.open(we)))
        seen.append(end_state(p, qdisc) == before)
    got, got_end = run_one_context(net, qdisc, "staged", offers, hooks={2: hook})
    assert seen == ["INVALID", "STATE", True]
    for k, (g, w) in enumerate(zip(got, want)):
        same(g, w, f"window {k}: ")
    assert got_end == want_end


def run_sharded(net, world, mode, all_offers, hooks_at=None, make_hook=None):
    """The windows on `world` in-process ranks, each rank its own hosts' offers (FIFO)."""
    from tests.test_window_sharded_gpu import _run_ranks, _world
    engines, parts = _world(world, net, net.rng0, net.out_b, net.in_b)
    try:
        out = []
        for k, cols in enumerate(all_offers):
            mine = [shard(cols, p.lo, p.hi) for p in parts]
            hooks = [make_hook(i) if hooks_at == k else None for i in range(world)]
            out.append(_run_ranks([lambda i=i: window(parts[i], mode, mine[i], k, "fifo", fetch=mode == "staged",
                                                      hook=hooks[i]) for i in range(world)]))
        return out, [end_state(p, "fifo") for p in parts]
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("world,n_hosts", [(2, 40), (3, 2)])
def test_twin_runs_sharded(world, n_hosts):
    """Two ranks over 40 hosts, and three ranks over two hosts -- the third has none and stages
    nothing (n_stages = 0): each rank's results are those of the sharded device-array run."""
    net = Net(n_hosts)
    offers = offers_of(net, "fifo", 4)
    want, want_end = run_sharded(net, world, "arrays", offers)
    assert sum(r["n_batch"] for w in want for r in w) > 5 and sum(r["n_events"] for w in want for r in w) > 5
    got, got_end = run_sharded(net, world, "staged", offers)
    for k, (g, w) in enumerate(zip(got, want)):
        for rank, (gr, wr) in enumerate(zip(g, w)):
            same(gr, wr, f"window {k} rank {rank}: ")
    assert got_end == want_end


def test_a_refused_rank_refuses_every_close():
    """Window 1: rank 1 stages a host of rank 0.  Its grouping is refused locally and that status is
    its word in the close's agreement: every rank's close returns SHD_ERR_NO_HOST, no rank's
    outbound state has changed, and the corrected close on every rank is the twin's."""
    from shadow_amd.outbound import OfferStages
    net = Net(40)
    offers = offers_of(net, "fifo", 3)
    want, want_end = run_sharded(net, 2, "arrays", offers)
    noted = {}

    def make_hook(rank):
        def hook(p, we, cols):
            st = staged(cols, 1, p.lo, "fifo")
            if rank == 1:
                k = next(i for i, h in enumerate(st.run_host) if len(h))
                hosts = [h.copy() for h in st.run_host]
                hosts[k][0] = 0   # a host of rank 0
                st = OfferStages(hosts, st.run_count, st.offers, st.words)
            before = end_state(p, "fifo")
            code = _code(lambda: p.win.close_staged(st, FIRST + RA, we, END))
            noted[rank] = (code, end_state(p, "fifo") == before)
        return hook
    got, got_end = run_sharded(net, 2, "staged", offers, hooks_at=1, make_hook=make_hook)
    assert noted == {0: ("NO_HOST", True), 1: ("NO_HOST", True)}
    for k, (g, w) in enumerate(zip(got, want)):
        for rank, (gr, wr) in enumerate(zip(g, w)):
            same(gr, wr, f"window {k} rank {rank}: ")
    assert got_end == want_end
