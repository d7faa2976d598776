"""GPU parity of the two-call scheduling window under a communicator of several ranks
(csrc/window.cpp): every rank runs open and close on its shard of the hosts -- in-process ranks on
one GPU, one host thread per rank -- against the composed oracle of tests/test_outbound_gpu.py run
once for all hosts.  A rank's inbound records, sent ids, statuses, local deliveries, stored totals
and task times are the oracle's for its hosts [lo, hi); the pending totals add up; the next window
is the oracle's on every rank.  Assertions run only after every thread has joined."""
import threading

import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S
from tests.outbound_model import IDLE
from tests.test_outbound_gpu import ChainOracle, _arrays, chain_case, chain_offers

pytestmark = pytest.mark.gpu


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


def _rows(bs):
    return [np.array([(0, 0, 0, S)[i] if b is None else b[i] for b in bs], np.uint64) for i in range(4)]


class RankParts:
    """One rank's parts under the communicator: the sharded relay, the queues of its shard, both
    stages for its hi - lo hosts (the outbound stage's first_host = lo), runahead, ledger, window.
    A rank without hosts has neither queues nor stages."""

    def __init__(self, eng, o, rng0, out_b, in_b):
        from shadow_amd import dist as D
        from shadow_amd.equeue import EventQueues
        from shadow_amd.ledger import PacketLedger
        from shadow_amd.rounds import Runahead
        from shadow_amd.window import Window
        self.eng = eng
        self.relay = D.ShardedRelay(eng, o.host_node, rng0, np.zeros(o.H, np.uint64), o.lat, o.loss)
        self.lo, self.hi = self.relay.lo, self.relay.hi
        self.out_b, self.in_b = out_b, in_b
        self.queues = EventQueues(eng, o.H) if self.hi > self.lo else None
        self.runahead = Runahead(eng, True, int(o.lat.min()))
        self.ostage = self.istage = None
        if self.hi > self.lo:
            self.setup_outbound()
            from shadow_amd.inbound import InboundStage
            self.istage = InboundStage(eng, *_rows(in_b[self.lo:self.hi]), ring_capacity=512)
        self.ledger = PacketLedger(eng)
        self.win = Window(eng, self.hi - self.lo)

    def setup_outbound(self):
        from shadow_amd.outbound import OutboundStage
        self.ostage = OutboundStage(self.eng, *_rows(self.out_b[self.lo:self.hi]), first_host=self.lo, ring_capacity=64)


def _dev(arr):
    import torch
    d = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(a.dtype.str.replace("u", "i"))).cuda()
         for a in arr]
    torch.cuda.synchronize()
    return d


def _offers_of(per_host, lo, hi):
    mine = per_host[lo:hi]
    arr = _arrays(mine) if any(mine) else (None,) * 7
    return _dev(arr), (0 if arr[0] is None else len(arr[1]))


def _code(fn):
    from shadow_amd._native import ShdError
    try:
        return None, fn()
    except ShdError as e:
        return e.code, None


def _world(n, o, rng0, out_b, in_b, knob=None, x24=None):
    from shadow_amd import dist as D
    from shadow_amd.routing import Engine
    engines = [Engine(0) for _ in range(n)]
    if knob is not None:
        for e in engines:
            knob("RELAY_SHARD_X24", 1 if x24 else 0, eng=e)
    D.comm_init_local(engines)
    return engines, [RankParts(e, o, rng0, out_b, in_b) for e in engines]


def run_windows(parts, o, offers, n, first, wrong_end_rank=None, all_ranks=True):
    """n windows through every rank's open and close, each rank's outputs against the oracle's
    step for its hosts.  wrong_end_rank: in window 0 that rank first calls the close with another
    window_end -- every rank's close is refused with SHD_ERR_INVALID, nothing has run.
    all_ranks=False: `parts` holds this process's rank alone (the others run in processes of
    their own), so the totals over all ranks are not taken."""
    from shadow_amd.rounds import next_window as eng_window
    ws, we = first
    for k in range(n):
        per_host = offers(k, ws, we)
        arr = _arrays(per_host) if any(per_host) else (None,) * 7
        mo, status, popped, mi, want_win = o.step(arr, we)
        sent = status == 2
        n_sent = int(sent.sum())
        pending = sum(len(x) for x in o.q.q) - n_sent   # the engine merges this window's batch at the next open
        devs = [_offers_of(per_host, p.lo, p.hi) for p in parts]

        def rank_window(i, k=k, we=we):
            p = parts[i]
            d_arr, n_off = devs[i]
            op = p.win.open(we)
            rec = p.win.records(op)
            led_open = p.ledger.stats()
            refused = None
            if k == 0 and wrong_end_rank is not None:
                refused = _code(lambda: p.win.close(*d_arr, n_off, we + (1 if i == wrong_end_rank else 0), o.end_time))[0]
            cl = p.win.close(*d_arr, n_off, we, o.end_time)
            ch = p.win.closed(cl)
            led_close = p.ledger.stats()
            cpu_next = min(op.records.next_task_time, cl.next_task_time)
            got_win = eng_window(p.eng, None if cpu_next == IDLE else cpu_next, o.end_time)
            return op, rec, led_open, refused, cl, ch, led_close, got_win
        res = _run_ranks([lambda i=i: rank_window(i) for i in range(len(parts))])
        live = 0
        for p, (op, rec, led_open, refused, cl, ch, led_close, got_win) in zip(parts, res):
            lo, hi = p.lo, p.hi
            if wrong_end_rank is not None and k == 0:
                assert refused == "INVALID", (k, p.lo, refused)
            # the open: the inbound records of the rank's hosts
            a, z = int(mi[0][lo]), int(mi[0][hi])
            assert np.array_equal(rec.off.astype(np.int64), mi[0][lo:hi + 1].astype(np.int64) - a), k
            for got, want in zip((rec.pkt, rec.time, rec.kind), mi[1:4]):
                assert np.array_equal(got, want[a:z]), k
            in_hosts, out_hosts = o.im.hosts[lo:hi], o.om.hosts[lo:hi]
            tasks = [x.task for x in in_hosts if x.task is not None]
            assert (rec.n_stored, rec.next_task_time) == (sum(x.stored() for x in in_hosts), min(tasks, default=IDLE)), k
            assert op.n_popped == int(popped["off"][hi]) - int(popped["off"][lo]), k
            assert led_open.live_events == op.n_pending, k
            # the close: the rank's own sends and local deliveries, the events it received
            b0, b1 = int(mo["src_off"][lo]), int(mo["src_off"][hi])
            assert np.array_equal(ch.sent_pkt, mo["sent_pkt"][b0:b1]) and np.array_equal(ch.sent_status, status[b0:b1]), k
            l0, l1 = int(mo["loc_off"][lo]), int(mo["loc_off"][hi])
            assert np.array_equal(ch.loc_off.astype(np.int64), mo["loc_off"][lo:hi + 1].astype(np.int64) - l0), k
            assert np.array_equal(ch.loc_pkt, mo["loc_pkt"][l0:l1]) and np.array_equal(ch.loc_time, mo["loc_time"][l0:l1]), k
            tasks = [x.task for x in out_hosts if x.task is not None]
            dst = mo["dst_host"][sent]
            n_recv = int(((dst >= lo) & (dst < hi)).sum())
            assert (cl.n_batch, cl.n_events, cl.n_local, cl.n_stored, cl.next_task_time) == \
                   (b1 - b0, n_recv, l1 - l0, sum(x.stored() for x in out_hosts), min(tasks, default=IDLE)), k
            assert (cl.min_deliver == IDLE) == (n_sent == 0), k
            assert led_close.live_events == op.n_pending + n_recv, k
            assert got_win == want_win, (k, got_win, want_win)
            live += op.n_pending
        if all_ranks:
            assert live == pending, k
            assert sum(r[0].n_popped for r in res) == len(popped["tag"]), k
        if want_win is not None:
            ws, we = want_win
        else:
            assert k == n - 1


def _chain(world, knob=None, x24=None, wrong_end_rank=None):
    o = ChainOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    engines, parts = _world(world, o, rng0, out_b, in_b, knob, x24)
    try:
        prio = [0] * o.H
        first = (S + 10**9, S + 10**9 + o.ra.get())
        run_windows(parts, o, lambda k, ws, we: chain_offers(k, ws, we, o.H, prio), 3, first, wrong_end_rank)
        assert len(o.batches) >= 2 and sum(len(b[1]) for b in o.batches) > 150
        return [p.relay.last_pipeline() for p in parts]
    finally:
        for e in engines:
            e.close()


@pytest.mark.parametrize("world", [2, 3])
def test_chain_three_windows(world):
    _chain(world)


@pytest.mark.parametrize("x24", [False, True])
def test_chain_both_exchange_forms(engine, knob, x24):
    """The round's two exchange forms under the window: the stamp's bins sent as they lie, and the
    packed 24-byte events (RELAY_SHARD_X24)."""
    pipes = _chain(2, knob, x24)
    if x24:
        assert 8 not in pipes


def test_chain_nine_ranks_one_without_hosts():
    """64 hosts on nine ranks: the ninth owns no host and still takes part in every close."""
    _chain(9)


@pytest.mark.parametrize("world", [2, 3])
def test_long_run(world):
    """70 hosts, 14 windows, several batches live on every rank."""
    from tests.test_window_gpu import LONG_WINDOWS, _long_oracle
    o = _long_oracle()
    prio = [0] * o.H
    engines, parts = _world(world, o, o.rng0, o.out_b, o.in_b)
    try:
        first = (S + 10**9, S + 10**9 + o.ra.get())
        run_windows(parts, o, lambda k, ws, we: o.offers(k, ws, we, prio), LONG_WINDOWS, first)
        assert max(o.live_at_once) >= 3
    finally:
        for e in engines:
            e.close()


def test_wrong_window_end_on_one_rank_is_refused_everywhere():
    """Rank 1 calls the first close with another window_end: every rank gets SHD_ERR_INVALID and
    nothing has run -- the right close that follows, and the two windows after it, match the oracle."""
    _chain(2, wrong_end_rank=1)


def test_outbound_violation_on_one_rank_fails_every_close():
    """Window 1: rank 1 offers a packet timed before the previous window_end, which its outbound
    stage refuses.  Every rank's close returns that status; no rank's relay state has advanced;
    after rank 1 has set its stage up again a further window runs on every rank."""
    o = ChainOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    engines, parts = _world(2, o, rng0, out_b, in_b)
    try:
        prio = [0] * o.H
        ws, we = S + 10**9, S + 10**9 + o.ra.get()
        run_windows(parts, o, lambda k, a, b: chain_offers(k, a, b, o.H, prio), 1, (ws, we))
        we2, we3 = we + o.ra.get(), we + 2 * o.ra.get()
        per_host = chain_offers(1, we, we2, o.H, prio)
        lo1 = parts[1].lo
        per_host[lo1] = [(we - 1, prio[lo1], 100 + 52, 100, 0, 900_000)]   # below the previous window_end
        devs = [_offers_of(per_host, p.lo, p.hi) for p in parts]

        def bad_window(i):
            p = parts[i]
            p.win.open(we2)
            before = p.relay.host_state()
            code = _code(lambda: p.win.close(*devs[i][0], devs[i][1], we2, o.end_time))[0]
            return code, before, p.relay.host_state()
        res = _run_ranks([lambda i=i: bad_window(i) for i in range(2)])
        for code, before, after in res:
            assert code == "INVALID"
            assert np.array_equal(before[0], after[0]) and np.array_equal(before[1], after[1])
        parts[1].setup_outbound()

        def next_window(i):
            p = parts[i]
            op = p.win.open(we3)
            live = p.ledger.stats().live_events
            cl = p.win.close(*(None,) * 7, 0, we3, o.end_time)
            return op.n_pending, live, cl.n_batch
        res = _run_ranks([lambda i=i: next_window(i) for i in range(2)])
        for n_pending, live, _ in res:
            assert live == n_pending
    finally:
        for e in engines:
            e.close()
