"""GPU parity of the two-call scheduling window (shadow_amd/window.py, csrc/window.cpp): open =
event queues -> ledger gather -> inbound stage, close = outbound stage -> relay round -> ledger
record, against the composed oracle of tests/test_outbound_gpu.py (outbound model -> oracle relay
-> oracle queues -> inbound model).  The oracle merges a batch in the window that sent it, the
engine at the next open: every event of a batch has deliver >= that window's end, so both pop the
same events with the same tags.  No size or id array is built on the host for the engine."""
import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S
from tests.outbound_model import IDLE, OutboundModel
from tests.test_outbound import MS, bucket
from tests.test_outbound_gpu import HEADER, ChainOracle, _arrays, chain_case, chain_offers

pytestmark = pytest.mark.gpu


class Parts:
    """Everything the window calls need, set up on one engine for the oracle's hosts."""

    def __init__(self, eng, o, rng0, out_b, in_b, first_host=0, max_live=0):
        from shadow_amd.equeue import EventQueues
        from shadow_amd.inbound import InboundStage
        from shadow_amd.ledger import PacketLedger
        from shadow_amd.outbound import OutboundStage
        from shadow_amd.relay import Relay
        from shadow_amd.rounds import Runahead
        from shadow_amd.window import Window
        H = o.H
        rows = lambda bs: [np.array([(0, 0, 0, S)[i] if b is None else b[i] for b in bs], np.uint64)  # noqa: E731
                           for i in range(4)]
        self.eng = eng
        self.relay = Relay(o.host_node, rng0, np.zeros(H, np.uint64), o.lat, o.loss, engine=eng)
        self.queues = EventQueues(eng, H)
        self.runahead = Runahead(eng, True, int(o.lat.min()))
        self.ostage = OutboundStage(eng, *rows(out_b), first_host=first_host, ring_capacity=64)
        self.istage = InboundStage(eng, *rows(in_b), ring_capacity=512)
        self.ledger = PacketLedger(eng, max_live)
        self.win = Window(eng, H)


def _dev(arr):
    import torch
    d = [None if a is None else torch.from_numpy(np.ascontiguousarray(a).view(a.dtype.str.replace("u", "i"))).cuda()
         for a in arr]
    torch.cuda.synchronize()
    return d


def run_windows(p, o, offers, n, first, mischief=False, windows=None):
    """n windows through open and close, every output against the oracle's step; the next window
    from shd_round_window (or the list `windows`).  mischief: the wrong calls of the call-order
    contract in between -- each is refused and changes nothing.  Returns the ledger's stats after
    every close."""
    from shadow_amd._native import ShdError
    from shadow_amd.rounds import next_window as eng_window
    win, led = p.win, p.ledger
    ws, we = first
    stats = []
    for k in range(n):
        per_host = offers(k, ws, we)
        arr = _arrays(per_host) if any(per_host) else (None,) * 7
        mo, status, popped, mi, want_win = o.step(arr, we)
        n_sent = int((status == 2).sum())
        pending = sum(len(x) for x in o.q.q) - n_sent   # the engine merges this window's batch at the next open
        d_arr = _dev(arr)
        n_off = 0 if arr[0] is None else len(arr[1])
        if mischief:   # a close first / a second close
            with pytest.raises(ShdError, match="STATE"):
                win.close(*d_arr, n_off, we, o.end_time)
        op = win.open(we)
        rec = win.records(op)
        for got, want in zip((rec.off, rec.pkt, rec.time, rec.kind, rec.n_stored, rec.next_task_time), mi):
            assert np.array_equal(got, want), k
        assert (op.n_popped, op.n_pending) == (len(popped["tag"]), pending), k
        heads = [t for t in (o.q.next_event_time(h) for h in range(o.H)) if t is not None]
        if n_sent == 0:   # (otherwise the oracle's heads already count this window's batch)
            assert op.queue_next_time == (min(heads) if heads else IDLE)
        st = led.stats()
        assert st.live_events == op.n_pending and (st.live_events == 0) == (pending == 0), k
        if mischief:
            with pytest.raises(ShdError, match="STATE"):
                win.open(we)
            with pytest.raises(ShdError, match="INVALID"):
                win.close(*d_arr, n_off, we + 1, o.end_time)
        cl = win.close(*d_arr, n_off, we, o.end_time)
        ch = win.closed(cl)
        assert np.array_equal(ch.sent_pkt, mo["sent_pkt"]) and np.array_equal(ch.sent_status, status), k
        for x in ("loc_off", "loc_pkt", "loc_time"):
            assert np.array_equal(getattr(ch, x), mo[x]), (k, x)
        assert (cl.n_batch, cl.n_events, cl.n_stored, cl.next_task_time) == \
               (len(mo["sent_pkt"]), n_sent, mo["n_stored"], mo["next_task_time"]), k
        assert (cl.min_deliver == IDLE) == (n_sent == 0)
        st = led.stats()
        stats.append(st)
        assert st.live_events == pending + n_sent, k
        cpu_next = min(op.records.next_task_time, cl.next_task_time)
        got_win = eng_window(p.eng, None if cpu_next == IDLE else cpu_next, o.end_time)
        assert got_win == want_win, (k, got_win, want_win)
        if windows is not None:
            ws, we = windows[k] or (ws, we)
        elif want_win is not None:
            ws, we = want_win
        else:
            assert k == n - 1
    return stats


def _chain(eng, mischief=False):
    """The chain test's three windows."""
    o = ChainOracle(S + 10**12)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    p = Parts(eng, o, rng0, out_b, in_b)
    prio = [0] * o.H
    first = (S + 10**9, S + 10**9 + o.ra.get())
    run_windows(p, o, lambda k, ws, we: chain_offers(k, ws, we, o.H, prio), 3, first, mischief)
    assert o.decided[0] == ["outbound"] and o.decided[2] == ["inbound"], o.decided
    assert len(o.batches) >= 2 and sum(len(b[1]) for b in o.batches) > 150
    return o, p


def test_chain_through_open_and_close():
    from shadow_amd.routing import Engine
    from tests.test_inbound_gpu import _same_state as _same_in_state
    from tests.test_outbound_gpu import _same_state
    with Engine(0) as eng:
        o, p = _chain(eng)
        for h in range(o.H):
            _same_state(p.ostage.state(h), o.om.hosts[h])
            _same_in_state(p.istage.state(h), o.im.hosts[h])


class LongOracle(ChainOracle):
    """70 hosts, one node each, path latencies from one to four and a half runaheads (10 ms, the
    pair 0 <-> 1), fast buckets on a few hosts; per window it notes how many batches had events
    pending, how many batches its pops came from, and whether a batch drained before an older one."""
    H_, RA = 70, 10 * MS

    def __init__(self, end_time, seed):
        from oracle.relay import EventQueues, RunaheadState
        from shadow_amd import synth
        from tests.inbound_model import InboundModel
        H = self.H = self.H_
        rng = np.random.default_rng(seed)
        self.lat = rng.integers(self.RA, 45 * MS, (H, H)).astype(np.uint64)
        self.lat[0, 1] = self.lat[1, 0] = self.RA
        self.loss = np.full((H, H), 0.02, np.float32)
        self.host_node = np.arange(H, dtype=np.uint32)
        self.rng0 = synth.host_rng_states(H, 3)
        self.out_b = [bucket(1_250_000) if h % 4 == 1 else None for h in range(H)]
        self.in_b = [bucket(1_250_000) if h % 2 else None for h in range(H)]
        self.om, self.im = OutboundModel(self.out_b), InboundModel(self.in_b)
        self.rng, self.nid = self.rng0.copy(), np.zeros(H, np.uint64)
        self.q = EventQueues(H)
        self.ra = RunaheadState(True, int(self.lat.min()))
        self.end_time = end_time
        self.batches, self.decided = [], []
        self.live, self.stored, self.expect, self.live_sets = {}, [], [], []
        self.live_at_once, self.popped_from, self.early_drain = [], [], False
        self.offer_rng = np.random.default_rng(seed + 1)

    def step(self, arr, we):
        n_before = len(self.batches)
        out = super().step(arr, we)
        status, popped = out[1], out[2]
        if len(self.batches) > n_before:
            self.stored.append(len(status) if (status == 2).any() else 0)   # a batch without an event is not kept
            if (status == 2).any():
                self.live[n_before] = int((status == 2).sum())
        self.live_at_once.append(len(self.live))
        b, c = np.unique((popped["tag"] >> np.uint64(32)).astype(np.int64), return_counts=True)
        self.popped_from.append(len(b))
        for x, y in zip(b.tolist(), c.tolist()):
            self.live[x] -= y
            if self.live[x] == 0:
                del self.live[x]
                self.early_drain |= any(z < x for z in self.live)
        # the ledger after this window's close: (live_batches, live_events, entries_held, oldest_batch)
        old = min(self.live) if self.live else None
        self.live_sets.append(set(self.live))
        self.expect.append((len(self.live), sum(self.live.values()), 0 if old is None else sum(self.stored[old:]), old))
        return out

    def offers(self, k, ws, we, prio):
        """Every fourth window host 0 alone sends one packet down the shortest path; otherwise
        every host offers up to two packets anywhere (a tenth local)."""
        rng = self.offer_rng
        per_host, pid = [], k * 100_000
        for h in range(self.H):
            if k % 4 == 3:
                offers = [(ws, prio[h], 100 + HEADER, 100, 1, pid)] if h == 0 else []
            else:
                times = np.sort(rng.integers(ws, we, int(rng.integers(0, 3)))).tolist()
                offers = []
                for i, t in enumerate(times):
                    dst = h if rng.random() < 0.1 else int(rng.integers(0, self.H))
                    pay = int(rng.choice([0, 1448, int(rng.integers(1, 1449))]))
                    offers.append((t, prio[h] + i, pay + HEADER, pay, dst, pid + i))
            prio[h] += len(offers)
            pid += len(offers)
            per_host.append(offers)
        return per_host


LONG_SEED, LONG_WINDOWS = 3, 14


def _long_oracle():
    return LongOracle(S + 10**12, LONG_SEED)


def _long_shape(o):
    assert max(o.live_at_once) >= 3 and max(o.popped_from) >= 3 and o.early_drain, \
        (o.live_at_once, o.popped_from, o.early_drain)
    assert int(o.lat.max()) >= 4 * o.ra.get() and int(o.lat.min()) == o.ra.get()
    assert o.im.counters["blocks"] > 0


def test_long_run():
    """70 hosts (no multiple of 64), 14 windows, offers in most of them, several batches live:
    every record, status and window; the ledger's entries follow the oldest batch held."""
    from shadow_amd.routing import Engine
    shape = _long_oracle()
    prio = [0] * shape.H
    ws, we = S + 10**9, S + 10**9 + shape.ra.get()
    for k in range(LONG_WINDOWS):
        per_host = shape.offers(k, ws, we, prio)
        ws, we = shape.step(_arrays(per_host) if any(per_host) else (None,) * 7, we)[4]
    _long_shape(shape)   # on the oracle alone, before any GPU call
    o = _long_oracle()
    prio = [0] * o.H
    with Engine(0) as eng:
        p = Parts(eng, o, o.rng0, o.out_b, o.in_b)
        first = (S + 10**9, S + 10**9 + o.ra.get())
        stats = run_windows(p, o, lambda k, ws, we: o.offers(k, ws, we, prio), LONG_WINDOWS, first)
    # the ledger after every close: a batch that drained before an older one still counts in entries_held
    assert [(s.live_batches, s.live_events, s.entries_held, s.oldest_batch) for s in stats] == o.expect
    assert any(e[2] > sum(o.stored[b] for b in range(e[3], len(o.stored)) if b in live) for e, live in
               zip(o.expect, o.live_sets) if e[3] is not None)


def test_call_order_refusals_change_nothing():
    """A close first, two opens, a close with another window_end, a second close: each refused,
    and the three windows still match the oracle."""
    from shadow_amd.routing import Engine
    with Engine(0) as eng:
        _chain(eng, mischief=True)


def _refused(p):
    from shadow_amd._native import ShdError
    with pytest.raises(ShdError, match="STATE"):
        p.win.open(S + 10**9)
    with pytest.raises(ShdError, match="STATE"):
        p.win.close(*(None,) * 7, 0, S + 10**9, S + 10**12)


def test_first_host_not_zero_is_refused():
    from shadow_amd.routing import Engine
    with Engine(0) as eng:
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        _refused(Parts(eng, o, rng0, out_b, in_b, first_host=5))
        _chain(eng)


def test_missing_stage_is_refused():
    """An inbound stage set up for another host count than the other parts."""
    from shadow_amd.inbound import InboundStage
    from shadow_amd.routing import Engine
    with Engine(0) as eng:
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(eng, o, rng0, out_b, in_b)
        InboundStage(eng, *(np.zeros(o.H + 1, np.uint64),) * 3)
        _refused(p)
        _chain(eng)


def test_two_rank_communicator_is_refused():
    """A context under a two-rank in-process communicator: refused; with the communicator gone
    and the parts set up again the windows match the oracle."""
    from shadow_amd import _native as N
    from shadow_amd import dist as D
    from shadow_amd.routing import Engine
    engines = [Engine(0), Engine(0)]
    try:
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(engines[0], o, rng0, out_b, in_b)
        D.comm_init_local(engines)
        _refused(p)
        for e in engines:
            N.check(e.lib.shd_comm_destroy(e.ctx), "shd_comm_destroy")
        _chain(engines[0])
    finally:
        for e in engines:
            e.close()


def test_nothing_pending_and_no_offers():
    from shadow_amd.routing import Engine
    with Engine(0) as eng:
        o = ChainOracle(S + 10**12)
        _, _, _, _, rng0, out_b, in_b = chain_case()
        p = Parts(eng, o, rng0, out_b, in_b)
        for we in (S + 10**9, S + 2 * 10**9):
            op = p.win.open(we)
            assert (op.n_popped, op.n_pending, op.queue_next_time) == (0, 0, IDLE)
            assert (op.records.n_out, op.records.n_stored, op.records.next_task_time) == (0, 0, IDLE)
            assert p.win.records(op).off.tolist() == [0] * (o.H + 1)
            cl = p.win.close(*(None,) * 7, 0, we, S + 10**12)
            assert (cl.n_batch, cl.n_events, cl.n_local, cl.n_stored, cl.next_task_time, cl.min_deliver) == \
                   (0, 0, 0, 0, IDLE, IDLE)
            s = p.ledger.stats()
            assert (s.live_batches, s.live_events, s.entries_held, s.oldest_batch) == (0, 0, 0, None)
            assert p.ledger.next_batch() == 0


def test_sim_end_inside_a_window():
    """The experiment ends two thirds into the first window: the packets sent after it are
    SKIPPED -- they lie in the batch's ledger slice (the indices of the later ones stay right) but
    are not counted live.  A second, far window pops every event."""
    from shadow_amd.routing import Engine
    ws = S + 10**9
    probe = ChainOracle(S + 10**12)
    we = ws + probe.ra.get()
    o = ChainOracle(ws + (we - ws) * 2 // 3)
    _, _, _, _, rng0, out_b, in_b = chain_case()
    prio = [0] * o.H
    far = we + 10**10
    with Engine(0) as eng:
        p = Parts(eng, o, rng0, out_b, in_b)
        stats = run_windows(p, o, lambda k, a, b: chain_offers(0, a, b, o.H, prio) if k == 0 else [[]] * o.H, 2,
                            (ws, we), windows=[(we, far), None])
        op = p.win.open(far + 1)
        s = p.ledger.stats()
    n0 = len(o.batches[0][1])
    assert o.decided and stats[0].entries_held == n0 and 0 < stats[0].live_events < n0
    skipped = n0 - stats[0].live_events
    assert skipped > 10   # (2 % of the rest is dropped: most of the gap is SKIPPED packets)
    assert (op.n_pending, s.live_events, s.entries_held) == (0, 0, 0)
