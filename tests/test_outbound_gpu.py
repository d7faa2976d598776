"""GPU parity of the outbound stage (shadow_amd/outbound.py, csrc/outbound.hip) against the CPU model
(tests/outbound_model.py): the batch arrays, sent_pkt, the local CSR, the stored total, the next
task time and the per-host state, exactly."""
import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.outbound_model import IDLE, LOCAL, SENT, OutboundModel
from tests.test_outbound import CASES, MS, arrays, bucket, check_final

pytestmark = pytest.mark.gpu

HEADER = 52   # total size = HEADER + payload; 1448 + 52 = CONFIG_MTU, within every bucket
KEYS = ("src_off", "send_time", "dst_host", "payload", "sent_pkt", "loc_off", "loc_pkt", "loc_time")


def _stage(engine, buckets, first_host=0, ring=512):
    from shadow_amd.outbound import OutboundStage
    rows = [(0, 0, 0, S) if b is None else b for b in buckets]
    cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
    return OutboundStage(engine, cap, inc, itv, last, first_host=first_host, ring_capacity=ring)


def _arrays(per_host):
    """[[(time, prio, size, payload, dst, pkt)] per host] -> off, time, prio, size, payload, dst, pkt."""
    off = np.zeros(len(per_host) + 1, np.uint32)
    off[1:] = np.cumsum([len(e) for e in per_host])
    flat = [x for e in per_host for x in e]
    col = lambda i, dt: np.array([x[i] for x in flat], dt)  # noqa: E731
    return (off, col(0, np.uint64), col(1, np.uint64), col(2, np.uint32), col(3, np.uint32), col(4, np.uint32),
            col(5, np.uint32))


def _same(r, want):
    for k in KEYS:
        assert np.array_equal(getattr(r, k), want[k]), k
    assert (r.n_stored, r.next_task_time) == (want["n_stored"], want["next_task_time"])


def _same_state(st, host):
    assert st["task_time"] == host.task
    assert st["cached"] == (None if host.cached is None else (host.cached[1], host.cached[2]))
    assert st["queue_len"] == len(host.q)
    assert st["head_pkt"] == (min(host.q)[1] if host.q else None)
    if host.tb is None:
        assert st["bucket"] is None
    else:
        b = st["bucket"]
        assert (b["capacity"], b["balance"], b["refill_increment"], b["refill_interval"], b["last_refill"]) == \
               (host.tb.capacity, host.tb.balance, host.tb.refill_increment, host.tb.refill_interval,
                host.tb.last_refill)
        assert b["pending_until"] == (host.task or 0)


@pytest.mark.parametrize("name", list(CASES))
def test_hand_cases_on_device(engine, name):
    b, first, steps, final = CASES[name]
    stage = _stage(engine, [b], first)
    model = OutboundModel([b], first)
    for offers, w_end, boot, recs, n_stored, nxt in steps:
        arr = [np.asarray(a) for a in arrays([[(S + t, pr, s, d, p) for t, pr, s, d, p in offers]])]
        r = stage.advance(*arr, window_end=S + w_end, bootstrap_end=boot)
        got = [(SENT, p, t - S) for p, t, _, _ in r.sent_for(0)] + [(LOCAL, p, t - S) for p, t in r.local_for(0)]
        assert got == recs
        assert (r.n_stored, r.next_task_time) == (n_stored, IDLE if nxt is None else S + nxt)
        _same(r, model.advance(*arr, S + w_end, boot))
    st = stage.state(0)
    check_final(final, None if st["task_time"] is None else st["task_time"] - S,
                None if st["cached"] is None else st["cached"][0],
                None if st["bucket"] is None else st["bucket"]["balance"], st["queue_len"])
    _same_state(st, model.hosts[0])


def test_from_bandwidth(engine):
    """OutboundStage.from_bandwidth: create_token_bucket per host, None or a negative entry for a
    host without a bucket.  The carried case on the 1000 B/s host, a burst on the two others."""
    from shadow_amd.outbound import OutboundStage
    stage = OutboundStage.from_bandwidth(engine, [1000, None, -1, 0], S, ring_capacity=16)
    burst = [(S + 5, 1 + p, 1500, 1448, 0, p) for p in range(3)]
    r = stage.advance(*_arrays([[(S, 1, 1500, 1448, 1, 10), (S, 2, 1500, 1448, 1, 11)], burst,
                                [(t, pr, s, pl, d, p + 3) for t, pr, s, pl, d, p in burst], []]),
                      window_end=S + 10 * MS)
    assert r.sent_for(0) == [(10, S, 1, 1448)] and r.next_task_time == S + 1499 * MS and r.n_stored == 1
    assert r.sent_for(1) == [(p, S + 5, 0, 1448) for p in range(3)]
    assert r.sent_for(2) == [(p, S + 5, 0, 1448) for p in range(3, 6)]
    assert len(r.loc_pkt) == 0
    want = dict(zip(("capacity", "refill_increment", "refill_interval"), create_token_bucket(1000)))
    b = stage.state(0)["bucket"]
    assert {k: b[k] for k in want} == want and (b["balance"], b["last_refill"]) == (1, S)
    assert stage.state(0)["cached"] == (11, 1500)
    assert stage.state(1)["bucket"] is None and stage.state(2)["bucket"] is None
    b = stage.state(3)["bucket"]   # a rate of 0 is still a bucket: 1 byte per ms
    assert (b["capacity"], b["refill_increment"], b["balance"]) == (1501, 1, 1501)


RATES = [0, 1000, 20_000, 125_000, 1_250_000, 125_000_000]


def _random_window(rng, model, start, end, pid, prio, max_offers=40, n_dst=None):
    """Offers for every host of the model in [start, end): 10 % local, 10 % of the priorities out
    of arrival order (neighbours swapped, same-instant pairs included), half the hosts with a
    same-instant pair, half of the pending ones with an offer at the outstanding task's time."""
    per_host = []
    n_dst = n_dst or len(model.hosts)
    for h, host in enumerate(model.hosts):
        n = int(rng.integers(0, max_offers))
        times = np.sort(rng.integers(start, end, n)).tolist()
        if n >= 2 and rng.random() < 0.5:
            times[1] = times[0]
        if n and host.task is not None and start <= host.task < end and rng.random() < 0.5:
            times[int(rng.integers(0, n))] = host.task   # an offer at exactly the outstanding task's time
            times.sort()
        prios = list(range(prio[h], prio[h] + n))         # the host's counter (host.rs:604-610)
        prio[h] += n
        for i in range(n - 1):
            if rng.random() < 0.1:
                prios[i], prios[i + 1] = prios[i + 1], prios[i]
        offers = []
        for i, t in enumerate(times):
            dst = host.id if rng.random() < 0.1 else int(rng.integers(0, n_dst))
            pay = int(rng.integers(0, 1449))
            offers.append((t, prios[i], pay + HEADER, pay, dst, pid + i))
        per_host.append(offers)
        pid += n
    return per_host, pid


@pytest.mark.parametrize("seed", range(6))
def test_random_windows_vs_model(engine, seed):
    """Five consecutive windows over up to 300 hosts (past one 256-lane workgroup, a partial wave)
    with mixed buckets, bootstrap_end inside the second window: every array of every window, then
    every host's state.  The model's counters show that each branch ran."""
    rng = np.random.default_rng(1924 + seed)   # 298, 64, 159, 65, 218 and 30 hosts
    n_hosts = int(rng.integers(1, 301))
    buckets = [None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(RATES))), S)
               for _ in range(n_hosts)]
    stage = _stage(engine, buckets, ring=512)
    model = OutboundModel(buckets)
    ends = np.cumsum([int(rng.choice([1, 20, 150, 400])) * MS for _ in range(5)]) + S
    boot = int(ends[0] + (ends[1] - ends[0]) // 2)
    start, pid, prio = S, 0, [0] * n_hosts
    for end in ends.tolist():
        per_host, pid = _random_window(rng, model, start, end, pid, prio)
        arr = _arrays(per_host)
        want = model.advance(*arr, end, boot)
        _same(stage.advance(*arr, window_end=end, bootstrap_end=boot), want)
        for h in range(n_hosts):
            _same_state(stage.state(h), model.hosts[h])
        start = end
    for k, v in model.counters.items():
        assert v > 0, (k, model.counters)
    assert model.max_depth <= 512


def test_many_hosts_past_one_scan_tile(engine):
    """9001 hosts: more than one 8192-entry tile in all three scans (region bounds, sent offsets,
    local offsets) and 36 workgroups of lanes; two windows, a quarter of the hosts blocked across
    them, every host with local packets."""
    rng = np.random.default_rng(78)
    n_hosts = 9001
    buckets = [bucket(1000) if h % 4 == 0 else (None if h % 4 == 1 else bucket(125_000)) for h in range(n_hosts)]
    stage = _stage(engine, buckets, ring=8)
    model = OutboundModel(buckets)
    start, pid, prio = S, 0, [0] * n_hosts
    for win in (20 * MS, 4000 * MS):
        per_host, pid = _random_window(rng, model, start, start + 20 * MS, pid, prio, max_offers=4)
        arr = _arrays(per_host)
        want = model.advance(*arr, start + win, 0)
        _same(stage.advance(*arr, window_end=start + win), want)
        assert want["src_off"][-1] > 8192 and want["loc_off"][-1] > 500
        for h in range(n_hosts):
            _same_state(stage.state(h), model.hosts[h])
        start += win
    assert model.counters["blocks"] > 500 and model.counters["carried"] > 500


def test_nonzero_first_host(engine):
    """first_host = 4500: a packet is local when dst is the host's global id, not its index.  The
    local one is larger than every bucket: the size contract binds packets the bucket weighs."""
    rng = np.random.default_rng(79)
    n_hosts, first = 64, 4500
    buckets = [bucket(125_000) if h % 2 else None for h in range(n_hosts)]
    stage = _stage(engine, buckets, first_host=first, ring=64)
    model = OutboundModel(buckets, first)
    per_host, _ = _random_window(rng, model, S, S + 20 * MS, 0, [0] * n_hosts, max_offers=12)
    for h, offers in enumerate(per_host):   # + one packet to the host's own index, one to its global id
        t = offers[-1][0] if offers else S
        offers += [(t, 1000, 100, 48, h, 10_000 + h), (t, 1001, 5000, 4948, first + h, 20_000 + h)]
    arr = _arrays(per_host)
    want = model.advance(*arr, S + 4000 * MS, 0)
    r = stage.advance(*arr, window_end=S + 4000 * MS)
    _same(r, want)
    assert set(range(20_000, 20_000 + n_hosts)) <= set(r.loc_pkt.tolist())
    assert set(range(10_000, 10_000 + n_hosts)) <= set(r.sent_pkt.tolist())
    for h in range(n_hosts):
        _same_state(stage.state(h), model.hosts[h])


# (buckets, ring, [(per_host offers or "raw", window_end)]): the last step violates the contract
_P = lambda t, prio, pkt, size=100, dst=1: (t, prio, size, size - HEADER, dst, pkt)  # noqa: E731
BAD = {
    "offsets_not_a_csr": ([bucket(), bucket()], 4, [("raw", S + 10)]),
    "offer_at_window_end": ([bucket()], 4, [([[_P(S + 10, 1, 0)]], S + 10)]),
    # the relay is blocked, its task carried past the window's end, and the offer lies beyond that
    # task: the check must not depend on the offer being weighed against the task
    "offer_past_window_end_behind_a_carried_task":
        ([bucket()], 4, [([[_P(S, 1, 0, 1500), _P(S, 2, 1, 1500)]], S + 10 * MS),
                         ([[_P(S + 1500 * MS, 3, 2)]], S + 20 * MS)]),
    "decreasing_time": ([bucket()], 4, [([[_P(S + 5, 1, 0), _P(S + 4, 2, 1)]], S + 10)]),
    "before_the_last_window": ([bucket()], 4, [([[_P(S + 5, 1, 0)]], S + 10), ([[_P(S + 9, 2, 1)]], S + 20)]),
    "size_above_capacity": ([bucket()], 4, [([[_P(S + 5, 1, 0, 1502)]], S + 10)]),
    "pkt_id_uint32_max": ([bucket()], 4, [([[_P(S + 5, 1, 2**32 - 1)]], S + 10)]),
    # p0 leaves, p1 is cached, p2 (priority 7) stays queued; p3 offers priority 7 again
    "priority_equal_to_a_queued_one":
        ([bucket()], 4, [([[_P(S, 1, 0, 1500), _P(S, 2, 1, 1500), _P(S + 1, 7, 2)]], S + 10),
                         ([[_P(S + 20, 9, 4), _P(S + 21, 7, 3)]], S + 100)]),
    # capacity 4: p1 is cached behind p0, then five offers before its task runs
    "ring_overflow": ([bucket()], 4, [([[_P(S, 1, 0, 1500), _P(S, 2, 1, 1500)]], S + 10),
                                      ([[_P(S + 20 + i, 3 + i, 2 + i) for i in range(5)]], S + 100)]),
    # the bucket was last refilled after the offer's time: duration_since(..).unwrap() panics
    "time_before_the_last_refill": ([bucket(1000, S + 50)], 4, [([[_P(S + 5, 1, 0)]], S + 10)]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_contract_errors(engine, name):
    """Each violation is SHD_ERR_INVALID from a check (no lane may spin or read out of range), the
    next advance and get_state SHD_ERR_STATE, and a fresh setup works again."""
    from shadow_amd._native import ShdError
    buckets, ring, steps = BAD[name]
    stage = _stage(engine, buckets, ring=ring)
    for per_host, w_end in steps[:-1]:
        stage.advance(*_arrays(per_host), window_end=w_end)
    per_host, w_end = steps[-1]
    if per_host == "raw":   # host 0's range runs past host 1's
        arr = (np.array([0, 3, 2], np.uint32), np.full(2, S + 1, np.uint64), np.arange(2, dtype=np.uint64),
               np.full(2, 100, np.uint32), np.full(2, 48, np.uint32), np.ones(2, np.uint32),
               np.arange(2, dtype=np.uint32))
    else:
        arr = _arrays(per_host)
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance(*arr, window_end=w_end)
    with pytest.raises(ShdError, match="STATE"):
        stage.advance(window_end=w_end + 10)
    with pytest.raises(ShdError, match="STATE"):
        stage.state(0)
    stage = _stage(engine, buckets, ring=ring)
    r = stage.advance(*_arrays([[_P(S + 61, 1, 7)]] + [[]] * (len(buckets) - 1)), window_end=S + 70)
    assert r.sent_for(0) == [(7, S + 61, 1, 48)] and r.n_stored == 0 and r.next_task_time == IDLE


def test_argument_errors_leave_the_stage_as_it_was(engine):
    """A NULL array with offers, or a window_end below the previous one: SHD_ERR_INVALID before
    anything runs, and the next call works."""
    import torch
    from shadow_amd._native import ShdError
    stage = _stage(engine, [bucket()])
    stage.advance(window_end=S + 10)
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance(window_end=S + 9)
    d = torch.zeros(4, dtype=torch.int64, device="cuda")
    with pytest.raises(ShdError, match="INVALID"):
        stage.advance_device(d, d, None, d, d, d, d, 1, S + 20)
    r = stage.advance(*_arrays([[_P(S + 11, 1, 7)]]), window_end=S + 20)
    assert r.sent_for(0) == [(7, S + 11, 1, 48)]


def chain_case():
    """The chain's fixed parts: 64 hosts on 60 nodes, every path 60-70 ms with 2 % loss; outbound
    buckets of 125 kB/s (12 ms a full packet) on three hosts of four, inbound buckets of 20 kB/s
    (75 ms a full packet) on every second host."""
    from shadow_amd import synth
    H, NN = 64, 60
    rng = np.random.default_rng(51)
    lat = rng.integers(60 * MS, 70 * MS, (NN, NN)).astype(np.uint64)
    loss = np.full((NN, NN), 0.02, np.float32)
    out_b = [None if h % 4 == 3 else bucket(125_000) for h in range(H)]
    in_b = [bucket(20_000) if h % 2 else None for h in range(H)]
    return H, lat, loss, synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1), out_b, in_b


def chain_offers(k, ws, we, H, prio):
    """Window 0: every host offers a burst in the window's last two thirds (a tenth local);
    window 1: the hosts without an outbound bucket offer a few more, early; window 2: none."""
    rng = np.random.default_rng(60 + k)
    per_host = []
    pid = k * 100_000
    for h in range(H):
        n = int(rng.integers(2, 7)) if k == 0 else (int(rng.integers(0, 4)) if k == 1 and h % 4 == 3 else 0)
        lo, hi = (ws + (we - ws) // 3, we) if k == 0 else (ws, ws + (we - ws) // 2)
        times = np.sort(rng.integers(lo, hi, n)).tolist()
        offers = []
        for i, t in enumerate(times):
            dst = h if rng.random() < 0.1 else int(rng.integers(0, H))
            pay = int(rng.choice([0, 1448, 1448, int(rng.integers(1, 1449))]))
            offers.append((t, prio[h] + i, pay + HEADER, pay, dst, pid + i))
        prio[h] += n
        pid += n
        per_host.append(offers)
    return per_host


class ChainOracle:
    """outbound_model -> oracle.relay -> the oracle event queues -> inbound_model, one window per
    step; the next window from the restated controller."""

    def __init__(self, end_time):
        from oracle.relay import EventQueues, RunaheadState
        from tests.inbound_model import InboundModel
        self.H, self.lat, self.loss, self.host_node, rng0, out_b, in_b = chain_case()
        self.om, self.im = OutboundModel(out_b), InboundModel(in_b)
        self.rng, self.nid = rng0.copy(), np.zeros(self.H, np.uint64)
        self.q = EventQueues(self.H)
        self.ra = RunaheadState(True, int(self.lat.min()))
        self.end_time = end_time
        self.batches = []     # per relay round: (payload, sent_pkt) of its batch
        self.decided = []

    def step(self, arr, we):
        from oracle import relay as OR
        mo = self.om.advance(*arr, we, 0)
        status = np.zeros(0, np.uint8)
        if len(mo["sent_pkt"]):
            src = np.repeat(np.arange(self.H, dtype=np.uint32), np.diff(mo["src_off"].astype(np.int64)))
            rr = OR.relay_round(mo["send_time"], src, mo["dst_host"], mo["payload"], self.host_node, self.lat,
                                self.loss, self.rng, self.nid, we, self.end_time, 0)
            self.rng, self.nid, status = rr.rng_state, rr.next_event_id, rr.status
            if rr.min_latency != IDLE:
                self.ra.update_lowest_used_latency(rr.min_latency)
            self.q.push_round(rr.events, len(self.batches))
            self.batches.append((mo["payload"], mo["sent_pkt"]))
        off, ev = [0], []
        for h in range(self.H):
            ev += self.q.pop_until(h, we)
            off.append(len(ev))
        popped = dict(off=np.array(off, np.uint32), deliver=np.array([e[0] for e in ev], np.uint64),
                      src=np.array([e[1] for e in ev], np.uint32), seq=np.array([e[2] for e in ev], np.uint64),
                      tag=np.array([e[3] for e in ev], np.uint64))
        size, pkt = self.sizes(popped["tag"])
        mi = self.im.advance(popped["off"], popped["deliver"], size, pkt, we)
        heads = [t for t in (self.q.next_event_time(h) for h in range(self.H)) if t is not None]
        cands = dict(outbound=mo["next_task_time"], inbound=mi[5], queues=min(heads) if heads else IDLE)
        low = min(cands.values())
        self.decided.append([k for k, v in cands.items() if v == low])
        from oracle.relay import next_window
        return mo, status, popped, mi, next_window(None if low == IDLE else low, self.ra.get(), self.end_time)

    def sizes(self, tag):
        """A popped event's total size and packet id, from the batch its tag names."""
        b, i = (tag >> np.uint64(32)).astype(np.int64), (tag & np.uint64(0xFFFFFFFF)).astype(np.int64)
        size = np.array([self.batches[x][0][y] + HEADER for x, y in zip(b, i)], np.uint32)
        pkt = np.array([self.batches[x][1][y] for x, y in zip(b, i)], np.uint32)
        return size, pkt


def test_chain_outbound_relay_queues_inbound():
    """Three windows of OutboundStage.advance_device -> shd_relay_round_device (the engine's batch
    as it stands) -> shd_equeue_advance -> InboundStage.advance_device, the popped off / deliver
    arrays as they lie on the device, against the composed oracle: every status, event and record,
    and every window from shd_round_window fed the two stages' next_task_time.  After window 0 the
    outbound stage's task alone decides the next window's start (the events are 60 ms away), after
    window 2 the inbound stage's (the outbound side has drained, the queues are empty).  A fresh
    engine: the runahead and the queues are the context's."""
    import ctypes as C
    import torch
    from shadow_amd import _native as N
    from shadow_amd.equeue import EventQueues
    from shadow_amd.inbound import InboundStage
    from shadow_amd.outbound import OutboundStage
    from shadow_amd.relay import Relay
    from shadow_amd.rounds import Runahead, next_window as eng_window
    from shadow_amd.routing import Engine
    from tests.test_inbound_gpu import _same_state as _same_in_state
    end_time = S + 10**12
    o = ChainOracle(end_time)
    H = o.H
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    with Engine(0) as eng:
        _, _, _, _, rng0, out_b, in_b = chain_case()
        rl = Relay(o.host_node, rng0, np.zeros(H, np.uint64), o.lat, o.loss, engine=eng)
        q = EventQueues(eng, H)
        Runahead(eng, True, int(o.lat.min()))
        rows = lambda bs: [np.array([(0, 0, 0, S)[i] if b is None else b[i] for b in bs], np.uint64)  # noqa: E731
                           for i in range(4)]
        ostage = OutboundStage(eng, *rows(out_b), ring_capacity=64)
        istage = InboundStage(eng, *rows(in_b), ring_capacity=512)
        ws, we = S + 10**9, S + 10**9 + o.ra.get()
        prio = [0] * H
        for k in range(3):
            per_host = chain_offers(k, ws, we, H, prio)
            arr = _arrays(per_host) if any(per_host) else (None,) * 7
            mo, status, popped, mi, want_win = o.step(arr, we)
            ob = ostage.advance_device(*(None if a is None else dev(a, a.dtype.str.replace("u", "i")) for a in arr),
                                       0 if arr[0] is None else len(arr[1]), we)
            sent = ostage.sent(ob)
            _same(sent, mo)
            out = None
            if ob.n_sent:
                bufs = rl.device_buffers(ob.n_sent)
                out = N.RelayOut(*(N.ptr(bufs[x]).value for x in ("status", "ev_off", "ev_deliver", "ev_src",
                                                                   "ev_seq", "ev_pkt")), 0, 0, 0, 0, 0)
                rd = N.Round(we, end_time, 0)
                N.check(eng.lib.shd_relay_round_device(eng.ctx, C.byref(ob.batch), C.byref(rd), C.byref(out)),
                        "shd_relay_round_device")
                assert np.array_equal(bufs["status"][:ob.n_sent].cpu().numpy(), status)
                assert out.n_sent == int((status == 2).sum())
            eq = q.advance_device(out, we)
            p = q.popped(eq)
            for x in ("off", "deliver", "src", "seq", "tag"):
                assert np.array_equal(getattr(p, x), popped[x]), (k, x)
            size, pkt = o.sizes(p.tag)
            d_size, d_pkt = dev(size, np.int32), dev(pkt, np.int32)
            torch.cuda.synchronize()
            ib = istage.advance_device(eq.off, eq.deliver, d_size, d_pkt, eq.n_popped, we)
            rec = istage.records(ib)
            for got, want in zip((rec.off, rec.pkt, rec.time, rec.kind, rec.n_stored, rec.next_task_time), mi):
                assert np.array_equal(got, want), k
            for h in range(H):
                _same_state(ostage.state(h), o.om.hosts[h])
                _same_in_state(istage.state(h), o.im.hosts[h])
            cpu_next = min(ob.next_task_time, ib.next_task_time)
            win = eng_window(eng, None if cpu_next == IDLE else cpu_next, end_time)
            assert win == want_win, (k, win, want_win)
            ws, we = want_win
    assert o.decided[0] == ["outbound"] and o.decided[2] == ["inbound"], o.decided
    assert o.om.counters["blocks"] > 20 and o.om.counters["carried"] > 5 and o.om.counters["local_forwards"] > 5
    assert o.im.counters["blocks"] > 5 and o.im.counters["carried"] > 5
    assert len(o.batches) >= 2 and sum(len(b[1]) for b in o.batches) > 150


@pytest.mark.parametrize("n_hosts", [1, 70])
def test_empty_and_edge_shapes(engine, n_hosts):
    """One host and a host count that is no multiple of 64: a window without offers or tasks (no
    packets, offsets all zero; NULL inputs and empty arrays alike), then offers that leave tasks
    outstanding, a call with every output pointer NULL that runs them, and the state after it."""
    buckets = [bucket()] * n_hosts
    stage = _stage(engine, buckets)
    model = OutboundModel(buckets)
    empty = (np.zeros(n_hosts + 1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint64)) + \
        (np.zeros(0, np.uint32),) * 4
    for arr in (None, empty):
        r = stage.advance(*(arr or ()), window_end=S + 5)
        assert len(r.sent_pkt) == len(r.loc_pkt) == 0
        assert r.src_off.tolist() == r.loc_off.tolist() == [0] * (n_hosts + 1)
        assert (r.n_stored, r.next_task_time) == (0, IDLE)
    per_host = [[(S + 5 + h, 1, 1500, 1448, n_hosts, 2 * h), (S + 6 + h, 2, 1500, 1448, n_hosts, 2 * h + 1)]
                for h in range(n_hosts)]
    arr = _arrays(per_host)
    _same(stage.advance(*arr, window_end=S + MS), model.advance(*arr, S + MS))
    none = (None,) * 7
    st = engine.lib.shd_outbound_advance(engine.ctx, *none, 0, S + 3000 * MS, 0, *(None,) * 8)
    assert st == 0
    model.advance(*none, S + 3000 * MS)
    assert model.counters["carried"] == n_hosts
    for h in {0, n_hosts - 1}:
        _same_state(stage.state(h), model.hosts[h])
        assert stage.state(h)["task_time"] is None and stage.state(h)["bucket"]["balance"] == 0
    st = engine.lib.shd_outbound_get_state(engine.ctx, 0, *(None,) * 7)
    assert st == 0
    r = stage.advance(window_end=S + 3001 * MS)
    assert len(r.sent_pkt) == 0 and r.n_stored == 0
