"""GPU parity of the inbound stage (shadow_amd/inbound.py, csrc/inbound.hip) against the CPU model
(tests/inbound_model.py): records, offsets, the stored total, the next task time and the per-host
state, exactly."""
import numpy as np
import pytest

from oracle.token_bucket import SIM_START as S, create_token_bucket
from tests.inbound_model import IDLE, InboundModel
from tests.test_inbound import CASES, MS, bucket, check_final

pytestmark = pytest.mark.gpu

HEADER = 52   # chain test: total size = HEADER + payload; 1448 + 52 = CONFIG_MTU, within every bucket


def _stage(engine, buckets, ring=512):
    from shadow_amd.inbound import InboundStage
    rows = [(0, 0, 0, S) if b is None else b for b in buckets]
    cap, inc, itv, last = (np.array([r[i] for r in rows], np.uint64) for i in range(4))
    return InboundStage(engine, cap, inc, itv, last, ring_capacity=ring)


def _arrays(per_host):
    """[[(time, size, pkt)] per host] -> off, time, size, pkt."""
    off = np.zeros(len(per_host) + 1, np.uint32)
    off[1:] = np.cumsum([len(e) for e in per_host])
    flat = [x for e in per_host for x in e]
    return (off, np.array([t for t, _, _ in flat], np.uint64), np.array([s for _, s, _ in flat], np.uint32),
            np.array([p for _, _, p in flat], np.uint32))


def _same_records(r, want):
    o_off, o_pkt, o_time, o_kind, n_stored, nxt = want
    assert np.array_equal(r.off, o_off)
    assert np.array_equal(r.kind, o_kind)
    assert np.array_equal(r.pkt, o_pkt)
    assert np.array_equal(r.time, o_time)
    assert (r.n_stored, r.next_task_time) == (n_stored, nxt)


def _same_state(st, host):
    q = host.q
    assert st["task_time"] == host.task
    assert st["cached"] == (None if host.cached is None else (host.cached, host.size[host.cached]))
    assert st["codel"] == {"len": len(q), "mode": q.mode, "interval_end": q.interval_end, "drop_next": q.drop_next,
                           "current_drop_count": q.current_drop_count,
                           "previous_drop_count": q.previous_drop_count,
                           "total_bytes_stored": q.total_bytes_stored}
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
    b, steps, final = CASES[name]
    stage = _stage(engine, [b])
    model = InboundModel([b])
    for events, w_end, boot, recs, n_stored, nxt in steps:
        ev = [(S + t, s, p) for t, s, p in events]
        r = stage.advance(*_arrays([ev]), window_end=S + w_end, bootstrap_end=boot)
        assert r.off.tolist() == [0, len(recs)]
        assert r.records_for(0) == [(k, p, S + t) for k, p, t in recs]
        assert (r.n_stored, r.next_task_time) == (n_stored, IDLE if nxt is None else S + nxt)
        model.advance(*_arrays([ev]), S + w_end, boot)
    st = stage.state(0)
    check_final(final, None if st["task_time"] is None else st["task_time"] - S,
                None if st["cached"] is None else st["cached"][0],
                None if st["bucket"] is None else st["bucket"]["balance"], st["codel"])
    _same_state(st, model.hosts[0])


def test_from_bandwidth(engine):
    """InboundStage.from_bandwidth: create_token_bucket per host, None or a negative entry for a
    host without a bucket.  Case A1 on the 1000 B/s host, case E's events on the two others."""
    from shadow_amd.inbound import InboundStage
    stage = InboundStage.from_bandwidth(engine, [1000, None, -1, 0], S, ring_capacity=16)
    burst = [(S + 5, 1500, p) for p in range(3)]
    r = stage.advance(*_arrays([[(S, 1500, 10), (S, 1500, 11)], burst, [(t, s, p + 3) for t, s, p in burst], []]),
                      window_end=S + 10 * MS)
    assert r.records_for(0) == [(1, 10, S)] and r.next_task_time == S + 1499 * MS and r.n_stored == 1
    assert r.records_for(1) == [(1, p, S + 5) for p in range(3)]
    assert r.records_for(2) == [(1, p, S + 5) for p in range(3, 6)]
    want = dict(zip(("capacity", "refill_increment", "refill_interval"), create_token_bucket(1000)))
    b = stage.state(0)["bucket"]
    assert {k: b[k] for k in want} == want and (b["balance"], b["last_refill"]) == (1, S)
    assert stage.state(1)["bucket"] is None and stage.state(2)["bucket"] is None
    b = stage.state(3)["bucket"]   # a rate of 0 is still a bucket: 1 byte per ms
    assert (b["capacity"], b["refill_increment"], b["balance"]) == (1501, 1, 1501)


RATES = [0, 1000, 20_000, 125_000, 1_250_000, 125_000_000]


def _random_window(rng, model, start, end, pid):
    per_host = []
    for host in model.hosts:
        n = int(rng.integers(0, 40))
        times = np.sort(rng.integers(start, end, n)).tolist()
        if n >= 2 and rng.random() < 0.5:
            times[1] = times[0]
        if n and host.task is not None and start <= host.task < end and rng.random() < 0.5:
            times[int(rng.integers(0, n))] = host.task   # an event at exactly the outstanding task's time
            times.sort()
        per_host.append([(t, int(rng.integers(1, 1501)), pid + i) for i, t in enumerate(times)])
        pid += n
    return per_host, pid


@pytest.mark.parametrize("seed", range(6))
def test_random_windows_vs_model(engine, seed):
    """Five consecutive windows over up to 199 hosts with mixed buckets: every record of every
    window, then every host's state.  The model's counters show that each branch ran: blocks,
    tasks carried across a call, event/task ties, bootstrapped forwards, CoDel drops."""
    rng = np.random.default_rng(900 + seed)
    n_hosts = int(rng.integers(1, 200))
    buckets = [None if rng.random() < 0.1 else (*create_token_bucket(int(rng.choice(RATES))), S)
               for _ in range(n_hosts)]
    stage = _stage(engine, buckets, ring=512)
    model = InboundModel(buckets)
    start, pid = S, 0
    for _ in range(5):
        end = start + int(rng.choice([1, 20, 150, 400])) * MS
        per_host, pid = _random_window(rng, model, start, end, pid)
        arr = _arrays(per_host)
        want = model.advance(*arr, end, S + 30 * MS)
        _same_records(stage.advance(*arr, window_end=end, bootstrap_end=S + 30 * MS), want)
        start = end
    for h in range(n_hosts):
        _same_state(stage.state(h), model.hosts[h])
    for k, v in model.counters.items():
        assert v > 0, (k, model.counters)
    assert 0 < model.max_depth <= 512


def test_many_hosts_past_one_scan_tile(engine):
    """9001 hosts: more than one 8192-entry tile in both scans (region bounds, record offsets) and
    36 workgroups of lanes; two windows, a quarter of the hosts blocked across them."""
    rng = np.random.default_rng(77)
    n_hosts = 9001
    buckets = [bucket(1000) if h % 4 == 0 else (None if h % 4 == 1 else bucket(125_000)) for h in range(n_hosts)]
    stage = _stage(engine, buckets, ring=8)
    model = InboundModel(buckets)
    start, pid = S, 0
    for win in (20 * MS, 4000 * MS):
        per_host = []
        for h in range(n_hosts):
            n = int(rng.integers(0, 4))
            times = np.sort(rng.integers(start, start + 20 * MS, n)).tolist()
            per_host.append([(t, 1500, pid + i) for i, t in enumerate(times)])
            pid += n
        arr = _arrays(per_host)
        want = model.advance(*arr, start + win, 0)
        _same_records(stage.advance(*arr, window_end=start + win), want)
        start += win
    assert model.counters["blocks"] > 500 and model.counters["carried"] > 500
    for h in (0, 1, 2, 4096, 8191, 8192, 9000):
        _same_state(stage.state(h), model.hosts[h])


BAD = {
    "event_at_window_end": ([bucket()], 4, [([[(S + 10, 100, 0)]], S + 10)]),
    # the relay is blocked, its task carried past the window's end (case A1), and the event lies
    # beyond that task: the check must not depend on the event being weighed against the task
    "event_past_window_end_behind_a_carried_task":
        ([bucket()], 4, [([[(S, 1500, 0), (S, 1500, 1)]], S + 10 * MS), ([[(S + 1500 * MS, 100, 2)]], S + 20 * MS)]),
    "event_at_window_end_behind_a_carried_task":
        ([bucket()], 4, [([[(S, 1500, 0), (S, 1500, 1)]], S + 10 * MS), ([[(S + 20 * MS, 100, 2)]], S + 20 * MS)]),
    "decreasing_time": ([bucket()], 4, [([[(S + 5, 100, 0), (S + 4, 100, 1)]], S + 10)]),
    "before_the_last_window": ([bucket()], 4, [([[(S + 5, 100, 0)]], S + 10), ([[(S + 9, 100, 1)]], S + 20)]),
    "size_above_capacity": ([bucket()], 4, [([[(S + 5, 1502, 0)]], S + 10)]),
    # capacity 4: p1 is cached behind p0, then five pushes before its task runs
    "ring_overflow": ([bucket()], 4, [([[(S, 1500, 0), (S, 1500, 1)]], S + 10),
                                      ([[(S + 20 + i, 100, 2 + i) for i in range(5)]], S + 100)]),
    "offsets_not_a_csr": ([bucket(), bucket()], 4, [("raw", S + 10)]),
}


@pytest.mark.parametrize("name", list(BAD))
def test_contract_errors(engine, name):
    """Each violation is SHD_ERR_INVALID from a check (no lane may spin or read out of range), the
    next call SHD_ERR_STATE, and a fresh setup works again."""
    from shadow_amd._native import ShdError
    buckets, ring, steps = BAD[name]
    stage = _stage(engine, buckets, ring=ring)
    for per_host, w_end in steps[:-1]:
        stage.advance(*_arrays(per_host), window_end=w_end)
    per_host, w_end = steps[-1]
    if per_host == "raw":   # host 0's range runs past host 1's
        arr = (np.array([0, 3, 2], np.uint32), np.full(2, S + 1, np.uint64), np.full(2, 100, np.uint32),
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
    r = stage.advance(*_arrays([[(S + 1, 100, 7)]] + [[]] * (len(buckets) - 1)), window_end=S + 10)
    assert r.records_for(0) == [(1, 7, S + 1)] and r.n_stored == 0 and r.next_task_time == IDLE


def test_chain_from_the_event_queues(engine):
    """One relay round on a golden-sized routing graph -> shd_equeue_advance -> shd_inbound_advance
    fed the popped off / deliver arrays as they lie on the device; size and packet id gathered on
    the device from the popped tags.  Half the hosts have a 1000 B/s bucket, so packets block and
    carry into a second window.  Against the model fed from shd_equeue_copy_popped."""
    import torch
    from oracle import corc
    from shadow_amd import synth
    from shadow_amd.equeue import EventQueues
    from shadow_amd.relay import Relay
    H, P, NN = 64, 2000, 60
    el = synth.complete_graph(NN, 31)
    used = np.arange(NN, dtype=np.uint32)
    code, lat, loss, _ = corc.routing(NN, el.src, el.dst, el.latency_ns, el.packet_loss, False, used)
    assert code == "OK"
    rl = Relay(synth.c5_host_nodes(H, NN), synth.host_rng_states(H, 1), np.zeros(H, np.uint64), lat, loss,
               engine=engine)
    q = EventQueues(engine, H)
    buckets = [bucket(1000) if h % 2 else None for h in range(H)]
    stage = _stage(engine, buckets, ring=512)
    model = InboundModel(buckets)
    start, win = S + 10**9, 50 * MS
    b = synth.packet_batch(H, P, start, start + win, seed=41)
    dev = lambda a, dt: torch.from_numpy(np.ascontiguousarray(a).view(dt)).cuda()  # noqa: E731
    d = [dev(b.src_off, np.int32), dev(b.send_time, np.int64), dev(b.dst_host, np.int32), dev(b.payload, np.int32)]
    torch.cuda.synchronize()
    bufs = rl.device_buffers(P)
    out = rl.round_device(*d, start + win, start + 10**12, 0, bufs)
    w_end = start + 400 * MS   # every path is below 300 ms + the 50 ms round: all events pop
    eq = q.advance_device(out, w_end)
    p = q.popped(eq)
    assert eq.n_popped == out.n_sent > 1000 and p.n_pending == 0
    d_idx = dev(p.tag & np.uint64(0xFFFFFFFF), np.int64)
    d_size = (d[3].long()[d_idx] + HEADER).int()
    d_pkt = d_idx.int()
    torch.cuda.synchronize()
    got = stage.records(stage.advance_device(eq.off, eq.deliver, d_size, d_pkt, eq.n_popped, w_end))
    pkt = (p.tag & np.uint64(0xFFFFFFFF)).astype(np.uint32)
    want = model.advance(p.off, p.deliver, b.payload[pkt] + HEADER, pkt, w_end)
    _same_records(got, want)
    assert model.counters["blocks"] >= 16 and got.n_stored > 100 and got.next_task_time < IDLE
    # the carried packets leave in a later window without new events
    _same_records(stage.advance(window_end=w_end + 4000 * 10**9), model.advance(None, None, None, None,
                                                                               w_end + 4000 * 10**9))
    assert model.counters["carried"] > 10
    for h in range(H):
        _same_state(stage.state(h), model.hosts[h])


@pytest.mark.parametrize("n_hosts", [1, 70])
def test_empty_and_edge_shapes(engine, n_hosts):
    """One host and a host count that is no multiple of 64: a window without events or tasks (no
    records, offsets all zero), then events that leave tasks outstanding, then a window of no
    events that runs them."""
    buckets = [bucket()] * n_hosts
    stage = _stage(engine, buckets)
    model = InboundModel(buckets)
    for arr in (None, (np.zeros(n_hosts + 1, np.uint32), np.zeros(0, np.uint64), np.zeros(0, np.uint32),
                       np.zeros(0, np.uint32))):
        r = stage.advance(*(arr or ()), window_end=S + 5)
        assert len(r.pkt) == 0 and r.off.tolist() == [0] * (n_hosts + 1)
        assert (r.n_stored, r.next_task_time) == (0, IDLE)
    per_host = [[(S + 5 + h, 1500, 2 * h), (S + 6 + h, 1500, 2 * h + 1)] for h in range(n_hosts)]
    arr = _arrays(per_host)
    _same_records(stage.advance(*arr, window_end=S + MS), model.advance(*arr, S + MS))
    r = stage.advance(window_end=S + 3000 * MS)
    _same_records(r, model.advance(None, None, None, None, S + 3000 * MS))
    assert len(r.pkt) == n_hosts and r.n_stored == 0 and model.counters["carried"] == n_hosts
