"""CPU tier of the outbound stage: the model (tests/outbound_model.py, a heapq by packet priority
and the oracle's TokenBucket composed as the interface's FIFO discipline -> Relay -> forward task
composes them) pinned on hand vectors, each derivable by reading relay/mod.rs and token_bucket.rs.
tests/test_outbound_gpu.py runs the same cases on the device."""
from oracle.token_bucket import SIM_START as S, TokenBucket, create_token_bucket
from tests.outbound_model import IDLE, LOCAL, SENT, OutboundModel

MS = 10**6


def bucket(bps=1000, last=S):
    return (*create_token_bucket(bps), last)


def payload_of(pkt):
    """The pass-through value the hand cases give packet ``pkt``."""
    return 1000 + pkt


def arrays(per_host):
    """[[(time, prio, size, dst, pkt)] per host] -> off, time, prio, size, payload, dst, pkt lists."""
    off = [0]
    for e in per_host:
        off.append(off[-1] + len(e))
    flat = [x for e in per_host for x in e]
    return (off, [x[0] for x in flat], [x[1] for x in flat], [x[2] for x in flat], [payload_of(x[4]) for x in flat],
            [x[3] for x in flat], [x[4] for x in flat])


def records(r, h=0):
    """Host h's (kind, pkt, time) of a model result: the SENT ones, then the LOCAL ones."""
    a, b = int(r["src_off"][h]), int(r["src_off"][h + 1])
    c, d = int(r["loc_off"][h]), int(r["loc_off"][h + 1])
    return ([(SENT, int(p), int(t)) for p, t in zip(r["sent_pkt"][a:b], r["send_time"][a:b])] +
            [(LOCAL, int(p), int(t)) for p, t in zip(r["loc_pkt"][c:d], r["loc_time"][c:d])])


def one_host(b, first_host=0):
    """A one-host model and step(offers, window_end, bootstrap_end) -> (records, n_stored, next
    task) with every time an offset from S (offers: [(time, prio, size, dst, pkt)])."""
    m = OutboundModel([b], first_host)
    dst_of = {}

    def step(offers, window_end, bootstrap_end=0):
        dst_of.update({p: d for _, _, _, d, p in offers})
        r = m.advance(*arrays([[(S + t, pr, s, d, p) for t, pr, s, d, p in offers]]), S + window_end, bootstrap_end)
        a, b_ = int(r["src_off"][0]), int(r["src_off"][1])
        assert r["dst_host"][a:b_].tolist() == [dst_of[int(p)] for p in r["sent_pkt"][a:b_]]
        assert r["payload"][a:b_].tolist() == [payload_of(int(p)) for p in r["sent_pkt"][a:b_]]
        nxt = r["next_task_time"]
        return [(k, p, t - S) for k, p, t in records(r)], r["n_stored"], (None if nxt == IDLE else nxt - S)
    return m, step


# the hand cases, shared with the device tests: (bucket, first_host, [(offers, window_end,
# bootstrap_end, records (SENT first, then LOCAL), n_stored, next task)], checks on the final state)
T0 = 5 * MS + 300
TWO = [(0, 1, 1500, 1, 0), (0, 2, 1500, 1, 1)]   # two full packets at S on a 1000 B/s bucket (1501, 1, 1 ms)
A1 = (TWO, 10 * MS, 0, [(SENT, 0, 0)], 1, 1499 * MS)
CASES = {
    # 125 kB/s = (1625, 125, 1 ms).  p10 leaves at t0 (the bucket is full: 1625 - 1500 = 125); p11
    # misses 1375 = 11 refills: 999 700 ns to the next one + 10 ms.  At t0 + 10 999 700 = S + 16 ms
    # the bucket holds 1500: p11 leaves, 0 left; p13 (priority 3) overtakes p12 (priority 4) and
    # misses 1500 = 12 refills from a refill boundary: 12 ms.  The local p12 waits behind the cached
    # head and is forwarded right after it, bucket empty.
    "priority_and_head_of_line": (bucket(125_000), 0, [
        ([(T0, 1, 1500, 1, 10), (T0, 2, 1500, 1, 11), (T0 + 2 * MS, 4, 1500, 0, 12), (T0 + 3 * MS, 3, 1500, 1, 13)],
         T0 + 30 * MS, 0,
         [(SENT, 10, T0), (SENT, 11, T0 + 10_999_700), (SENT, 13, T0 + 22_999_700), (LOCAL, 12, T0 + 22_999_700)],
         0, None)], dict(task=None, cached=None, balance=0, queue_len=0)),
    "unlimited": (None, 0, [([(5, 1, 1500, 1, 0), (5, 2, 1500, 1, 1), (9, 3, 10, 1, 2)], 10, 0,
                             [(SENT, 0, 5), (SENT, 1, 5), (SENT, 2, 9)], 0, None)],
                  dict(task=None, cached=None, queue_len=0)),
    "bootstrap": (bucket(), 0, [(TWO, 10 * MS, S + MS, [(SENT, 0, 0), (SENT, 1, 0)], 0, None)],
                  dict(task=None, cached=None, balance=1501, queue_len=0)),
    # p1 misses 1499 tokens of 1 per ms: the task is carried over an empty window and runs in the third
    "carried_over_two_windows": (bucket(), 0, [A1, ([], 1000 * MS, 0, [], 1, 1499 * MS),
                                               ([], 2000 * MS, 0, [(SENT, 1, 1499 * MS)], 0, None)],
                                 dict(task=None, cached=None, balance=0, queue_len=0)),
    "carried_blocked": (bucket(), 0, [A1], dict(task=1499 * MS, cached=1, balance=1, queue_len=0)),
    # p2 is offered at exactly the carried task's time: inserted first, so that task forwards p1
    # and then weighs p2 (60 tokens: 60 ms); p3 one ns later waits in the queue
    "offer_at_the_tasks_time": (bucket(), 0, [A1, ([(1499 * MS, 3, 60, 1, 2), (1499 * MS + 1, 4, 60, 1, 3)],
                                                   1600 * MS, 0, [(SENT, 1, 1499 * MS), (SENT, 2, 1559 * MS)],
                                                   1, 1619 * MS)],
                                dict(task=1619 * MS, cached=3, balance=0, queue_len=0)),
    # the bucket holds 1 token after p0; the local p1 is forwarded all the same, p2 blocks:
    # 1499 refills from 6 ns after a boundary
    "local_with_an_empty_bucket": (bucket(), 7, [([(0, 1, 1500, 1, 0), (5, 2, 1500, 7, 1), (6, 3, 1500, 8, 2)],
                                                  10 * MS, 0, [(SENT, 0, 0), (LOCAL, 1, 5)], 1, 1499 * MS)],
                                   dict(task=1499 * MS, cached=2, balance=1, queue_len=0)),
}


def check_final(want, task, cached, balance, queue_len):
    """The case's checks against a host's final state (times as offsets from S)."""
    assert task == want["task"]
    assert cached == want["cached"]
    assert queue_len == want["queue_len"]
    if "balance" in want:
        assert balance == want["balance"]


def run_case(name):
    b, first, steps, final = CASES[name]
    m, step = one_host(b, first)
    for offers, w_end, boot, recs, n_stored, nxt in steps:
        assert step(offers, w_end, boot) == (recs, n_stored, nxt), name
    h = m.hosts[0]
    check_final(final, None if h.task is None else h.task - S, None if h.cached is None else h.cached[1],
                h.tb.balance if h.tb is not None else None, len(h.q))
    return m


def test_priority_order_and_head_of_line_blocking():
    m = run_case("priority_and_head_of_line")
    assert m.counters["out_of_order"] == 1 and m.counters["local_forwards"] == 1 and m.counters["blocks"] == 2


def test_the_hand_vector_against_the_oracles_bucket():
    """The two blocking durations of the case above, from the oracle's TokenBucket alone."""
    tb = TokenBucket(*bucket(125_000))
    assert tb.conforming_remove(1500, S + T0) == (True, 125)
    assert tb.conforming_remove(1500, S + T0) == (False, 10_999_700)
    assert tb.conforming_remove(1500, S + T0 + 10_999_700) == (True, 0)
    assert tb.conforming_remove(1500, S + T0 + 10_999_700) == (False, 12 * MS)
    assert tb.conforming_remove(1500, S + T0 + 22_999_700) == (True, 0)


def test_no_bucket_sends_at_each_notify():
    run_case("unlimited")


def test_bootstrapping_bypasses_the_bucket():
    m = run_case("bootstrap")
    assert m.counters["boot_forwards"] == 2 and m.counters["blocks"] == 0


def test_a_task_is_carried_over_two_windows():
    run_case("carried_blocked")
    m = run_case("carried_over_two_windows")
    assert m.counters["carried"] == 2


def test_offer_at_the_tasks_own_time_is_inserted_before_the_task_runs():
    m = run_case("offer_at_the_tasks_time")
    assert m.counters["ties"] == 2   # p1 at p0's task (both at 0), p2 at the carried task's time


def test_local_packet_is_forwarded_when_the_bucket_is_empty():
    m = run_case("local_with_an_empty_bucket")
    assert m.counters["local_forwards"] == 1 and m.hosts[0].tb.balance == 1


def test_local_detection_uses_the_global_id():
    """The same offers on a host whose global id is not 7: dst 7 is a remote packet and blocks."""
    _, step = one_host(bucket(), 0)
    assert step([(0, 1, 1500, 1, 0), (5, 2, 1500, 7, 1), (6, 3, 1500, 8, 2)], 10 * MS) == \
        ([(SENT, 0, 0)], 2, 1499 * MS)


def test_task_at_window_end_stays_outstanding():
    """A task exactly at window_end is not run (T < window_end); the next window runs it."""
    _, step = one_host(bucket())
    assert step(TWO, 10 * MS) == ([(SENT, 0, 0)], 1, 1499 * MS)
    assert step([], 1499 * MS) == ([], 1, 1499 * MS)
    assert step([], 1499 * MS + 1) == ([(SENT, 1, 1499 * MS)], 0, None)
